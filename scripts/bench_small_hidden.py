#!/usr/bin/env python3
"""Run ON THE GPU BOX: the synthetic study's ACM-GCN at the study's hidden width 32 (synthetic-experiments/arg_parser.py:40)
and at 64, on a study-shaped workload -- ``synthetic.generate_graph("random", 5, 400, ...)`` (2 000 nodes), sparse
bag-of-words-like features (1 433 columns, ~1.3 % density, row-normalised; Cora's own are not in the checkout),
``baselines.GCN(1433, hidden, 5, 0.5, "acmgcn", nnodes=n)`` (the study's ACM dialect: attn_layernorm=False), FusedAdam.

    python scripts/bench_small_hidden.py [--label NAME] [--hidden 32,64] [--out profiles/small_hidden.jsonl]

Public API only, so the same file runs on a checkout from before the small-graph step took width 32 (there width 32 trains
on the general path: ``small`` is false in its lines).  One JSON line per (hidden, arm), appended to ``--out``:

    step            the captured TrainStep: after ``--warm`` seconds of replays, ``--windows`` windows of ``--steps`` replays,
                    each a host clock around replays that end in a device synchronise -> median / min / max ms per step
    fit             ``train.fit(use_graph=True, sync_every=32)``: ms per epoch (training step + evaluation pass + selection)
    fit_concurrent2 ``train.fit_concurrent(streams=2, sync_every=32)`` over ``--runs`` runs: ms per run-epoch
    fit_batched/B   ``train.fit_batched(batch=B, sync_every=32)`` over the same runs: ms per run-epoch, with
                    ``fit_batched.last_refusal`` (not None: the call was its fallback, fit_concurrent)

The fit arms are DIFFERENCES of two calls from the same initial state (``--base`` and ``--base + --epochs`` epochs), so plan
construction and captures cancel -- to within their own jitter, a few milliseconds, more after an arm that built 32 models.  So
the timed difference is made large against that: 6 400 epochs of one run (0.3-0.6 s), 640 epochs of 32 runs (0.6-2 s); the
models of a call are built, the garbage of the previous call collected and the device synchronised BEFORE the clock starts.
The rule is "max_val_acc", under which a run uses its whole budget; ``--repeats`` rounds visit the arms in turn.  ``spread`` =
(max - min) / median of an arm's samples.

A/A control: on a checkout where ``fit_batched`` falls back at width 32 (``refusal`` not None) its arm IS
``fit_concurrent(streams=2, sync_every=32)``; the two arms must then agree within their spreads, or the protocol is measuring
itself.  No threshold; nothing here means anything without the GPU."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import acm_gnn_amd  # noqa: E402
from acm_gnn_amd import FusedAdam, baselines, data as D, functional as AF, synthetic as S, train as T  # noqa: E402

DEV = torch.device("cuda:0")
SYNC = 32
F_IN, CLASSES, DENSITY = 1433, 5, 0.013


def workload(hidden):
    g = S.generate_graph("random", CLASSES, 400, degree_intra=2, edge_homo=0.3, seed=0, device=DEV)
    rng = np.random.default_rng(1433)
    x_np = D.row_normalize_features((rng.random((g.n, F_IN)) < DENSITY).astype(np.float32))
    x = acm_gnn_amd.SparseFeatures.from_scipy(sp.csr_matrix(x_np), DEV)

    def make(seed=0):
        torch.manual_seed(seed)
        model = baselines.GCN(F_IN, hidden, CLASSES, 0.5, "acmgcn", nnodes=g.n).to(DEV)
        model.fused_dropout, model.dropout_state = True, AF.DropoutState(DEV, seed=7 + seed)
        return model, FusedAdam(model.parameters(), lr=0.05, weight_decay=5e-4)
    return dict(ops=g.operators(), x=x, y=g.labels, n=g.n, make=make, nnz_x=int(x_np.astype(bool).sum()))


def splits(n, seed=0):
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).to(DEV)
    return idx[: int(0.6 * n)], idx[int(0.6 * n): int(0.8 * n)], idx[int(0.8 * n):]


def stats(v):
    med = statistics.median(v)
    return dict(ms=round(med, 5), min=round(min(v), 5), max=round(max(v), 5), spread=round((max(v) - min(v)) / med, 4))


def bench_step(w, args):
    model, opt = w["make"]()
    tr, _, _ = splits(w["n"])
    step = T.TrainStep(model, opt, w["x"], w["ops"], w["y"], T.row_weights(tr, w["n"], device=DEV), use_graph=True)
    small = getattr(step, "small", None) is not None
    t_end = time.perf_counter() + args.warm
    while time.perf_counter() < t_end:
        for _ in range(50):
            step()
        torch.cuda.synchronize()
    v = []
    for _ in range(args.windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            step()
        torch.cuda.synchronize()
        v.append((time.perf_counter() - t0) / args.steps * 1e3)
    return dict(small=small, refused=getattr(step, "small_refused", None), steps=args.steps, windows=args.windows, **stats(v))


def timed(w, arm, epochs, n_runs):
    runs = [w["make"](k) + splits(w["n"], k) for k in range(1 if arm == "fit" else n_runs)]
    gc.collect()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    refusal = None
    if arm == "fit":
        model, opt, tr, va, te = runs[0]
        T.fit(model, opt, w["x"], w["ops"], w["y"], tr, va, te, epochs, rule="max_val_acc", use_graph=True, sync_every=SYNC)
    elif arm == "fit_concurrent2":
        T.fit_concurrent(runs, w["x"], w["ops"], w["y"], epochs, rule="max_val_acc", streams=2, sync_every=SYNC)
    else:
        T.fit_batched(runs, w["x"], w["ops"], w["y"], epochs, rule="max_val_acc", batch=int(arm.split("/")[1]), sync_every=SYNC)
        refusal = T.fit_batched.last_refusal
    torch.cuda.synchronize()
    return time.perf_counter() - t0, refusal


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="head", help="what the lines are tagged with (e.g. head / parent)")
    ap.add_argument("--hidden", default="32,64")
    ap.add_argument("--warm", type=float, default=2.0, help="seconds of replays before the step windows")
    ap.add_argument("--windows", type=int, default=9)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--epochs", type=int, default=6400)
    ap.add_argument("--base", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--runs", type=int, default=32)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--batched-hidden", default="32", help="widths that also get the fit_concurrent2 / fit_batched arms")
    ap.add_argument("--batched-epochs", type=int, default=640)
    ap.add_argument("--arms", default="step,fit,sweep", help="step, fit, sweep (= fit_concurrent2 + fit_batched)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "small_hidden.jsonl"))
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error("--repeats: at least 3 rounds")
    out = open(args.out, "a")

    def emit(**rec):
        line = json.dumps(dict(label=args.label, device=torch.cuda.get_device_name(0), **rec))
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    batched_hidden = [int(h) for h in args.batched_hidden.split(",") if h]
    for hidden in [int(h) for h in args.hidden.split(",")]:
        w = workload(hidden)
        shape = dict(hidden=hidden, n=w["n"], nnz_a=int(w["ops"].low.nnz), f_in=F_IN, nnz_x=w["nnz_x"], classes=CLASSES)
        if "step" in args.arms.split(","):
            emit(arm="step", **shape, **bench_step(w, args))
        arms = [("fit", args.epochs, 1)] if "fit" in args.arms.split(",") else []
        if hidden in batched_hidden and "sweep" in args.arms.split(","):
            arms += [("fit_concurrent2", args.batched_epochs, args.runs), (f"fit_batched/{args.batch}", args.batched_epochs, args.runs)]
        samples, refusals = {a: [] for a, _, _ in arms}, {}
        for a, _, n_runs in arms:                         # warm-up: allocator pools, lazy handles
            timed(w, a, args.base, n_runs)
        for _ in range(args.repeats):
            for a, epochs, n_runs in arms:
                short, _ = timed(w, a, args.base, n_runs)
                long, refusals[a] = timed(w, a, args.base + epochs, n_runs)
                samples[a].append((long - short) / (epochs * n_runs) * 1e3)
        for a, epochs, n_runs in arms:
            emit(arm=a, **shape, runs=n_runs, epochs=epochs, base=args.base, sync_every=SYNC, refusal=refusals[a], **stats(samples[a]))


if __name__ == "__main__":
    main()
