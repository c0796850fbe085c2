#!/usr/bin/env python3
"""Run ON THE GPU BOX: ACM-GCN++ (``GCN(..., "acmgcnpp")``, init_layers_X = 1) on the small graphs the reference trains it on --
the Cora, Chameleon and Squirrel structures of tests/golden with the feature widths and dropouts scripts/bench_configs.py gives
them (Cora's and Squirrel's own feature matrices; Chameleon's are not in the checkout: a Bernoulli matrix of its width at
Squirrel's density), CSR features, hidden 64, FusedAdam -- and on the study-shaped 2 000-node workload of
scripts/bench_small_hidden.py at hidden 32.  As a regression arm, cora/acmgcn (a model without the residual branch).

    python scripts/bench_small_residual.py [--label NAME] [--round K] [--out profiles/small_residual.jsonl]
    python scripts/bench_small_residual.py --summarize profiles/small_residual.jsonl

Public API only, so the same file runs on a checkout from before the small-graph step took the model (there acmgcnpp trains on
the general path: ``small`` is false in its lines).  The protocol is bench_small_hidden.py's: one JSON line per (workload, arm),

    step   the captured TrainStep: after ``--warm`` seconds of replays, ``--windows`` windows of ``--steps`` replays, each a
           host clock around replays that end in a device synchronise -> median / min / max ms per step
    fit    ``train.fit(use_graph=True, sync_every=32)``: ms per epoch (training step + evaluation pass + selection), the
           DIFFERENCE of two calls from the same initial state (``--base`` and ``--base + --epochs`` epochs), ``--repeats`` times

``spread`` = (max - min) / median of an arm's samples.  Two checkouts are compared by ALTERNATING processes of the two in one
session (``--label parent`` / ``--label head``, ``--round`` 1, 2, ...), and the A/A control is a second head process per round
(``--label head_aa``): head and head_aa must agree within their spreads, or the protocol is measuring itself.
``--summarize`` pools the rounds of a file per (workload, arm, label).  No threshold; nothing here means anything without the GPU."""
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
GOLDEN = os.path.join(ROOT, "tests", "golden")
SYNC = 32
# graph, f_in, classes, model_type, structure_info, dropout, hidden (scripts/bench_configs.py: configs 1-3)
WORKLOADS = {
    "cora/acmgcnpp": ("cora", 1433, 7, "acmgcnpp", 0, 0.6, 64),
    "chameleon/acmgcnpp+A": ("chameleon", 2325, 5, "acmgcnpp", 1, 0.7, 64),
    "squirrel/acmgcnpp+A": ("squirrel", 2089, 5, "acmgcnpp", 1, 0.6, 64),
    "study2000/acmgcnpp/h32": ("study", 1433, 5, "acmgcnpp", 0, 0.5, 32),
    "cora/acmgcn": ("cora", 1433, 7, "acmgcn", 0, 0.6, 64),                 # the regression arm: no residual branch
}


def _graph(name):
    g = np.load(os.path.join(GOLDEN, f"graph_{name}.npz"))
    n = int(g["n"])
    adj = sp.csr_matrix((np.ones(len(g["adj_un_indices"]), np.float32), g["adj_un_indices"], g["adj_un_indptr"]), shape=(n, n))
    if "feat_indices" in g.files:
        vals = g["feat_vals"] if "feat_vals" in g.files else np.ones(len(g["feat_indices"]), np.float32)
        x = sp.csr_matrix((vals, g["feat_indices"], g["feat_indptr"]), shape=(n, int(g["feat_dim"]))).astype(np.float32)
    else:
        x = None
    return adj, x


def workload(key, dev):
    import acm_gnn_amd
    from acm_gnn_amd import FusedAdam, GCN, data as D, functional as AF, synthetic as S
    from acm_gnn_amd.distributed import make_sharded_operators
    graph, f_in, classes, mt, s, p_drop, hidden = WORKLOADS[key]
    if graph == "study":
        g = S.generate_graph("random", classes, 400, degree_intra=2, edge_homo=0.3, seed=0, device=dev)
        n, ops, y = g.n, g.operators(), g.labels
        rng = np.random.default_rng(1433)
        x = sp.csr_matrix(D.row_normalize_features((rng.random((n, f_in)) < 0.013).astype(np.float32)))
    else:
        adj, x = _graph(graph)
        n = adj.shape[0]
        if x is None:
            x = sp.csr_matrix((np.random.default_rng(f_in).random((n, f_in)) < 0.0086).astype(np.float32))
        assert x.shape == (n, f_in), x.shape
        low, deg = D.build_filters(adj)
        ops = make_sharded_operators(low, deg, dev, with_structure=bool(s))
        y = torch.from_numpy(np.random.default_rng(7).integers(0, classes, n)).to(dev)
    xs = acm_gnn_amd.SparseFeatures.from_scipy(x, dev)

    def make(seed=0):
        torch.manual_seed(seed)
        model = GCN(f_in, hidden, classes, 2, n, p_drop, mt, s).to(dev)
        model.fused_dropout, model.dropout_state = True, AF.DropoutState(dev, seed=7 + seed)
        return model, FusedAdam(model.parameters(), lr=0.01, weight_decay=5e-4)
    shape = dict(workload=key, n=n, nnz_a=int(ops.low.nnz), f_in=f_in, nnz_x=int(x.nnz), classes=classes, hidden=hidden)
    return dict(ops=ops, x=xs, y=y, n=n, make=make, shape=shape)


def splits(n, dev, seed=0):
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).to(dev)
    return idx[: int(0.6 * n)], idx[int(0.6 * n): int(0.8 * n)], idx[int(0.8 * n):]


def stats(v):
    med = statistics.median(v)
    return dict(ms=round(med, 5), min=round(min(v), 5), max=round(max(v), 5), spread=round((max(v) - min(v)) / med, 4),
                samples=[round(s, 5) for s in v])


def bench_step(w, args, dev):
    from acm_gnn_amd import train as T
    model, opt = w["make"]()
    tr, _, _ = splits(w["n"], dev)
    step = T.TrainStep(model, opt, w["x"], w["ops"], w["y"], T.row_weights(tr, w["n"], device=dev), use_graph=True)
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


def timed_fit(w, epochs, dev):
    from acm_gnn_amd import train as T
    model, opt = w["make"](0)
    tr, va, te = splits(w["n"], dev, 0)
    gc.collect()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    T.fit(model, opt, w["x"], w["ops"], w["y"], tr, va, te, epochs, rule="max_val_acc", use_graph=True, sync_every=SYNC)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def summarize(path):
    rows = {}
    for line in open(path):
        r = json.loads(line)
        rows.setdefault((r["workload"], r["arm"], r["label"]), []).append(r)
    print("| workload | arm | label | small path | rounds | ms (median of all samples) | min | max | spread |")
    print("|---|---|---|---|---|---|---|---|---|")
    for (wl, arm, label), rs in sorted(rows.items()):
        v = [s for r in rs for s in r["samples"]]
        med = statistics.median(v)
        small = {r.get("small") for r in rs}
        print(f"| {wl} | {arm} | {label} | {'/'.join(str(s) for s in sorted(small, key=str))} | {len(rs)} | {med:.4f} | {min(v):.4f} | "
              f"{max(v):.4f} | {(max(v) - min(v)) / med:.3f} |")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--label", default="head", help="what the lines are tagged with (head / parent / head_aa)")
    ap.add_argument("--round", type=int, default=1)
    ap.add_argument("--workloads", default=",".join(WORKLOADS))
    ap.add_argument("--warm", type=float, default=1.0, help="seconds of replays before the step windows")
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--epochs", type=int, default=1600)
    ap.add_argument("--base", type=int, default=64)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--arms", default="step,fit")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "small_residual.jsonl"))
    ap.add_argument("--summarize", default=None, help="print the pooled table of a results file and exit")
    args = ap.parse_args()
    if args.summarize:
        return summarize(args.summarize)
    dev = torch.device("cuda:0")
    out = open(args.out, "a")

    def emit(**rec):
        line = json.dumps(dict(label=args.label, round=args.round, device=torch.cuda.get_device_name(0), **rec))
        print(line, flush=True)
        out.write(line + "\n")
        out.flush()

    for key in args.workloads.split(","):
        w = workload(key, dev)
        if "step" in args.arms.split(","):
            emit(arm="step", **w["shape"], **bench_step(w, args, dev))
        if "fit" in args.arms.split(","):
            timed_fit(w, args.base, dev)                  # warm-up: allocator pools, lazy handles
            v = []
            for _ in range(args.repeats):
                short = timed_fit(w, args.base, dev)
                long = timed_fit(w, args.base + args.epochs, dev)
                v.append((long - short) / args.epochs * 1e3)
            from acm_gnn_amd import train as T
            ev_small = None
            try:                                           # whether the evaluation pass took the small path too (public API)
                model, _ = w["make"](0)
                ev_small = T.EvalStep(model, w["x"], w["ops"], w["y"], splits(w["n"], dev)).small is not None
            except Exception:
                pass
            emit(arm="fit", **w["shape"], epochs=args.epochs, base=args.base, sync_every=SYNC, small=ev_small, **stats(v))


if __name__ == "__main__":
    main()
