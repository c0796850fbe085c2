#!/usr/bin/env python3
"""Run ON THE GPU BOX: ms per RUN-EPOCH of ``--runs`` (32) independent training runs on one small graph -- the shape of the
reference's ten-split loop and of its hyper-parameter grid (ACM-Pytorch/train.py:49-139, hyperparameter_searching.py:51-70) --
trained three ways in the same process:

    fit                 ``train.fit(use_graph=True, sync_every=32)`` one run after the other             (plain baseline)
    fit_concurrent2     ``train.fit_concurrent(streams=2, sync_every=32)``                               (THE YARDSTICK)
    fit_batched/B       ``train.fit_batched(batch=B, sync_every=32)``, B = 2, 4, 8, 16, 32               (the batched launches)

    python scripts/bench_batched_fit.py [cora] [chameleon] [squirrel] [--runs 32] [--epochs 400] [--base 20] [--repeats 3] [--out FILE]

Protocol of scripts/bench_resident_fit.py: a host clock around the whole call, ending in a device synchronise; every figure
is the DIFFERENCE of two calls from the same initial state (``--base`` and ``--base + --epochs`` epochs per run), so captures
and plan construction cancel; one warm-up call per arm, then ``--repeats`` (>= 3) rounds that visit the arms in turn.  One JSON
line per (workload, arm): median / min / max ms per run-epoch.  No threshold; nothing here means anything without the GPU."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))
from acm_gnn_amd import train as T  # noqa: E402
from bench_resident_fit import small_workload, splits  # noqa: E402

SYNC = 32


def runs_of(w, n_runs):
    return [w["make"](k) + splits(w["n"], k) for k in range(n_runs)]


def timed(w, n_runs, epochs, arm):
    runs = runs_of(w, n_runs)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if arm == "fit":
        for model, opt, tr, va, te in runs:
            T.fit(model, opt, w["x"], w["ops"], w["y"], tr, va, te, epochs, rule="max_val_acc", use_graph=True, sync_every=SYNC)
    elif arm == "fit_concurrent2":
        T.fit_concurrent(runs, w["x"], w["ops"], w["y"], epochs, rule="max_val_acc", streams=2, sync_every=SYNC)
    else:
        T.fit_batched(runs, w["x"], w["ops"], w["y"], epochs, rule="max_val_acc", batch=int(arm.split("/")[1]), sync_every=SYNC)
        if T.fit_batched.last_refusal is not None:
            raise RuntimeError(f"fit_batched fell back: {T.fit_batched.last_refusal}")
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("names", nargs="*", default=[])
    ap.add_argument("--runs", type=int, default=32)
    ap.add_argument("--epochs", type=int, default=400)
    ap.add_argument("--base", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", default="2,4,8,16,32")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error("--repeats: at least 3 rounds")
    arms = ["fit", "fit_concurrent2"] + [f"fit_batched/{b}" for b in args.batches.split(",") if int(b) <= args.runs]
    out = open(args.out, "a") if args.out else None
    for name in args.names or ["cora", "chameleon", "squirrel"]:
        w = small_workload(name)
        samples = {a: [] for a in arms}
        for a in arms:                                   # warm-up: allocator pools, lazy handles
            timed(w, args.runs, args.base, a)
        for _ in range(args.repeats):
            for a in arms:
                short = timed(w, args.runs, args.base, a)
                long = timed(w, args.runs, args.base + args.epochs, a)
                samples[a].append((long - short) / (args.epochs * args.runs) * 1e3)
        for a, v in samples.items():
            rec = dict(workload=w["name"], n=w["n"], runs=args.runs, arm=a, sync_every=SYNC, epochs=args.epochs, base=args.base,
                       ms_per_run_epoch=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
