#!/usr/bin/env python3
"""Run ON THE GPU BOX: ms per RUN-EPOCH of the synthetic study's inner loop (synthetic-experiments/train.py:64-164) -- ten
generated graphs at one edge homophily, each with its own adjacency, its own features and its own split, one run per graph --
trained two ways in the same process:

    fit                     ``train.fit(use_graph=True, sync_every=32)`` one run after the other     (the only route before)
    fit_batched_graphs/B    ``train.fit_batched_graphs(batch=B, sync_every=32)``, B = 8, 10          (the shared launches)

    python scripts/bench_batched_graphs.py [--graphs 10] [--epochs 400] [--base 20] [--repeats 3] [--density 1.0] [--out FILE]

The graphs are ``synthetic.generate_graph("random", 5, 400, edge_homo=0.3, graph_index=g)`` (2 000 nodes), the features
``synthetic.random_features(2000, 1433, graph_index=g)`` as CSR (``--density`` < 1 keeps the entries below it and zeroes the
rest: a bag-of-words-like matrix of that density, still one per graph), the model ``baselines.GCN(1433, 32, 5, 0.5, "acmgcn",
nnodes=2000)`` with counter-based dropout, FusedAdam.

Protocol of scripts/bench_batched_fit.py: a host clock around the whole call, ending in a device synchronise; every figure is
the DIFFERENCE of two calls from the same initial state (``--base`` and ``--base + --epochs`` epochs per run), so captures and
plan construction cancel; one warm-up call per arm, then ``--repeats`` (>= 3) rounds that visit the arms in turn.  The rule
is "max_val_acc", under which a run uses its whole budget.  One JSON line per arm: median / min / max ms per run-epoch.  No
threshold; nothing here means anything without the GPU."""
import argparse
import gc
import json
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import acm_gnn_amd  # noqa: E402
from acm_gnn_amd import FusedAdam, baselines, functional as AF, synthetic as S, train as T  # noqa: E402

DEV = torch.device("cuda:0")
SYNC = 32
F_IN, CLASSES, PER_CLASS, HIDDEN = 1433, 5, 400, 32


def workload(n_graphs, density):
    graphs = []
    for g in range(n_graphs):
        sg = S.generate_graph("random", CLASSES, PER_CLASS, degree_intra=2, edge_homo=0.3, seed=0, graph_index=g, device=DEV)
        x = S.random_features(sg.n, F_IN, seed=0, graph_index=g, device=DEV)
        if density < 1.0:
            x = torch.where(x < density, x / density, torch.zeros_like(x))
        xs = acm_gnn_amd.SparseFeatures.from_torch(x)
        graphs.append(dict(ops=sg.operators(), x=xs, y=sg.labels, n=sg.n, nnz_x=int(xs.csr.nnz), nnz_a=int(sg.adj.nnz),
                           splits=S.disassortative_splits(sg.labels, CLASSES, seed=0, split_index=g)))
    return graphs


def runs_of(graphs):
    runs = []
    for k, g in enumerate(graphs):
        torch.manual_seed(k)
        model = baselines.GCN(F_IN, HIDDEN, CLASSES, 0.5, "acmgcn", nnodes=g["n"]).to(DEV)
        model.fused_dropout, model.dropout_state = True, AF.DropoutState(DEV, seed=7 + k)
        runs.append((model, FusedAdam(model.parameters(), lr=0.05, weight_decay=5e-4), g["x"], g["ops"], g["y"]) + tuple(g["splits"]))
    return runs


def timed(graphs, epochs, arm):
    runs = runs_of(graphs)
    gc.collect()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    if arm == "fit":
        for model, opt, x, ops, y, tr, va, te in runs:
            T.fit(model, opt, x, ops, y, tr, va, te, epochs, rule="max_val_acc", use_graph=True, sync_every=SYNC)
    else:
        T.fit_batched_graphs(runs, epochs, rule="max_val_acc", batch=int(arm.split("/")[1]), sync_every=SYNC)
        if T.fit_batched_graphs.last_refusal is not None:
            raise RuntimeError(f"fit_batched_graphs fell back: {T.fit_batched_graphs.last_refusal}")
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--graphs", type=int, default=10)
    ap.add_argument("--epochs", type=int, default=400)
    ap.add_argument("--base", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--batches", default="8,10")
    ap.add_argument("--density", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.repeats < 3:
        ap.error("--repeats: at least 3 rounds")
    arms = ["fit"] + [f"fit_batched_graphs/{b}" for b in args.batches.split(",") if int(b) <= args.graphs]
    graphs = workload(args.graphs, args.density)
    samples = {a: [] for a in arms}
    for a in arms:                                       # warm-up: allocator pools, lazy handles
        timed(graphs, args.base, a)
    for _ in range(args.repeats):
        for a in arms:
            short = timed(graphs, args.base, a)
            long = timed(graphs, args.base + args.epochs, a)
            samples[a].append((long - short) / (args.epochs * len(graphs)) * 1e3)
    out = open(args.out, "a") if args.out else None
    for a, v in samples.items():
        rec = dict(workload="synthetic_random_h0.3", graphs=len(graphs), n=graphs[0]["n"], f_in=F_IN, hidden=HIDDEN, density=args.density,
                   nnz_x=[g["nnz_x"] for g in graphs][:3], nnz_a=[g["nnz_a"] for g in graphs][:3], arm=a, sync_every=SYNC,
                   epochs=args.epochs, base=args.base, ms_per_run_epoch=round(statistics.median(v), 4), min=round(min(v), 4),
                   max=round(max(v), 4))
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()


if __name__ == "__main__":
    main()
