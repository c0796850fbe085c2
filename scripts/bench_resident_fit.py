#!/usr/bin/env python3
"""Run ON THE GPU BOX: ms per epoch of ``train.fit(use_graph=True, rule="max_val_acc")`` with the selection on the host
(``sync_every=1``: one synchronising read per epoch, the yardstick) and on the device (``sync_every`` = 8 / 32 / 128, with and
without ``keep_best``), and of ``train.fit_concurrent(streams=2)`` at ``sync_every`` = 1 / 32.

    python scripts/bench_resident_fit.py [cora] [chameleon] [squirrel] [study] [--epochs 2000] [--repeats 3] [--out FILE]

Workloads: the Cora-, Chameleon- and Squirrel-shaped configurations of scripts/bench_configs.py with CSR features (the fused
small-graph step) and the synthetic study's ``gcn`` baseline at study size (2 000 nodes, 1 433 dense features, hidden 32).

Timing: a host clock around the whole ``fit`` call, ending in a device synchronise.  A call pays its captures once, so every
measurement is the DIFFERENCE of two calls from the same initial state -- ``--base`` epochs and ``--base + --epochs`` epochs --
divided by ``--epochs``: what an epoch costs once the graphs exist.  One warm-up call per arm, then ``--repeats`` rounds that
visit the arms one after the other (drift hits all arms alike).  One JSON line per (workload, arm): median / min / max ms per
epoch.  No threshold; nothing here is meaningful without the GPU."""
import argparse
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
sys.path.insert(0, os.path.join(ROOT, "scripts"))
import acm_gnn_amd  # noqa: E402
from acm_gnn_amd import FusedAdam, baselines, data as D, distributed as DD, functional as AF, synthetic as S, train as T  # noqa: E402
from bench_configs import CONFIGS, real_graph  # noqa: E402

DEV = torch.device("cuda:0")
SHAPES = {"cora": "cora/acmgcn", "chameleon": "chameleon/acmgcnp+A", "squirrel": "squirrel/acmgcnp+A"}


def small_workload(name):
    cfg = CONFIGS[SHAPES[name]]
    adj, _ = real_graph(cfg["graph"])
    n, f_in, classes = adj.shape[0], cfg["f_in"], cfg["classes"]
    rng = np.random.default_rng(0)
    x_np = (rng.random((n, f_in)) < 0.01).astype(np.float32)
    y = torch.from_numpy(rng.integers(0, classes, n)).to(DEV)
    if not cfg["s"]:
        x_np = D.row_normalize_features(x_np)
    low, deg = D.build_filters(adj)
    ops = DD.make_sharded_operators(low, deg, DEV, with_structure=bool(cfg["s"]))
    x = acm_gnn_amd.SparseFeatures.from_scipy(sp.csr_matrix(x_np), DEV)

    def make(seed=0):
        torch.manual_seed(seed)
        model = acm_gnn_amd.GCN(f_in, 64, classes, 2, n, cfg["dropout"], cfg["method"], cfg["s"], variant=bool(cfg["variant"]),
                                attn_layernorm=True).to(DEV)
        model.fused_dropout, model.dropout_state = True, AF.DropoutState(DEV, seed=7 + seed)
        return model, FusedAdam(model.parameters(), lr=0.01, weight_decay=1e-4)
    return dict(name=name, ops=ops, x=x, y=y, n=n, make=make, small=True)


def study_workload():
    g = S.generate_graph("regular", 5, 400, degree_intra=2, edge_homo=0.3, seed=0, device=DEV)
    x = S.random_features(g.n, 1433, seed=0, device=DEV)

    def make(seed=0):
        torch.manual_seed(seed)
        model = baselines.GCN(1433, 32, 5, 0.5, "gcn").to(DEV)
        model.fused_dropout, model.dropout_state = True, AF.DropoutState(DEV, seed=7 + seed)
        return model, FusedAdam(model.parameters(), lr=0.05, weight_decay=5e-4)
    return dict(name="study/gcn", ops=g.operators(), x=x, y=g.labels, n=g.n, make=make, small=False)


def splits(n, seed=0):
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(seed)).to(DEV)
    return idx[: n // 2], idx[n // 2: 3 * n // 4], idx[3 * n // 4:]


def timed_fit(w, epochs, sync_every, keep_best):
    model, opt = w["make"]()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    T.fit(model, opt, w["x"], w["ops"], w["y"], *splits(w["n"]), epochs, rule="max_val_acc", use_graph=True, sync_every=sync_every,
          keep_best=keep_best)
    torch.cuda.synchronize()
    return time.perf_counter() - t0


def timed_concurrent(w, epochs, sync_every, keep_best):
    runs = [w["make"](k) + splits(w["n"], k) for k in range(2)]
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    T.fit_concurrent(runs, w["x"], w["ops"], w["y"], epochs, rule="max_val_acc", streams=2, sync_every=sync_every, keep_best=keep_best)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / 2            # per run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("names", nargs="*", default=[])
    ap.add_argument("--epochs", type=int, default=2000)
    ap.add_argument("--base", type=int, default=100)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    names = args.names or ["cora", "chameleon", "squirrel", "study"]
    arms = [("fit", timed_fit, s, k) for k in (False, True) for s in (1, 8, 32, 128)]
    arms += [("fit_concurrent2", timed_concurrent, s, False) for s in (1, 32)]
    out = open(args.out, "a") if args.out else None
    for name in names:
        w = study_workload() if name == "study" else small_workload(name)
        step = T.TrainStep(*w["make"](), w["x"], w["ops"], w["y"], T.row_weights(splits(w["n"])[0], w["n"], device=DEV))
        samples = {a[0:1] + a[2:]: [] for a in arms}
        for kind, fn, s, k in arms:                          # warm-up: allocator pools, lazy handles, both epoch counts
            fn(w, args.base, s, k)
        for _ in range(args.repeats):
            for kind, fn, s, k in arms:
                short = fn(w, args.base, s, k)
                long = fn(w, args.base + args.epochs, s, k)
                samples[(kind, s, k)].append((long - short) / args.epochs * 1e3)
        for (kind, s, k), v in samples.items():
            rec = dict(workload=w["name"], n=w["n"], small_plan=step.small is not None, loop=kind, sync_every=s, keep_best=k,
                       epochs=args.epochs, ms_per_epoch=round(statistics.median(v), 4), min=round(min(v), 4), max=round(max(v), 4))
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()


if __name__ == "__main__":
    main()
