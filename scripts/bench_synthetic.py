#!/usr/bin/env python3
"""Time of the synthetic graph generator (acm_gnn_amd.synthetic) against the same generation built from torch ops on the same
GPU, at the reference's 5 x 400 and at a twitch-sized and a pokec-sized shape.

    python scripts/bench_synthetic.py [small] [twitch] [pokec] [--reps 7]

One JSON line per (shape, graph type):

  generate_ms          median host-clock time of ``generate_graph`` ending in a device synchronise (the random type ends in its
                       one host read anyway), after two warm-up calls
  torch_ms             the comparison arm, written here: ``regular`` = ``randint`` of k ids per row, rows holding a duplicate
                       drawn again until none is left (a rejection sampler: uniform over k-subsets), shifted, concatenated and
                       sorted per row; ``random`` = ``randint`` keys + ``unique`` + a ``randperm`` subset per class, the class
                       chain with its count read on the host, both directions, one sort of the keys
  kernel_us            (regular) device events around the C entry point ``acm_synth_regular`` alone, and
  written_GBps / stream_fraction   = 4 B x n x d / kernel time, and that over 6.29 TB/s, the stream rate measured on this part
                       (EXPERIMENTS.md).  The kernel writes 4 d bytes per row and reads nothing; per row one wave runs d
                       dependent Floyd steps (multiply-high, compare with the chosen set, ballot), so it is EXPECTED to be
                       bound by the latency of that chain, not by the stores; the measured fraction says which
  reference_host_s     (small) the seconds ``graph_generation.py`` took per graph on the host where the golden file was
                       recorded (tests/golden/synthetic_cases.npz)

No threshold: the numbers are recorded in EXPERIMENTS.md."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acm_gnn_amd import _lib, synthetic as S  # noqa: E402
from acm_gnn_amd.graph import _stream  # noqa: E402

DEV = torch.device("cuda:0")
STREAM_TBPS = 6.29
# name: (C, npc, degree_intra for regular, h for regular, degree_intra for random, h for random)
SHAPES = {"small": (5, 400, 2, 0.3, 2, 0.3),
          "twitch": (2, 84_057, 41, 0.5, 40, 0.5),            # 168 114 nodes; 13.8 M / 13.4 M entries
          "pokec": (2, 816_401, 19, 0.5, 18, 0.47)}           # 1 632 802 nodes; 62.0 M / 62.5 M entries


def _median_ms(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t) * 1e3)
    return statistics.median(times), min(times), max(times)


def _distinct_rows(rows, k, m, gen):
    """int64 [rows, k]: k distinct of [0, m) per row -- randint, rows with a duplicate drawn again."""
    ids = torch.randint(m, (rows, k), device=DEV, generator=gen)
    if k < 2:
        return ids
    while True:
        srt = torch.sort(ids, 1).values
        bad = torch.nonzero((srt[:, 1:] == srt[:, :-1]).any(1))[:, 0]
        if bad.numel() == 0:
            return ids
        ids[bad] = torch.randint(m, (bad.numel(), k), device=DEV, generator=gen)


def torch_regular(c, npc, k, d_inter, gen):
    n = c * npc
    j = torch.arange(n, device=DEV)
    base = j // npc * npc
    a = _distinct_rows(n, k, npc - 1, gen)
    a = base[:, None] + a + (a >= (j - base)[:, None])
    o = _distinct_rows(n, d_inter, n - npc, gen)
    o = o + torch.where(o >= base[:, None], npc, 0)
    return torch.sort(torch.cat([a, o], 1), 1).values.to(torch.int32)


def _subset(keys, m, gen):
    u = torch.unique(keys)
    assert u.numel() >= m, "torch arm: too few distinct keys drawn"
    return u[torch.randperm(u.numel(), device=DEV, generator=gen)[:m]]


def torch_random(c, npc, k, h, gen):
    n, s_edges = c * npc, k * npc
    rows, cols = [], []
    for i in range(c):
        want = s_edges // 2
        x = torch.randint(npc, (int(1.3 * want) + 64,), device=DEV, generator=gen)
        y = torch.randint(npc, (int(1.3 * want) + 64,), device=DEV, generator=gen)
        keep = x != y
        key = _subset(torch.minimum(x, y)[keep] * npc + torch.maximum(x, y)[keep], want, gen)
        rows += [key // npc + i * npc, key % npc + i * npc]
        cols += [key % npc + i * npc, key // npc + i * npc]
    t = s_edges * (1 - h) / h
    placed = torch.zeros(c, dtype=torch.int64, device=DEV)
    for i in range(c - 1):
        m = max(0, round(t - float(placed[i])) + 1)                      # a host read per class
        width = (c - 1 - i) * npc
        key = _subset(torch.randint(npc * width, (int(1.2 * m) + 64,), device=DEV, generator=gen), m, gen)
        x, y = key // width + i * npc, key % width + (i + 1) * npc
        rows += [x, y]
        cols += [y, x]
        placed += torch.bincount(y // npc, minlength=c)
    keys = torch.sort(torch.cat(rows) * n + torch.cat(cols)).values
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    indptr[1:] = torch.cumsum(torch.bincount(keys // n, minlength=n), 0)
    return indptr.to(torch.int32), (keys % n).to(torch.int32)


def run(name, reps):
    c, npc, k_reg, h_reg, k_rnd, h_rnd = SHAPES[name]
    n = c * npc
    gen = torch.Generator(device=DEV).manual_seed(0)
    recorded = {}
    if name == "small":
        with np.load(os.path.join(ROOT, "tests", "golden", "synthetic_cases.npz")) as f:
            recorded = {kind: float(f[f"{kind}:{h_reg}:seconds"]) for kind in ("regular", "random")}
    # ---- regular
    d_inter = int(k_reg / h_reg - k_reg)
    d = k_reg + d_inter
    out = {"shape": name, "type": "regular", "nodes": n, "classes": c, "degree": d, "entries": n * d}
    counter = [0]

    def ours():
        counter[0] += 1
        return S.generate_graph("regular", c, npc, k_reg, h_reg, seed=0, graph_index=counter[0], device=DEV)

    med, lo, hi = _median_ms(ours, reps)
    out.update(generate_ms=round(med, 3), generate_ms_range=[round(lo, 3), round(hi, 3)])
    med, lo, hi = _median_ms(lambda: torch_regular(c, npc, k_reg, d_inter, gen), reps)
    out.update(torch_ms=round(med, 3), torch_ms_range=[round(lo, 3), round(hi, 3)], speedup_over_torch=round(med / out["generate_ms"], 1))
    indices = torch.empty(n * d, dtype=torch.int32, device=DEV)
    lib = _lib.load()

    def raw():
        _lib.check(lib.acm_synth_regular(c, npc, k_reg, d_inter, 0, 1, 0, n, ctypes.c_void_p(indices.data_ptr()), _stream()), "acm_synth_regular")

    iters = 200 if name == "small" else 20
    for _ in range(3):
        raw()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        raw()
    b.record()
    torch.cuda.synchronize()
    us = a.elapsed_time(b) / iters * 1e3
    out.update(kernel_us=round(us, 1), written_GBps=round(4.0 * n * d / us * 1e-3, 1),
               stream_fraction=round(4.0 * n * d / (us * 1e-6) / (STREAM_TBPS * 1e12), 4))
    if recorded:
        out["reference_host_s"] = round(recorded["regular"], 3)
    print(json.dumps(out), flush=True)
    del indices
    # ---- random
    out = {"shape": name, "type": "random", "nodes": n, "classes": c}

    def ours_random():
        counter[0] += 1
        return S.generate_graph("random", c, npc, k_rnd, h_rnd, seed=0, graph_index=counter[0], device=DEV)

    g = ours_random()
    out.update(entries=int(g.indices.numel()), attempts=g.info["attempts"])
    del g
    med, lo, hi = _median_ms(ours_random, reps)
    out.update(generate_ms=round(med, 3), generate_ms_range=[round(lo, 3), round(hi, 3)])
    med, lo, hi = _median_ms(lambda: torch_random(c, npc, k_rnd, h_rnd, gen), reps)
    out.update(torch_ms=round(med, 3), torch_ms_range=[round(lo, 3), round(hi, 3)], speedup_over_torch=round(med / out["generate_ms"], 2))
    if recorded:
        out["reference_host_s"] = round(recorded["random"], 3)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["small", "twitch", "pokec"])
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_synthetic.py needs the GPU"
    for nm in args.shapes:
        run(nm, args.reps)
