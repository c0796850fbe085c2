#!/usr/bin/env python3
"""Time of the homophily measures (acm_gnn_amd.homophily) on the twitch-shaped and the pokec-shaped synthetic graph.

    python scripts/bench_homophily.py [twitch] [pokec]

One JSON line per graph:

  census_us            the three launches of acm_homophily_census into reused buffers, the C entry point called directly with
                       prepared arguments (device events around ``--iters`` calls after a warm-up); ``census_call_us`` is the same
                       through ``homophily.census(..., out=buffers)``, i.e. with the wrapper's operand checks on the host; and ``census_stream_fraction`` = (4 B x nnz of column ids / census time) / 6.29 TB/s, the
                       stream rate measured on this part (EXPERIMENTS.md): the id stream is the one large thing the census must read
                       from HBM (the byte-label table is smaller than one XCD's L2)
  torch_counts_us      the comparison arm on the same GPU: the same counts with torch ops -- ``index_select`` of the int64 labels
                       by column id, then ``bincount`` for M and the two per-row counters (the row index of every entry is made
                       outside the timed window); its M must equal the census's
  agg_onehot_ms / agg_f64_ms   aggregation_homophily end to end (SpMM with the operator's values, class means, score, the host
                       read of the two counts; host clock around calls that end in that read) with F = C (features = one-hot
                       labels) and with F = 64

The reference cannot run at these sizes (its dense n x n matrices: 113 GB at twitch size), so there is no reference time to
compare with and no pass/fail bound: the numbers are recorded in EXPERIMENTS.md."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acm_gnn_amd import _lib, data as D, homophily as H  # noqa: E402
from acm_gnn_amd.graph import _stream  # noqa: E402
from acm_gnn_amd.graph import CsrGraph, FilterOperators, as_implicit  # noqa: E402

DEV = torch.device("cuda:0")
STREAM_TBPS = 6.29
POKEC = (1_632_803, 30_622_564, 14_854)


def pokec_shaped_operator(seed=3):
    """D^-1 (A + I) of a symmetric power-law graph of pokec's shape as pattern + row scale, built on the GPU: ~30.6 M distinct
    undirected pairs with Chung-Lu endpoints (the weights of acm_gnn_amd.data), both directions and the diagonal stored."""
    n, n_edges, max_deg = POKEC
    g = torch.Generator(device=DEV).manual_seed(seed)
    w = torch.from_numpy(D._powerlaw_weights(n, 2.0 * n_edges / n, max_deg)).to(DEV)
    cdf = torch.cumsum(w / w.sum(), 0)
    perm = torch.randperm(n, generator=g, device=DEV)
    u = perm[torch.searchsorted(cdf, torch.rand(n_edges, generator=g, device=DEV, dtype=torch.float64)).clamp_(0, n - 1)]
    v = perm[torch.searchsorted(cdf, torch.rand(n_edges, generator=g, device=DEV, dtype=torch.float64)).clamp_(0, n - 1)]
    keep = u != v
    u, v = u[keep], v[keep]
    diag = torch.arange(n, device=DEV)
    keys = torch.unique(torch.cat([u * n + v, v * n + u, diag * n + diag]))        # sorted: row-major order
    del u, v, keep
    counts = torch.bincount(keys // n, minlength=n)
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=DEV)
    indptr[1:] = torch.cumsum(counts, 0)
    pattern = CsrGraph.from_csr(indptr.to(torch.int32), (keys % n).to(torch.int32), None, n)
    return FilterOperators(pattern, row_scale=(1.0 / counts.to(torch.float32)).contiguous())


def _events(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3                       # us


def _clock(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(iters):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / iters * 1e3               # ms


def run(name, iters):
    c = 2
    if name == "twitch":
        low = D.bench_workload("twitch-gamer", seed=0, node_order="degree")["low"]
        ops = as_implicit(FilterOperators(CsrGraph.from_scipy(low, DEV)))
    else:
        ops = pokec_shaped_operator()
    graph = ops.low
    n = graph.n_rows
    rng = np.random.default_rng(1)
    y = torch.from_numpy(rng.integers(0, c, n).astype(np.int64)).to(DEV)
    out = {"graph": name, "nodes": n, "nnz": int(graph.nnz), "classes": c,
           "operator": "pattern + row scale" if ops.implicit else "valued CSR"}

    buf = H.census_buffers(graph, c)
    out["census_call_us"] = round(_events(lambda: H.census(graph, y, c, out=buf), iters), 1)
    lib, vp = _lib.load(), ctypes.c_void_p
    args = (graph.handle, vp(y.data_ptr()), 0, c, vp(buf._buf.data_ptr()), vp(buf._buf.data_ptr() + 8 * (c * c + 2 * c + 2)),
            vp(buf.row_same.data_ptr()), vp(buf.row_deg.data_ptr()), vp(buf._ws.data_ptr()), buf._ws.numel() * 8)

    def raw():
        _lib.check(lib.acm_homophily_census(*args, _stream()), "acm_homophily_census")

    us = _events(raw, iters)
    out["census_us"] = round(us, 1)
    out["census_id_stream_GBps"] = round(4.0 * graph.nnz / us * 1e-3, 1)
    out["census_stream_fraction"] = round(4.0 * graph.nnz / (us * 1e-6) / (STREAM_TBPS * 1e12), 3)
    res = H.census(graph, y, c, out=buf)
    out.update(edge=res.edge, node=res.node, klass=res.klass)

    ip, ix, _ = graph.arrays()
    cols = ix.to(torch.int64)
    rows = torch.repeat_interleave(torch.arange(n, device=DEV), (ip[1:] - ip[:-1]).to(torch.int64))

    def torch_counts():
        yc, yr = y.index_select(0, cols), y.index_select(0, rows)
        keep = rows != cols
        m = torch.bincount((yr * c + yc)[keep], minlength=c * c)
        deg = torch.bincount(rows[keep], minlength=n)
        same = torch.bincount(rows[keep & (yr == yc)], minlength=n)
        return m, deg, same

    out["torch_counts_us"] = round(_events(torch_counts, max(iters // 4, 5)), 1)
    m, deg, same = torch_counts()
    assert torch.equal(m, res.counts[:c * c]) and torch.equal(deg.to(torch.int32), res.row_deg) \
        and torch.equal(same.to(torch.int32), res.row_same)
    out["census_speedup_over_torch"] = round(out["torch_counts_us"] / out["census_us"], 1)
    del cols, rows, m, deg, same

    out["agg_onehot_ms"] = round(_clock(lambda: H.aggregation_homophily(None, ops, y), max(iters // 4, 5)), 3)
    x = torch.from_numpy(rng.standard_normal((n, 64)).astype(np.float32)).to(DEV)
    out["agg_f64_ms"] = round(_clock(lambda: H.aggregation_homophily(x, ops, y), max(iters // 4, 5)), 3)
    out["agg_onehot"], out["agg_f64"] = H.aggregation_homophily(None, ops, y), H.aggregation_homophily(x, ops, y)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("graphs", nargs="*", default=["twitch", "pokec"])
    ap.add_argument("--iters", type=int, default=40)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_homophily.py needs the GPU"
    for nm in args.graphs:
        print(json.dumps(run(nm, args.iters)), flush=True)
