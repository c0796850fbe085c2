"""ACM-Snowball (nlayers = 2, nhid = 64) with the features handed over dense -- the concatenating stack -- against the same
model handed SparseFeatures -- column blocks, functional.project_blocks: a captured TrainStep per arm, in the same process.

    python scripts/bench_snowball.py [--shapes cora,penn94] [--warm 2.0] [--window 1.0] [--rounds 5] [--out profiles/snowball_blocks.jsonl]

Shapes: Cora (2 708 nodes, 5 278 edges, 1 433 bag-of-words columns, 7 classes; about 18 stored words per row) and Penn94 (data.SHAPES:
41 554 nodes, 4 814 one-hot style columns, 5 stored per row); Chung-Lu graphs (data.chung_lu_graph), features generated sparse.
Per shape both arms are built from the same seed, warmed up for ``--warm`` seconds each, then timed alternately: ``--rounds``
windows of at least ``--window`` seconds of graph replays between device synchronisations; the median window is reported, every
window is kept.  Peak memory: torch.cuda.max_memory_allocated over one arm's build and warm-up, above what was
allocated before the arm was built (the dense arm's includes its [n, F_in] input).  One eager step per arm under a KernelTimer
lists the launches.  One JSON line per shape; a run rewrites ``--out``."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import acm_gnn_amd  # noqa: E402
from acm_gnn_amd import data as D, distributed as DD, functional as AF, train as T  # noqa: E402

DEV = torch.device("cuda:0")
# (nodes, undirected edges, input features, classes), largest degree, stored features per row
CORA = ((2_708, 5_278, 1_433, 7), 168, 18)
PENN94 = (D.SHAPES["penn94"], 4_400, 5)


def dataset(name, seed=0):
    (n, e, f_in, c), max_deg, per_row = {"cora": CORA, "penn94": PENN94}[name]
    adj = D.chung_lu_graph(n, e, max_deg, seed=seed)
    rng = np.random.default_rng(seed + 1)
    cols = rng.integers(0, f_in, size=(n, per_row))
    x = sp.csr_matrix((np.ones(n * per_row, np.float32), (np.repeat(np.arange(n), per_row), cols.reshape(-1))), shape=(n, f_in))
    x.sum_duplicates()
    x.data[:] = 1.0
    x = sp.diags(1.0 / np.maximum(np.asarray(x.sum(1)).reshape(-1), 1.0)).dot(x).astype(np.float32).tocsr()     # rows sum to one
    y = rng.integers(0, c, n).astype(np.int64)
    train = np.sort(rng.permutation(n)[: n // 2])
    return adj, x, y, train, (n, e, f_in, c)


class Arm:
    def __init__(self, name, sparse, data):
        adj, x, y, train, (n, _, f_in, c) = data
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        self.base = torch.cuda.memory_allocated()
        low, deg = D.build_filters(adj)
        ops = DD.make_sharded_operators(low, deg, DEV)
        feats = acm_gnn_amd.SparseFeatures.from_scipy(x, DEV) if sparse else torch.from_numpy(x.toarray()).to(DEV)
        torch.manual_seed(0)
        model = acm_gnn_amd.GCN(f_in, 64, c, 2, n, 0.5, "acmsnowball", 0).to(DEV)
        opt = acm_gnn_amd.FusedAdam(model.parameters(), lr=0.01, weight_decay=5e-4)
        args = (model, opt, feats, ops, torch.from_numpy(y).to(DEV), T.row_weights(torch.from_numpy(train).to(DEV), n))
        timer = AF.KernelTimer()                          # one eager step: which launches, how long each
        AF.set_kernel_timer(timer)
        try:
            T.TrainStep(*args)()
            self.kernels = {k: [v[0], round(v[1], 4)] for k, v in sorted(timer.summary().items())}
        finally:
            AF.set_kernel_timer(None)
        self.step = T.TrainStep(*args, use_graph=True)
        assert isinstance(self.step.x, acm_gnn_amd.SparseFeatures) == sparse
        self.name, self.windows = name, []

    def run_for(self, seconds):
        """Replays until ``seconds`` have passed (checked at synchronisations, 20 replays apart); ms per step."""
        torch.cuda.synchronize()
        t0, steps = time.perf_counter(), 0
        while True:
            for _ in range(20):
                self.step()
            steps += 20
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            if dt >= seconds:
                return dt / steps * 1e3

    def peak(self):
        return int(torch.cuda.max_memory_allocated() - self.base)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="cora,penn94")
    ap.add_argument("--warm", type=float, default=2.0)
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join("profiles", "snowball_blocks.jsonl"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_snowball.py measures on the GPU: no device found")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    open(args.out, "w").close()                                       # a run replaces the file: one line per shape
    for shape in args.shapes.split(","):
        data = dataset(shape)
        peaks, arms = {}, {}
        for name, sparse in (("dense", False), ("csr", True)):        # one after the other: each arm's own peak
            arm = arms[name] = Arm(name, sparse, data)
            arm.run_for(args.warm)
            peaks[name] = arm.peak()
        for _ in range(args.rounds):                                  # alternating: both arms see the same neighbours
            for arm in arms.values():
                arm.windows.append(round(arm.run_for(args.window), 4))
        med = {k: statistics.median(a.windows) for k, a in arms.items()}
        n, e, f_in, c = data[4]
        line = dict(bench="snowball_blocks", shape=shape, n=n, edges=e, f_in=f_in, classes=c, nnz_x=int(data[1].nnz), nhid=64, nlayers=2,
                    dropout=0.5, dense_ms=arms["dense"].windows, csr_ms=arms["csr"].windows, dense_ms_median=med["dense"],
                    csr_ms_median=med["csr"], dense_over_csr=round(med["dense"] / med["csr"], 3), dense_peak_bytes=peaks["dense"],
                    csr_peak_bytes=peaks["csr"], dense_eager_kernels=arms["dense"].kernels, csr_eager_kernels=arms["csr"].kernels,
                    warm_s=args.warm, window_s=args.window, device=torch.cuda.get_device_name(0))
        print(json.dumps(line), flush=True)
        with open(args.out, "a") as fh:
            fh.write(json.dumps(line) + "\n")
        del arms
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
