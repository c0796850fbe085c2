"""ACM-GCN++ with a deep residual stack (init_layers_X = 2: Linear-ReLU-BatchNorm-Linear): a captured TrainStep on the
acm_bnorm_* route against the same step with ``tuning mlp_stack=0``, i.e. the torch modules in the middle of the step.

    python scripts/bench_mlp_stack.py [--steps 100] [--rounds 3] [--out profiles/mlp_stack.jsonl] [--shapes twitch-gamer,penn94]

Shapes (data.synthetic_dataset): twitch-gamer (168 114 x 7, hidden 64) and penn94 (41 554 x 4 814 one-hot style features,
hidden 64); the kernel arm takes the penn94 input through GCN.auto_csr (CSR features), the torch arm gets it dense -- without
the kernels a deep stack refuses CSR features.  Per shape the two arms are built once (same seed) and timed alternately,
``--rounds`` windows of ``--steps`` graph replays each between device synchronisations, after three warm-up replays; one JSON
line per shape with every window and the medians, appended to ``--out``."""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import acm_gnn_amd  # noqa: E402
from acm_gnn_amd import data as D, distributed as DD, functional as AF, train as T, tuning  # noqa: E402

DEV = torch.device("cuda:0")


def build(shape, kernels):
    adj, x_np, y_np, splits, n = D.synthetic_dataset(shape)
    perm = D.degree_order(adj)
    adj, x_np, y_np, splits = D.permute_dataset(adj, x_np, y_np, splits, perm)
    x_np = D.row_normalize_features(x_np)
    low, deg = D.build_filters(adj)
    ops = DD.make_sharded_operators(low, deg, DEV)
    x, y = torch.from_numpy(x_np).to(DEV), torch.from_numpy(y_np.astype("int64")).to(DEV)
    torch.manual_seed(0)
    model = acm_gnn_amd.GCN(x.shape[1], 64, int(y_np.max()) + 1, 2, n, 0.1, "acmgcnpp", 0, attn_layernorm=True, init_layers_X=2).to(DEV)
    model.fused_dropout, model.dropout_state = True, AF.DropoutState(DEV, seed=1)
    opt = acm_gnn_amd.FusedAdam(model.parameters(), lr=0.01, weight_decay=1e-4)
    w = T.row_weights(torch.from_numpy(splits[0]).to(DEV), n)
    with tuning.override(mlp_stack=1 if kernels else 0):
        step = T.TrainStep(model, opt, x, ops, y, w, use_graph=True)          # (the route is fixed at capture)
        csr = isinstance(step.x, acm_gnn_amd.SparseFeatures)
        for _ in range(3):
            step()
    torch.cuda.synchronize()
    return step, dict(n=n, f_in=int(x.shape[1]), nnz_low=int(low.nnz), csr_features=csr)


def window(step, steps):
    torch.cuda.synchronize()
    t = time.perf_counter()
    for _ in range(steps):
        step()
    torch.cuda.synchronize()
    return (time.perf_counter() - t) / steps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--shapes", default="twitch-gamer,penn94")
    ap.add_argument("--out", default=os.path.join("profiles", "mlp_stack.jsonl"))
    args = ap.parse_args()
    for shape in args.shapes.split(","):
        (new, info), (old, info_old) = build(shape, True), build(shape, False)
        assert not info_old["csr_features"]
        ms = {"kernels": [], "torch": []}
        for _ in range(args.rounds):                                          # alternating: both arms see the same neighbours
            ms["kernels"].append(round(window(new, args.steps), 4))
            ms["torch"].append(round(window(old, args.steps), 4))
        k, t = statistics.median(ms["kernels"]), statistics.median(ms["torch"])
        line = dict(bench="mlp_stack", shape=shape, hidden=64, init_layers_X=2, steps=args.steps, **info, kernels_ms=ms["kernels"],
                    torch_ms=ms["torch"], kernels_ms_median=k, torch_ms_median=t, torch_over_kernels=round(t / k, 3),
                    device=torch.cuda.get_device_name(0))
        print(json.dumps(line), flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as fh:
            fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
