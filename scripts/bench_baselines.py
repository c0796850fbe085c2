#!/usr/bin/env python3
"""One captured training step of the synthetic study's ``gcn`` and ``sgc`` baselines (acm_gnn_amd.baselines), three arms in the
same process, alternated:

  fused      this package's path (acm_gcn_fwd / acm_gcn_bwd / acm_gemm_act, the cached P = A_low^k X), FORCED at any size
             (``model.fused = "always"``)
  default    ``model.fused = True`` where that is not the fused arm: above functional.gcn.FUSE_MAX_ITEMS work items the model
             takes the composed arm for the whole step (the row is there to show that it is the composed arm's time)
  composed   the same model with ``fused=False``: every graph product composed from the entry points that predate acm_gcn_*
  torch      the same model in plain torch on the same GPU: ``torch.sparse.mm`` on a CSR tensor, autograd, ``torch.optim.Adam``
             -- an EAGER step (``captured: false``): capturing it raised an AcceleratorError in the sparse product
  fused_eager   this package's step un-captured (train.TrainStep on its tape), the like-for-like row for the torch arm

    python scripts/bench_baselines.py [study] [twitch] [--seconds 0.4] [--repeats 5]

Shapes: ``study`` = 2 000 nodes (5 x 400, the generators' regular graph at h = 0.3), 1 433 dense uniform features, 5 classes,
hidden 32; ``twitch`` = the twitch-gamer-shaped workload of ``data.bench_workload`` (168 114 nodes, 7 features, 2 classes),
hidden 64.  ``gcn_project_first`` is the gcn model with the P cache switched off (x projected first, then gathered: the form
CSR features take), so that acm_gcn_fwd's hidden-layer form is timed as well.

Timing (device events): every arm is warmed up for ``--seconds``, then each of ``--repeats`` rounds times a window of at least
``--seconds`` per arm, arm after arm, so that drift hits all arms alike.  One JSON line per (shape, model, arm): median ms per
step with the min / max over the rounds, kernels per step (counted by the profiler in one eager step; ``library_launches`` =
this library's own launches in that step).  No threshold; nothing here is meaningful without the GPU."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from acm_gnn_amd import FusedAdam, baselines, data, synthetic as S, train as T  # noqa: E402
from acm_gnn_amd import functional as AF  # noqa: E402
from acm_gnn_amd.graph import CsrGraph, FilterOperators, as_implicit, explicit_arrays  # noqa: E402

DEV = torch.device("cuda:0")
LR, WD, P_DROP = 0.05, 5e-4, 0.5


def study_shape():
    g = S.generate_graph("regular", 5, 400, degree_intra=2, edge_homo=0.3, seed=0, device=DEV)
    x = S.random_features(g.n, 1433, seed=0, device=DEV)
    tr = S.disassortative_splits(g.labels, 5, seed=0)[0]
    return dict(name="study", ops=g.operators(), x=x, y=g.labels, train=tr, hidden=32, classes=5)


def twitch_shape():
    w = data.bench_workload("twitch-gamer")
    low = w["low"]
    ops = as_implicit(FilterOperators(CsrGraph.from_scipy(low, DEV)))
    return dict(name="twitch", ops=ops, x=torch.from_numpy(np.ascontiguousarray(w["x"], np.float32)).to(DEV),
                y=torch.from_numpy(w["y"]).to(DEV), train=torch.from_numpy(w["splits"][0]).to(DEV), hidden=64,
                classes=int(w["y"].max()) + 1)


# ---- the torch arm ---------------------------------------------------------------------------------------------------------
class TorchModel(torch.nn.Module):
    def __init__(self, kind, f_in, hidden, classes, adj):
        super().__init__()
        self.kind, self.adj = kind, adj
        dims = [(f_in, classes)] if kind == "sgc" else [(f_in, hidden), (hidden, classes)]
        self.w = torch.nn.ParameterList([torch.nn.Parameter(torch.empty(a, b, device=DEV).uniform_(-1 / b ** 0.5, 1 / b ** 0.5)) for a, b in dims])

    def forward(self, x):
        h = torch.sparse.mm(self.adj, x @ self.w[0])
        if self.kind == "sgc":
            return h
        h = F.dropout(F.relu(h), P_DROP, training=self.training)
        return torch.sparse.mm(self.adj, h @ self.w[1])


def torch_arm(kind, shape):
    ip, ix, v = explicit_arrays(shape["ops"])
    n = shape["x"].shape[0]
    adj = torch.sparse_csr_tensor(ip.to(torch.int64), ix.to(torch.int64), v, (n, n))
    model = TorchModel(kind, shape["x"].shape[1], shape["hidden"], shape["classes"], adj)
    opt = torch.optim.Adam(model.parameters(), lr=LR, weight_decay=WD)
    x, y, tr = shape["x"], shape["y"], shape["train"]

    def step():
        model.train()
        opt.zero_grad(set_to_none=True)
        loss = F.nll_loss(F.log_softmax(model(x), 1)[tr], y[tr])
        loss.backward()
        opt.step()
        return loss

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    # eager: capturing this step with torch.cuda.graph raised an AcceleratorError on the MI355X (the sparse CSR product), so this
    # arm pays its launches on the host; ``fused_eager`` is this package's un-captured step, the like-for-like row
    return step, step, False


# ---- this package's arms ---------------------------------------------------------------------------------------------------
def package_arm(kind, shape, fused):
    mt = "sgc" if kind == "sgc" else "gcn"
    torch.manual_seed(0)
    model = baselines.GCN(shape["x"].shape[1], shape["hidden"], shape["classes"], P_DROP, mt).to(DEV)
    model.fused = fused                                       # "always" | True | False
    if kind == "gcn_project_first":
        for layer in model.gcns:
            layer.eval_agg_cache = False
    opt = FusedAdam(model.parameters(), lr=LR, weight_decay=WD)
    w = T.row_weights(shape["train"], shape["x"].shape[0], device=DEV)
    eager = T.TrainStep(model, opt, shape["x"], shape["ops"], shape["y"], w)
    eager()                                                   # (one eager step also proves the tape)
    captured = T.TrainStep(model, opt, shape["x"], shape["ops"], shape["y"], w, use_graph=True)
    return captured, eager, True


def kernels_per_step(step):
    """(GPU kernels + memsets the profiler saw in one eager step, this library's launches in it)."""
    probe = AF.KernelTimer()
    AF.set_kernel_timer(probe)
    try:
        step()
        ours = sum(k for k, _ in probe.summary().values())
    finally:
        AF.set_kernel_timer(None)
    total = None
    try:                                                      # (a profiler that cannot count is reported in the row, not hidden)
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            step()
            torch.cuda.synchronize()
        total = sum(1 for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA"))
    except Exception as exc:
        total = f"profiler failed: {type(exc).__name__}"
    return total, ours


def window(run, seconds):
    """ms per call over a window of at least ``seconds`` (device events)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    calls, batch, total = 0, 16, 0.0
    while total < seconds * 1e3:
        a.record()
        for _ in range(batch):
            run()
        b.record()
        torch.cuda.synchronize()
        total += a.elapsed_time(b)
        calls += batch
        batch = min(batch * 2, 4096)
    return total / calls


def bench(shape, kinds, seconds, repeats):
    for kind in kinds:
        arms = {"fused": package_arm(kind, shape, "always"), "composed": package_arm(kind, shape, False)}
        if kind != "sgc" and not AF.gcn.fusion_pays(shape["ops"].low):
            arms["default"] = package_arm(kind, shape, True)
        arms["fused_eager"] = (arms["fused"][1], arms["fused"][1], False)
        if kind != "gcn_project_first":
            try:
                arms["torch"] = torch_arm(kind, shape)
            except Exception as exc:                              # (this torch build lacks an op of the arm: reported, not timed)
                print(json.dumps({"shape": shape["name"], "model": kind, "arm": "torch", "error": f"{type(exc).__name__}: {exc}"[:200]}), flush=True)
        counts = {name: kernels_per_step(arm[1]) for name, arm in arms.items()}
        for run, _, _ in arms.values():
            window(run, seconds)                                  # warm-up by time
        times = {name: [] for name in arms}
        for _ in range(repeats):
            for name, (run, _, _) in arms.items():
                times[name].append(window(run, seconds))
        for name, (_, _, captured) in arms.items():
            t = times[name]
            print(json.dumps({"shape": shape["name"], "nodes": shape["x"].shape[0], "features": shape["x"].shape[1], "hidden": shape["hidden"],
                              "classes": shape["classes"], "model": kind, "arm": name, "captured": captured,
                              "ms_per_step": round(statistics.median(t), 4), "ms_range": [round(min(t), 4), round(max(t), 4)],
                              "kernels_per_step": counts[name][0], "library_launches": counts[name][1]}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("shapes", nargs="*", default=["study", "twitch"])
    ap.add_argument("--seconds", type=float, default=0.4)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--models", default="gcn,sgc,gcn_project_first")
    args = ap.parse_args()
    assert torch.cuda.is_available(), "bench_baselines.py needs the GPU"
    for nm in args.shapes:
        bench({"study": study_shape, "twitch": twitch_shape}[nm](), args.models.split(","), args.seconds, args.repeats)
