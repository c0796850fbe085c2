"""Every copy of the mixing head where random inputs never take it: saturated sigmoids, near one-hot softmax, LayerNorm variances
far below eps, rows that are exactly zero (tests/head_regimes.py builds the cases and states what they reach; the CPU module
tests/test_head_regimes_cpu.py asserts those statements).  MI355X box.

The comparison rule (head_regimes.compare): for every tensor t on its own -- the output, the mixing weights, dX where the route
returns it, every parameter gradient, the loss and d-logits where a loss is part of the launch --

    max |kernel(t) - oracle64(t)|  <=  M * max(e32(t), 2^-23 max |oracle64(t)|),

e32(t) = max |oracle32(t) - oracle64(t)|, the float32 oracle's own error on the same inputs.  No absolute floor, no pooling, and
nothing is left out of a comparison (head_regimes.mask_safety is why that is fair).

M = 32 for every route, the bf16 mask form of ACMII included (exact products of a 0/1 operand with a three-way bf16
split of the fp32 operand, fp32 accumulation -- no route here is of deliberately lower precision, so there is one M).  Measured
on the MI355X over all cases below (EXPERIMENTS.md, "The mixing head off centre", has the table per route and tensor class): the
largest err / unit was 28.5 (d att_vec_low of the four-rows epilogue at 12 -> 64, four channels, LayerNorm; the sixteen-rows stage
on the same case: 19.9), rounded up to the next power of two.  The margin is what another summation order and the 1-ulp hardware
exp / rcp / rsq cost on sums whose terms cancel; the altered heads of tests/test_head_regimes_cpu.py exceed the unit by 7e4 .. 2e8.
"""
import numpy as np
import pytest
import scipy.sparse as sp
import torch

import head_regimes as H
from conftest import tune_now as tune

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M = H.M
F64, F32 = torch.float64, torch.float32


def _log(line):
    print(line)


def _used(timer):
    return {k.split("/")[0] for k in timer.events}


def _load(module, params):
    sd = module.state_dict()
    with torch.no_grad():
        for k, v in params.items():
            assert tuple(sd[k].shape) == tuple(v.shape), k
            sd[k].copy_(v)


def _layer_of(case, **kw):
    from acm_gnn_amd import GraphConvolution
    layer = GraphConvolution(case.f_in, case.f_out, case.n, case.model_type, variant=bool(case.variant), structure_info=case.structure_info,
                             attn_layernorm=case.attn_layernorm, **kw)
    _load(layer, case.params)
    return layer.to(DEV)


def _layer_results(layer, case, out, x=None):
    att = [layer.att_low, layer.att_high, layer.att_mlp] + ([layer.att_struc_vec_low] if case.k == 4 else [])
    got = {"out": out.detach(), "att": torch.cat(att, 1)}
    if x is not None:
        got["dX"] = x.grad
    got.update({f"grad:{k}": p.grad for k, p in layer.named_parameters() if p.grad is not None})
    return got


def _run_case(spec, monkeypatch):
    """The stressed case ``spec`` names through the layer, forced onto ``spec.route`` by its tuning switches; the kernels that ran
    are asserted from the kernel timer's labels, the results compared by the rule of the module docstring."""
    from acm_gnn_amd import functional as AF
    from acm_gnn_amd.graph import clear_cache, operators_for
    case = H.case_of(spec.args)
    tune(**spec.tune)
    if spec.force == "wide":
        # functional.agg_wide_supported takes the form from 8192 rows and a mean degree of 12 on (where it pays); the kernels
        # themselves take any row count, and the head in them is what this case is about
        from acm_gnn_amd.functional import conv
        monkeypatch.setattr(conv, "_conv_route", lambda *a, **k: "wide")
    clear_cache()
    layer = _layer_of(case)
    x = case.x.to(DEV).requires_grad_(spec.x_grad)
    low, high, un = case.low.to(DEV), case.high.to(DEV), case.un.to(DEV) if case.k == 4 else None
    assert operators_for(low, high, un).implicit == bool(spec.implicit)
    timer = AF.KernelTimer()
    AF.set_kernel_timer(timer)
    try:
        out = layer(x, low, high, un)
        out.backward(case.gout.to(DEV))
    finally:
        AF.set_kernel_timer(None)
    used = _used(timer)
    assert spec.expect <= used and not (spec.forbid & used), (spec.id, sorted(used))
    got = _layer_results(layer, case, out, x if spec.x_grad else None)
    ref64, ref32 = H.oracle_run(case.key, F64), H.oracle_run(case.key, F32)
    assert set(got) == set(ref64) - (set() if spec.x_grad else {"dX"}), sorted(set(got) ^ set(ref64))
    H.compare(got, ref64, ref32, M, spec.id, _log)


@pytest.mark.parametrize("spec", H.layer_cases(), ids=lambda s: s.id)
def test_layer_head_off_centre(spec, monkeypatch):
    _run_case(spec, monkeypatch)


# ---- the loss on the magnitudes the stressed layer produces ----------------------------------------------------------------
@pytest.mark.parametrize("args", H.NLL_ARGS, ids=lambda a: f"{a[5]}classes")
def test_masked_nll_on_logits_of_a_row_range_beyond_100(args):
    """acm_nll_loss on the stressed layer's output (per-row range > 100 on several loss rows; rows labelled -1 carry weight 0):
    loss and d-logits against float64 log_softmax.  (tests/test_gpu_train.py::test_masked_nll_kernel has logits of 3 randn.)"""
    from acm_gnn_amd import functional as AF
    case = H.case_of(args)
    y, w = H.loss_rows(case.n, case.f_out, case.seed)
    z = H.oracle_run(case.key, F64)["out"].float().to(DEV).requires_grad_(True)
    timer = AF.KernelTimer()
    AF.set_kernel_timer(timer)
    try:
        loss = AF.masked_nll(z, y.to(DEV), w.to(DEV))
        loss.backward()
    finally:
        AF.set_kernel_timer(None)
    assert "nll_loss" in _used(timer)
    got = {"loss": loss.detach(), "dlogits": z.grad}
    assert float(z.grad[w.to(DEV) == 0].abs().max()) == 0.0
    H.compare(got, H.nll_reference(args, F64), H.nll_reference(args, F32), M, f"nll_loss-{case.f_out}classes", _log)


@pytest.mark.parametrize("args", H.TAIL_ARGS, ids=lambda a: f"{a[0]}-{a[5]}classes")
def test_fused_loss_tail_on_the_stressed_output_layer(args):
    """acm_conv_fwd_tail (the output layer's head, the masked NLL and K3 in one row pass: a head copy of its own) on the stressed
    case as an output layer: loss, d-logits, logits, mixing weights and every gradient against the float64 oracle."""
    from acm_gnn_amd import functional as AF
    from acm_gnn_amd.graph import clear_cache
    case = H.case_of(args)
    y, w = H.loss_rows(case.n, case.f_out, case.seed)
    clear_cache()
    layer = _layer_of(case, output_layer=1)
    timer = AF.KernelTimer()
    AF.set_kernel_timer(timer)
    try:
        with AF.fused_loss_tail(y.to(DEV), w.to(DEV)) as tail:
            out = layer(case.x.to(DEV), case.low.to(DEV), case.high.to(DEV), None)
        assert tail.matches(out), "the output layer did not take the request"
        out.backward(tail.dz)
    finally:
        AF.set_kernel_timer(None)
    used = _used(timer)
    assert "conv_fwd_tail" in used and "conv_fwd" not in used and "nll_loss" not in used and "conv_bwd_local" not in used, sorted(used)
    got = _layer_results(layer, case, out)
    got.update(loss=tail.loss, dlogits=tail.dz)
    ref64, ref32 = H.tail_reference(args, F64), H.tail_reference(args, F32)
    assert set(got) == set(ref64), sorted(set(got) ^ set(ref64))
    H.compare(got, ref64, ref32, M, f"loss-tail-{case.model_type}-{case.f_out}classes", _log)


# ---- the small-graph step (acm_small.hip: expf / 1/sqrtf heads of its own, single and batched) ---------------------------------
def _small_setup(small):
    from acm_gnn_amd import SparseFeatures, data as D, train as T
    from acm_gnn_amd.distributed import make_sharded_operators
    low, deg = D.build_filters(sp.csr_matrix(small.adj, dtype=np.float32))
    ops = make_sharded_operators(low, deg, torch.device(DEV), with_structure=small.k == 4)
    xs = SparseFeatures.from_scipy(sp.csr_matrix(small.x.numpy()), DEV)
    y = small.y.to(DEV)
    w = T.row_weights(small.train.to(DEV), small.n)
    return ops, xs, y, w


def _small_model(small):
    from acm_gnn_amd import GCN
    model = GCN(H.SMALL_F_IN, 64, H.SMALL_CLASSES, 2, small.n, 0.0, small.model_type, small.structure_info, variant=False,
                attn_layernorm=small.attn_layernorm)
    _load(model, small.params)
    return model.to(DEV)


def _plan_results(plan, k, train):
    got = {"logits": plan.logits, "att1": plan.att1[:, :k], "att2": plan.att2[:, :k]}
    if train:
        got["loss"] = plan.loss
        got.update({f"grad:gcns.{li}.{name}": g for (li, name), g in plan.grads.items()})
    return {name: v.detach().clone() for name, v in got.items()}


@pytest.mark.parametrize("name", list(H.SMALL_CONFIGS))
def test_small_graph_step_with_both_heads_off_centre(name):
    """acm_small_step on a two-layer model whose both layers carry the stressed head parameters: the training step's loss,
    logits, mixing weights of both layers and every gradient (read as tests/test_gpu_small.py reads them: a plan that stops at
    the gradients), then the three-launch evaluation pass, against O.gcn_forward in float64."""
    from acm_gnn_amd import functional as AF
    from acm_gnn_amd.small import SmallPlan
    small = H.build_small(name)
    ops, xs, y, w = _small_setup(small)
    model = _small_model(small)
    model.train()
    assert SmallPlan.why_not(model, xs, ops) is None
    ref64, ref32 = H.small_reference(name, F64), H.small_reference(name, F32)
    timer = AF.KernelTimer()
    AF.set_kernel_timer(timer)
    try:
        plan = SmallPlan(model, xs, ops, y, w, optimizer=None, update=False)
        plan.run()
        torch.cuda.synchronize()
        got = _plan_results(plan, small.k, True)
        model.eval()
        ev = SmallPlan(model, xs, ops)
        ev.run()
        torch.cuda.synchronize()
        got_eval = _plan_results(ev, small.k, False)
    finally:
        AF.set_kernel_timer(None)
    assert {"small_step", "small_forward"} <= _used(timer), sorted(_used(timer))
    assert set(got) == set(ref64), sorted(set(got) ^ set(ref64))
    H.compare(got, ref64, ref32, M, f"small-step-{name}", _log)
    H.compare(got_eval, ref64, ref32, M, f"small-forward-{name}", _log)


def test_batched_small_graph_step_is_the_single_step_on_the_stressed_slot():
    """Two slots through acm_small_batch_step, the stressed model second (the first: the same draws without the gains): every
    result of each slot bit for bit what the single step leaves -- loss, logits, mixing weights, gradients, updated parameters."""
    from acm_gnn_amd import FusedAdam, functional as AF
    from acm_gnn_amd.small import SmallBatch, SmallPlan
    name = "acmgcnp-k4-ln"
    smalls = [H.build_small(name, False), H.build_small(name)]
    ops, xs, y, w = _small_setup(smalls[1])

    def runs():
        out = []
        for small in smalls:
            model = _small_model(small)
            model.train()
            opt = FusedAdam(model.parameters(), lr=0.01, weight_decay=0.0)
            assert SmallPlan.why_not(model, xs, ops, opt) is None
            out.append((model, SmallPlan(model, xs, ops, y, w, optimizer=opt, keep_grads=True)))
        return out

    single, batched = runs(), runs()
    timer = AF.KernelTimer()
    AF.set_kernel_timer(timer)
    try:
        for _, plan in single:
            plan.run()
        SmallBatch([plan for _, plan in batched]).run()
        torch.cuda.synchronize()
    finally:
        AF.set_kernel_timer(None)
    assert {"small_step", "small_batch_step"} <= _used(timer), sorted(_used(timer))
    for slot, ((ma, pa), (mb, pb)) in enumerate(zip(single, batched)):
        a, b = _plan_results(pa, smalls[slot].k, True), _plan_results(pb, smalls[slot].k, True)
        assert a.keys() == b.keys() and len(a) > 10
        for key in a:
            assert torch.equal(a[key], b[key]), (slot, key)
        for (key, va), (_, vb) in zip(ma.state_dict().items(), mb.state_dict().items()):
            assert torch.equal(va, vb), (slot, key)
    # ... and the stressed slot's step is the one the rule accepts against float64
    ref64, ref32 = H.small_reference(name, F64), H.small_reference(name, F32)
    H.compare(_plan_results(batched[1][1], smalls[1].k, True), ref64, ref32, M, f"small-batch-step-{name}", _log)
