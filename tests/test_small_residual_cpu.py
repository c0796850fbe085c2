"""ACM-GCN++ on the small-graph step, everything that needs no GPU: every branch of ``SmallPlan.why_not`` for the residual
model (a library without the probe is never offered one), the binding of the Linear's weight and bias (parameter, optimizer
state, gradient) and its renewal after a tensor was replaced, ``drop_res`` (tag 2, the operator's row offset), the workspace
sized by the entry that takes the shape, the batched forms' refusal with ``fit_batched``'s documented fall-back, the layout of
the fields appended to ``acm_small_step_t`` against a C program compiled from the header, the real library's refusals that
need no device, and -- on the CPU double with a small step that reads the residual (tests/fake_lib_residual.py) -- a training
run on the small path against the general path."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import fake_lib_residual
from select_ref import same_floats
from small_batch_double import install_batch
from test_resident_fit_cpu import _np_copy_if, _np_select_step, _problem

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _install(monkeypatch):
    fake = fake_lib_residual.install(monkeypatch)
    fake.acm_select_step, fake.acm_copy_if = _np_select_step, _np_copy_if
    from acm_gnn_amd import train as T
    monkeypatch.setattr(T.TrainStep, "_capture", lambda self: None)
    monkeypatch.setattr(T.EvalStep, "_capture", lambda self: None)
    return install_batch(fake)


def _make(hidden=64, n=90, p_drop=0.0, **kw):
    from acm_gnn_amd import GCN, FusedAdam, functional as AF

    def make(k):
        torch.manual_seed(k)
        model = GCN(50, hidden, 3, 2, n, p_drop, "acmgcnpp", 0, **kw)
        if p_drop > 0:
            model.fused_dropout = True
            model.dropout_state = AF.DropoutState(torch.device("cpu"), seed=1000 + k)
        idx = torch.randperm(n, generator=torch.Generator().manual_seed(k))
        return model, FusedAdam(model.parameters(), lr=0.05), idx[:40], idx[40:65], idx[65:]
    return make


def test_a_library_without_the_probe_is_never_offered_the_model(monkeypatch):
    import fake_lib
    fake_lib.install(monkeypatch)                       # the double as it stands: no acm_small_step_has_residual
    from acm_gnn_amd import small
    from acm_gnn_amd.small import SmallPlan
    assert not small.has_residual()
    ops, xs, y, _ = _problem()
    model, opt = _make()(0)[:2]
    want = "model_type 'acmgcnpp' (acmgcn | acmgcnp): library without the residual step"
    assert SmallPlan.why_not(model, xs, ops, opt) == want and SmallPlan.why_not(model, xs, ops) == want


def test_why_not_takes_the_default_model_and_names_what_it_refuses(monkeypatch):
    _install(monkeypatch)
    from acm_gnn_amd import FusedAdam, small
    from acm_gnn_amd.small import SmallPlan
    assert small.has_residual()
    ops, xs, y, _ = _problem()
    for hidden in (32, 64):
        for kw in ({}, dict(variant=True), dict(attn_layernorm=True)):
            model, opt = _make(hidden, **kw)(0)[:2]
            assert SmallPlan.why_not(model, xs, ops, opt) is None, (hidden, kw)
            assert SmallPlan.why_not(model, xs, ops) is None                       # an evaluation plan
    model, opt = _make(init_layers_X=2)(0)[:2]
    assert SmallPlan.why_not(model, xs, ops, opt) == "mlpX with 2 Linears (init_layers_X = 1 only)"
    model, _ = _make()(0)[:2]
    lin = model.mlpX.lins[0]
    model.mlpX.lins[0] = torch.nn.Linear(lin.in_features, lin.out_features, bias=False)
    assert SmallPlan.why_not(model, xs, ops) == "mlpX Linear without bias"
    model.mlpX.lins[0] = torch.nn.Linear(lin.in_features, 48)
    assert SmallPlan.why_not(model, xs, ops) == "mlpX Linear 50 -> 48 (the first layer is 50 -> 64)"
    model.mlpX.lins[0] = torch.nn.Linear(40, 64)
    assert SmallPlan.why_not(model, xs, ops) == "mlpX Linear 40 -> 64 (the first layer is 50 -> 64)"
    model.mlpX.lins[0] = torch.nn.Linear(50, 64).double()
    assert SmallPlan.why_not(model, xs, ops) == "parameters: contiguous fp32 on the features' device"
    model, _ = _make()(0)[:2]
    opt = FusedAdam(list(model.gcns.parameters()), lr=0.1)                        # the layers' parameters, not mlpX's
    assert SmallPlan.why_not(model, xs, ops, opt) == "a parameter of mlpX is not in the optimizer's group"
    opt = FusedAdam(list(model.gcns.parameters()) + [model.mlpX.lins[0].weight], lr=0.1)
    assert SmallPlan.why_not(model, xs, ops, opt) == "a parameter of mlpX is not in the optimizer's group"
    # a model_type outside the family still names the family
    model.model_type = "acmsgc"
    assert SmallPlan.why_not(model, xs, ops) == "model_type 'acmsgc' (acmgcn | acmgcnp | acmgcnpp)"


def test_the_plan_binds_the_two_tensors_and_binds_them_again(monkeypatch):
    fake = _install(monkeypatch)
    from acm_gnn_amd import train as T
    from acm_gnn_amd.small import SmallPlan
    ops, xs, y, _ = _problem()
    w = T.row_weights(torch.arange(40), 90)
    model, opt = _make(32)(0)[:2]
    lin = model.mlpX.lins[0]
    plan = SmallPlan(model, xs, ops, y, w, opt, keep_grads=True)
    p = plan.p
    assert plan.residual and p.residual == 1 and p.hidden == 32
    assert plan.workspace.numel() * 4 == 4096 + fake_lib_residual.RESIDUAL_EXTRA_BYTES       # sized by the entry that takes the shape
    assert (p.res[0].param, p.res[1].param) == (lin.weight.data_ptr(), lin.bias.data_ptr())
    assert (p.res[0].numel, p.res[1].numel) == (32 * 50, 32)
    gw, gb = plan.grads[("mlpX", "weight")], plan.grads[("mlpX", "bias")]
    assert gw.shape == (32, 50) and gb.shape == (32,)
    assert (p.res[0].grad, p.res[1].grad) == (gw.data_ptr(), gb.data_ptr())
    for k, t in enumerate((lin.weight, lin.bias)):
        st = opt.state[t]
        assert (p.res[k].exp_avg, p.res[k].exp_avg_sq, p.res[k].step) == (st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr())
    # the roles of the two layers are untouched by the residual's binding
    assert p.t[0][0].param == model.gcns[0].weight_low.data_ptr() and p.t[1][0].param == model.gcns[1].weight_low.data_ptr()
    assert not plan.stale()
    # a state tensor replaced (load_state_dict makes new ones), then a parameter's storage
    opt.state[lin.weight]["exp_avg"] = opt.state[lin.weight]["exp_avg"].clone()
    assert plan.stale()
    plan.run()
    assert not plan.stale() and p.res[0].exp_avg == opt.state[lin.weight]["exp_avg"].data_ptr()
    lin.bias.data = lin.bias.data.clone()
    assert plan.stale()
    plan.run()
    assert not plan.stale() and p.res[1].param == lin.bias.data_ptr()
    assert fake.small_residual_calls == 2
    # a gradient-only plan: no optimizer state is touched, the gradients are there
    model2, _ = _make(64)(1)[:2]
    plan2 = SmallPlan(model2, xs, ops, y, w, optimizer=None, update=False)
    assert plan2.p.residual == 1 and plan2.p.update == 0 and plan2.p.res[0].exp_avg is None and plan2.p.res[0].grad
    plan2.run()
    assert float(plan2.grads[("mlpX", "weight")].abs().max()) > 0 and float(plan2.grads[("mlpX", "bias")].abs().max()) > 0
    # an evaluation plan carries the residual too (four launches on the device)
    ev = SmallPlan(model2, xs, ops)
    assert ev.p.residual == 1 and ev.p.train == 0 and ev.p.res[0].param == model2.mlpX.lins[0].weight.data_ptr()
    # a model without the branch: residual 0, the stock workspace size, nothing bound
    from acm_gnn_amd import GCN, FusedAdam
    plain = GCN(50, 64, 3, 2, 90, 0.0, "acmgcnp", 0)
    plan3 = SmallPlan(plain, xs, ops, y, w, FusedAdam(plain.parameters(), lr=0.1))
    assert not plan3.residual and plan3.p.residual == 0 and plan3.p.res[0].param is None and plan3.workspace.numel() * 4 == 4096


def test_drop_res_carries_tag_2_and_the_operators_row_offset(monkeypatch):
    fake = _install(monkeypatch)
    from acm_gnn_amd import train as T
    from acm_gnn_amd.small import SmallPlan
    ops, xs, y, _ = _problem()
    w = T.row_weights(torch.arange(40), 90)
    model, opt = _make(64, p_drop=0.5)(0)[:2]
    plan = SmallPlan(model, xs, ops, y, w, opt)
    d = plan.p.drop_res
    assert (d.tag, d.row_offset, d.seed, d.step) == (2, ops.row_offset, model.dropout_state.seed, model.dropout_state.step.data_ptr())
    assert abs(d.p - 0.5) < 1e-7 and plan.p.drop_hidden.tag == 1 and plan.p.drop_in.tag == 0
    monkeypatch.setattr(ops, "row_offset", 17, raising=False)
    plan.refresh_hyper()
    assert plan.p.drop_res.row_offset == 17 and plan.p.drop_hidden.row_offset == 17 and plan.p.drop_in.row_offset == 0
    monkeypatch.setattr(ops, "row_offset", 0, raising=False)
    plan.run()
    assert fake.small_drop_res == (0.5, 2, 0)
    # evaluation: no dropout at all
    ev = SmallPlan(model, xs, ops)
    assert ev.p.drop_res.p == 0 and ev.p.drop_hidden.p == 0
    # a model without dropout: the field stays empty
    model0, opt0 = _make(64)(0)[:2]
    assert SmallPlan(model0, xs, ops, y, w, opt0).p.drop_res.p == 0


def test_training_on_the_small_path_equals_the_general_path_on_the_double(monkeypatch):
    fake = _install(monkeypatch)
    from acm_gnn_amd import train as T
    ops, xs, y, _ = _problem()
    w = T.row_weights(torch.arange(40), 90)

    def run(small, p_drop):
        model, opt = _make(32, p_drop=p_drop)(3)[:2]
        step = T.TrainStep(model, opt, xs, ops, y, w, small_step=None if small else False)
        assert (step.small is not None) == small, step.small_refused
        losses = [float(step()) for _ in range(5)]
        return model, opt, losses

    for p_drop in (0.0, 0.5):
        fake.small_residual_calls = 0
        (ma, oa, la), (mb, ob, lb) = run(True, p_drop), run(False, p_drop)
        assert fake.small_residual_calls == 5
        np.testing.assert_allclose(la, lb, rtol=2e-4, atol=1e-6)
        assert la[-1] < la[0]
        for (k, pa), (_, pb) in zip(ma.state_dict().items(), mb.state_dict().items()):
            torch.testing.assert_close(pa, pb, rtol=5e-3, atol=5e-4, msg=k)
        for name in ("weight", "bias"):
            ta, tb = getattr(ma.mlpX.lins[0], name), getattr(mb.mlpX.lins[0], name)
            assert float(oa.state[ta]["step"]) == float(ob.state[tb]["step"]) == 5.0
            torch.testing.assert_close(oa.state[ta]["exp_avg"], ob.state[tb]["exp_avg"], rtol=5e-3, atol=1e-5)
        if p_drop > 0:
            assert int(ma.dropout_state.step.item()) == int(mb.dropout_state.step.item()) == 5


def test_fit_keeps_the_best_mlpX_tensors(monkeypatch):
    """fit(keep_best=True) snapshots and restores the model's parameters by iterating them: the Linear's two are among them."""
    _install(monkeypatch)
    from acm_gnn_amd import train as T
    ops, xs, y, _ = _problem()
    model, opt, tr, va, te = _make(64)(2)
    sel, hist = T.fit(model, opt, xs, ops, y, tr, va, te, 8, use_graph=True, keep_best=True, sync_every=4)
    assert len(hist) == 8
    ev = T.EvalStep(model, xs, ops, y, (tr, va, te))
    assert ev.small is not None and ev.small.residual
    _, accs, _ = ev()
    assert abs(accs[2] - sel) < 1e-6                    # the model left behind is the selected epoch's


def test_the_batched_forms_refuse_residual_plans_and_fit_batched_falls_back(monkeypatch):
    fake = _install(monkeypatch)
    from acm_gnn_amd import train as T
    from acm_gnn_amd.small import SmallBatch, SmallGraphBatch, SmallPlan
    ops, xs, y, _ = _problem()
    make = _make(32)
    w = T.row_weights(torch.arange(40), 90)
    plans = [SmallPlan(m, xs, ops, y, w, o) for m, o in (make(k)[:2] for k in range(2))]
    for Batch in (SmallBatch, SmallGraphBatch):
        why = Batch.why_not(plans)
        assert why is not None and "residual" in why
        assert "residual" in Batch.why_not(plans[:1])
        with pytest.raises(ValueError, match="residual"):
            Batch(plans)
    want = T.fit_concurrent([make(k) for k in range(3)], xs, ops, y, epochs=5, rule="min_val_loss", sync_every=4)
    fake.small_batch_calls = 0
    got = T.fit_batched([make(k) for k in range(3)], xs, ops, y, 5, rule="min_val_loss", batch=2, sync_every=4)
    why = T.fit_batched.last_refusal
    assert why is not None and "residual" in why, why
    assert fake.small_batch_calls == 0 and fake.small_residual_calls > 0          # run by run, each on the (single) small path
    for k in range(3):
        assert same_floats(got[k][0], want[k][0]) and same_floats(got[k][1], want[k][1]), k


def _host_program(tmp_path):
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = tmp_path / "small_residual_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "acm_gnn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_abi", "small_residual_host.cpp"), "-o", str(exe)])
    return exe


def test_the_slot_checks_refuse_a_residual_slot_and_the_struct_mirror_agrees(tmp_path):
    """tests/c_abi/small_residual_host.cpp, built with AddressSanitizer and UBSan for the host as a stand-alone program: the slot
    checks of both batch flavours refuse ``residual``; the offsets it prints from the header are the ctypes mirror's."""
    from acm_gnn_amd import _lib
    exe = _host_program(tmp_path)
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "small_residual_host: ok" in out.stdout, (out.stdout, out.stderr)
    out = subprocess.run([str(exe), "--offsets"], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    S = _lib.SmallStep
    assert [int(v) for v in out.stdout.split()] == [S.residual.offset, S.workspace_bytes.offset, S.res.offset, S.drop_res.offset, C.sizeof(S)]
    # `residual` is where reserved1 was; the new fields lie behind what was the block's end
    assert S.residual.offset == S.f_in.offset + 4 and S.residual.size == 4
    assert S.res.offset == S.workspace_bytes.offset + 8 and S.drop_res.offset == S.res.offset + 2 * C.sizeof(_lib.AdamTensor)
    assert C.sizeof(S) == S.drop_res.offset + C.sizeof(_lib.Dropout)


def test_the_real_library_has_the_entry_points_and_refuses_before_any_launch():
    from acm_gnn_amd import _lib, small
    lib = _lib.load()
    assert {"acm_small_step_has_residual", "acm_small_step_workspace_bytes_for"} <= set(_lib.EXPORTED_SYMBOLS)
    assert int(lib.acm_small_step_has_residual()) == 1 and small.has_residual(lib)
    p = _lib.SmallStep()
    p.n_classes, p.n_channels, p.f_in, p.scale = 3, 3, 7, 3.0
    # zero-filled host memory stands in for the handles and the table (tests/test_small_hidden_cpu.py): every refusal below
    # comes before a handle's fields beyond the row count, or a byte of the table, is touched
    handle, handle_x, table = (C.create_string_buffer(1 << 16) for _ in range(3))
    for bad in (2, -1, 7):
        p.residual = bad
        assert lib.acm_small_step(handle, None, None, C.byref(p), None) == 1           # ACM_EINVAL
        assert b"residual must be 0 or 1" in lib.acm_last_error()
        nbytes = C.c_size_t(12345)
        assert lib.acm_small_step_workspace_bytes_for(handle, None, None, C.byref(p), C.byref(nbytes)) == 1 and nbytes.value == 12345
    p.residual = 1                                       # set, and no parameter behind it
    assert lib.acm_small_step(handle, None, None, C.byref(p), None) == 1
    assert b"residual without its parameters" in lib.acm_last_error()
    one = C.c_float()
    p.res[0].param = C.addressof(one)                    # the weight alone
    assert lib.acm_small_step(handle, None, None, C.byref(p), None) == 1
    assert b"residual without its parameters" in lib.acm_last_error()
    p.res[1].param = C.addressof(one)
    slots = (C.POINTER(_lib.SmallStep) * 1)(C.pointer(p))
    assert lib.acm_small_batch_bind(handle, None, None, 1, slots, table, len(table), None) == 4     # ACM_EUNSUPPORTED
    assert b"residual" in lib.acm_last_error()
    rows = (C.c_void_p * 1)(C.addressof(handle))
    grids = _lib.SmallBatchGrids()
    assert lib.acm_small_batch_bind_graphs(1, rows, rows, rows, slots, C.byref(grids), table, len(table), None) == 4
    assert b"residual" in lib.acm_last_error()
    assert lib.acm_small_batch_step(handle, handle_x, None, 1, C.byref(p), table, None) == 4
    assert b"residual" in lib.acm_last_error()
    assert lib.acm_small_batch_step_graphs(1, C.byref(p), C.byref(grids), table, None) == 4
    assert b"residual" in lib.acm_last_error()
    assert handle.raw == handle_x.raw == table.raw == bytes(1 << 16)
