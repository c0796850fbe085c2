"""Deep mlpX stacks (init_layers_X > 1: Linear -> ReLU -> BatchNorm1d between the Linears) on the acm_bnorm_* entry points,
without a GPU: the numpy restatement (tests/mlp_stack_ref.py) against the reference's own module (recorded in
tests/golden/mlp_stack_cases.npz), functional.residual_mlp on the extended test double against the restatement -- training and
evaluation mode, dense / padded dense / CSR features, on the Tape and under autograd, with the first bias gradient deferred --
and the envelope: what lies outside it, and CPU tensors on the stock double, keep running on the torch modules."""
import os

import numpy as np
import pytest
import torch

import fake_lib
import mlp_stack_ref as R
from conftest import ROOT, graph_tensors

GOLDEN = os.path.join(ROOT, "tests", "golden", "mlp_stack_cases.npz")
# the double computes in float64 and stores fp32: a handful of fp32 roundings per value
TOL = 2e-5


def _case(g, name):
    n, f_in, hid, f_out, n_lins, dead = (int(v) for v in g[f"{name}:shape"])
    lins = [(g[f"{name}:W{i}"], g[f"{name}:b{i}"]) for i in range(n_lins)]
    bns = [(g[f"{name}:gamma{i}"], g[f"{name}:beta{i}"]) for i in range(n_lins - 1)]
    return n, f_in, hid, f_out, n_lins, dead, lins, bns


def _close(got, want, tol, what=""):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    err = np.abs(got - want) / np.maximum(1.0, np.abs(want))
    assert got.shape == want.shape and float(err.max(initial=0.0)) <= tol, (what, float(err.max(initial=0.0)))


def test_restatement_equals_the_reference_module():
    g = np.load(GOLDEN)
    assert sorted(g["cases"]) == ["deep3", "tiny2", "wide2"]
    for name in g["cases"]:
        n, f_in, hid, f_out, n_lins, dead, lins, bns = _case(g, name)
        assert n <= 257 and max(f_in, hid, f_out) <= 24 and n_lins in (2, 3)
        running = [(np.zeros(hid), np.ones(hid)) for _ in bns]
        y, cache, running = R.forward(g[f"{name}:x"], lins, bns, True, running)
        _close(y, g[f"{name}:y"], 1e-12, f"{name} y")
        if dead >= 0:                                        # a unit that never fires: variance 0, xhat 0, the output is beta
            assert np.all(cache[0][2][:, dead] == 0.0)
        dx, d_lins, d_bns = R.backward(g[f"{name}:dy"], lins, bns, cache)
        for i in range(n_lins):
            _close(d_lins[i][0], g[f"{name}:dW{i}"], 1e-11, f"{name} dW{i}")
            _close(d_lins[i][1], g[f"{name}:db{i}"], 1e-11, f"{name} db{i}")
        for i in range(n_lins - 1):
            _close(d_bns[i][0], g[f"{name}:dgamma{i}"], 1e-11, f"{name} dgamma{i}")
            _close(d_bns[i][1], g[f"{name}:dbeta{i}"], 1e-11, f"{name} dbeta{i}")
            _close(running[i][0], g[f"{name}:rm1_{i}"], 1e-12)
            _close(running[i][1], g[f"{name}:rv1_{i}"], 1e-12)
            assert int(g[f"{name}:nbt1_{i}"]) == 1 and int(g[f"{name}:nbt3_{i}"]) == 3
        for _ in range(2):
            _, _, running = R.forward(g[f"{name}:x"], lins, bns, True, running)
        for i in range(n_lins - 1):
            _close(running[i][0], g[f"{name}:rm3_{i}"], 1e-12)
            _close(running[i][1], g[f"{name}:rv3_{i}"], 1e-12)
        y_eval, _, _ = R.forward(g[f"{name}:x"], lins, bns, False, running)
        _close(y_eval, g[f"{name}:y_eval"], 1e-12, f"{name} eval")


def test_torch_restatement_equals_the_numpy_one():
    g = np.load(GOLDEN)
    for name in g["cases"]:
        n, f_in, hid, f_out, n_lins, dead, lins, bns = _case(g, name)
        tl = [tuple(torch.from_numpy(t).requires_grad_(True) for t in p) for p in lins]
        tb = [tuple(torch.from_numpy(t).requires_grad_(True) for t in p) for p in bns]
        y = torch.relu(R.forward_torch(torch.from_numpy(g[f"{name}:x"]), tl, tb))
        (y * torch.from_numpy(g[f"{name}:dy"])).sum().backward()
        _close(y.detach().numpy(), g[f"{name}:y"], 1e-12)
        for i in range(n_lins):
            _close(tl[i][0].grad.numpy(), g[f"{name}:dW{i}"], 1e-11)
        for i in range(n_lins - 1):
            _close(tb[i][0].grad.numpy(), g[f"{name}:dgamma{i}"], 1e-11)
            _close(tb[i][1].grad.numpy(), g[f"{name}:dbeta{i}"], 1e-11)


def _mlp_from(lins, bns, f_in, hid, f_out):
    from acm_gnn_amd.layers import MLP
    mlp = MLP(f_in, hid, f_out, len(lins), dropout=0)
    with torch.no_grad():
        for lin, (w, b) in zip(mlp.lins, lins):
            lin.weight.copy_(torch.from_numpy(w).float())
            lin.bias.copy_(torch.from_numpy(b).float())
        for bn, (gm, bt) in zip(mlp.bns, bns):
            bn.weight.copy_(torch.from_numpy(gm).float())
            bn.bias.copy_(torch.from_numpy(bt).float())
    return mlp


def _as32(pairs):
    return [tuple(np.asarray(t, np.float32).astype(np.float64) for t in p) for p in pairs]


@pytest.mark.parametrize("kind", ["dense", "padded", "csr"])
@pytest.mark.parametrize("name", ["wide2", "deep3", "tiny2"])
def test_function_on_the_double_equals_the_restatement(monkeypatch, name, kind):
    """Training mode: forward, every gradient, the running buffers and num_batches_tracked after one and three forwards; then
    evaluation mode, which must not touch the buffers."""
    fake = R.install(monkeypatch)
    from acm_gnn_amd import SparseFeatures
    from acm_gnn_amd import functional as AF
    g = np.load(GOLDEN)
    n, f_in, hid, f_out, n_lins, dead, lins, bns = _case(g, name)
    mlp = _mlp_from(lins, bns, f_in, hid, f_out)
    lins, bns = _as32(lins), _as32(bns)
    x = torch.from_numpy(g[f"{name}:x"]).float()
    if kind == "csr":
        x = x * (torch.rand(n, f_in, generator=torch.Generator().manual_seed(1)) < 0.5)
    xn = x.numpy().astype(np.float64)
    xin = SparseFeatures.from_torch(x) if kind == "csr" else (torch.nn.functional.pad(x, (0, 3)) if kind == "padded" else x)
    dy = torch.from_numpy(g[f"{name}:dy"]).float()
    mlp.train()
    assert AF.residual_mlp_supported(xin, mlp, True)
    calls = []
    real = fake.acm_bnorm_stats
    monkeypatch.setattr(fake, "acm_bnorm_stats", lambda *a: (calls.append(a[8]), real(*a))[1])
    y = AF.residual_mlp(xin, mlp, relu=True)
    y.backward(dy)
    assert calls == [1] * (n_lins - 1)
    running = [(np.zeros(hid), np.ones(hid)) for _ in bns]
    y_ref, cache, running = R.forward(xn, lins, bns, True, running)
    _, d_lins, d_bns = R.backward(dy.numpy(), lins, bns, cache)
    _close(y.detach().numpy(), y_ref, TOL, "y")
    for i, lin in enumerate(mlp.lins):
        _close(lin.weight.grad.numpy(), d_lins[i][0], 10 * TOL, f"dW{i}")
        _close(lin.bias.grad.numpy(), d_lins[i][1], 10 * TOL, f"db{i}")
    for i, bn in enumerate(list(mlp.bns)[:n_lins - 1]):
        _close(bn.weight.grad.numpy(), d_bns[i][0], 10 * TOL, f"dgamma{i}")
        _close(bn.bias.grad.numpy(), d_bns[i][1], 10 * TOL, f"dbeta{i}")
        _close(bn.running_mean.numpy(), running[i][0], TOL)
        _close(bn.running_var.numpy(), running[i][1], TOL)
        assert bn.num_batches_tracked.dtype == torch.int64 and int(bn.num_batches_tracked) == 1
    with torch.no_grad():
        for _ in range(2):
            AF.residual_mlp(xin, mlp, relu=True)
            _, _, running = R.forward(xn, lins, bns, True, running)
    for i, bn in enumerate(list(mlp.bns)[:n_lins - 1]):
        _close(bn.running_mean.numpy(), running[i][0], TOL)
        _close(bn.running_var.numpy(), running[i][1], TOL)
        assert int(bn.num_batches_tracked) == 3
    # evaluation: the running statistics folded, nothing updated, no gradient -- through layers.MLP.forward too (relu=False)
    mlp.eval()
    before = {k: v.clone() for k, v in mlp.state_dict().items()}
    calls.clear()
    with torch.no_grad():
        assert AF.residual_mlp_supported(xin, mlp, False)
        y_eval = AF.residual_mlp(xin, mlp, relu=True)
        if kind == "dense":
            plain = mlp(xin, input_tensor=True)
    assert calls == [0] * (n_lins - 1) * (2 if kind == "dense" else 1) and not y_eval.requires_grad
    y_ref, _, _ = R.forward(xn, lins, bns, False, [(bn.running_mean.numpy(), bn.running_var.numpy()) for bn in mlp.bns])
    _close(y_eval.numpy(), y_ref, TOL, "eval")
    if kind == "dense":
        _close(plain.numpy(), R.forward(xn, lins, bns, False, [(bn.running_mean.numpy(), bn.running_var.numpy()) for bn in mlp.bns],
                                        relu=False)[0], TOL, "MLP.forward")
    assert all(torch.equal(before[k], v) for k, v in mlp.state_dict().items())
    assert not AF.residual_mlp_supported(xin, mlp, False)    # evaluation mode WITH gradients: the torch modules


def test_outer_dropout_rides_the_last_linear(monkeypatch):
    R.install(monkeypatch)
    from acm_gnn_amd import functional as AF
    g = np.load(GOLDEN)
    n, f_in, hid, f_out, n_lins, dead, lins, bns = _case(g, "wide2")
    mlp = _mlp_from(lins, bns, f_in, hid, f_out).train()
    lins, bns = _as32(lins), _as32(bns)
    x, dy = torch.from_numpy(g["wide2:x"]).float(), torch.from_numpy(g["wide2:dy"]).float()
    st = AF.DropoutState(torch.device("cpu"), seed=7)
    y = AF.residual_mlp(x, mlp, relu=True, drop=(0.4, 2, st, 0))
    y.backward(dy)
    fac = fake_lib.dropout_factors(st.spec(0.4, 2, 0), n, f_out)
    assert 0.2 < float((fac == 0).mean()) < 0.6
    y_ref, cache, _ = R.forward(x.numpy(), lins, bns, True, None, factors=fac)
    _, d_lins, d_bns = R.backward(dy.numpy(), lins, bns, cache, factors=fac)
    _close(y.detach().numpy(), y_ref, TOL)
    _close(mlp.lins[0].weight.grad.numpy(), d_lins[0][0], 10 * TOL)
    _close(mlp.bns[0].weight.grad.numpy(), d_bns[0][0], 10 * TOL)


@pytest.mark.parametrize("tape", [False, True])
def test_first_bias_gradient_is_deferred_until_the_flush(monkeypatch, tape):
    """With a deferral list the row-local kernel of the FIRST layer leaves db_0 to the shared second phase: NaN (the double
    poisons pending outputs) until the flush, the restatement's value after it; every other gradient is complete at once."""
    R.install(monkeypatch)
    from acm_gnn_amd import functional as AF
    g = np.load(GOLDEN)
    n, f_in, hid, f_out, n_lins, dead, lins, bns = _case(g, "deep3")
    mlp = _mlp_from(lins, bns, f_in, hid, f_out).train()
    lins, bns = _as32(lins), _as32(bns)
    x, dy = torch.from_numpy(g["deep3:x"]).float(), torch.from_numpy(g["deep3:dy"]).float()
    y_ref, cache, _ = R.forward(x.numpy(), lins, bns, True, None)
    _, d_lins, d_bns = R.backward(dy.numpy(), lins, bns, cache)
    with AF.deferred_reductions() as d:
        if tape:
            t = AF.Tape()
            with AF.on_tape(t):
                y = AF.residual_mlp(x, mlp, relu=True)
            t.backward(y, dy)
        else:
            y = AF.residual_mlp(x, mlp, relu=True)
            y.backward(dy)
        assert d.pending == 1
        assert torch.isnan(mlp.lins[0].bias.grad).all()
        for i in range(1, n_lins):
            _close(mlp.lins[i].bias.grad.numpy(), d_lins[i][1], 10 * TOL)
        assert d.all_adopted([p.grad for p in mlp.parameters()])
        d.flush()
        assert d.pending == 0
    _close(y.detach().numpy(), y_ref, TOL)
    for i, lin in enumerate(mlp.lins):
        _close(lin.weight.grad.numpy(), d_lins[i][0], 10 * TOL, f"dW{i}")
        _close(lin.bias.grad.numpy(), d_lins[i][1], 10 * TOL, f"db{i}")
    for i in range(n_lins - 1):
        _close(mlp.bns[i].weight.grad.numpy(), d_bns[i][0], 10 * TOL)
        _close(mlp.bns[i].bias.grad.numpy(), d_bns[i][1], 10 * TOL)


def test_outside_the_envelope_the_torch_modules_run(monkeypatch):
    fake = R.install(monkeypatch)
    from acm_gnn_amd import functional as AF, tuning
    from acm_gnn_amd.layers import MLP
    used = []
    real = fake.acm_bnorm_stats
    monkeypatch.setattr(fake, "acm_bnorm_stats", lambda *a: (used.append(1), real(*a))[1])
    x = torch.randn(20, 6)
    ok = MLP(6, 8, 8, 2, dropout=0).train()
    assert AF.residual_mlp_supported(x, ok, True)
    wide = MLP(6, 257, 8, 2, dropout=0).train()
    inner = MLP(6, 8, 8, 2, dropout=0.5).train()
    plain = MLP(6, 8, 8, 2, dropout=0).train()
    plain.bns[0] = torch.nn.BatchNorm1d(8, affine=False)
    cumulative = MLP(6, 8, 8, 2, dropout=0).train()
    cumulative.bns[0].momentum = None
    for mlp in (wide, inner, plain, cumulative):
        assert not AF.residual_mlp_supported(x, mlp, True)
        assert mlp(x, input_tensor=True).grad_fn is not None and not used
    assert AF.residual_mlp_supported(x, inner.eval(), False) is False        # (gradients enabled)
    with torch.no_grad():
        assert AF.residual_mlp_supported(x, inner, False)                    # its dropout is inactive in evaluation mode
    assert not AF.residual_mlp_supported(x.double(), ok, True) and not AF.residual_mlp_supported(x[:, :5], ok, True)
    with tuning.override(mlp_stack=0):
        assert not AF.residual_mlp_supported(x, ok, True)
        ok(x, input_tensor=True)
    assert not used
    ok(x, input_tensor=True)
    assert used


def test_one_row_in_training_raises_what_torch_raises(monkeypatch):
    R.install(monkeypatch)
    from acm_gnn_amd import functional as AF
    from acm_gnn_amd.layers import MLP
    mlp = MLP(6, 8, 8, 2, dropout=0).train()
    x = torch.randn(1, 6)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        AF.residual_mlp(x, mlp)
    with pytest.raises(ValueError, match="Expected more than 1 value per channel when training"):
        torch.nn.Sequential(mlp.lins[0], mlp.bns[0])(x)
    with torch.no_grad():
        assert AF.residual_mlp(x, mlp.eval()).shape == (1, 8)


def test_model_routes_and_csr_features(monkeypatch):
    """GCN("acmgcnpp", init_layers_X=2): dense and CSR features give the same logits and gradients through the new entry (the
    parent refused CSR features here), equal to the torch modules' (tuning switch off) up to fp32 storage; auto_csr converts a
    wide sparse-valued input for the deep stack."""
    fake = R.install(monkeypatch)
    from acm_gnn_amd import GCN, SparseFeatures, tuning
    low, high, un, _ = graph_tensors("geometric")
    n = low.shape[0]
    torch.manual_seed(3)
    model = GCN(12, 16, 3, 2, n, 0.0, "acmgcnpp", 0, init_layers_X=2)
    x = torch.randn(n, 12) * (torch.rand(n, 12) < 0.4)
    used = []
    real = fake.acm_bnorm_bwd
    monkeypatch.setattr(fake, "acm_bnorm_bwd", lambda *a: (used.append(1), real(*a))[1])
    outs, grads = {}, {}
    for kind in ("torch", "dense", "csr"):
        model.zero_grad()
        for bn in model.mlpX.bns:
            bn.reset_running_stats()
        with tuning.override(mlp_stack=0 if kind == "torch" else 1):
            out = model(SparseFeatures.from_torch(x) if kind == "csr" else x, low, high, None)
            out.square().sum().backward()
        assert bool(used) == (kind != "torch")
        outs[kind] = out.detach().numpy()
        grads[kind] = {k: p.grad.numpy().copy() for k, p in model.named_parameters() if p.grad is not None}
        grads[kind]["running_var"] = model.mlpX.bns[0].running_var.numpy().copy()
    for kind in ("dense", "csr"):
        _close(outs[kind], outs["torch"], 5e-5, kind)
        assert set(grads[kind]) == set(grads["torch"])
        for k, v in grads["torch"].items():
            _close(grads[kind][k], v, 5e-4, f"{kind} {k}")
    wide = torch.zeros(n, 300)
    wide[torch.arange(n), torch.arange(n) % 300] = 1.0
    m2 = GCN(300, 16, 3, 2, n, 0.0, "acmgcnpp", 0, init_layers_X=2)
    assert isinstance(m2.auto_csr(wide, None), SparseFeatures)
    with tuning.override(mlp_stack=0):
        assert m2.auto_csr(wide, None) is wide


def test_stock_double_with_cpu_tensors_keeps_the_torch_route(monkeypatch):
    """tests/fake_lib.install does not lift the stack's device seam: CPU tensors are outside the envelope, the stack runs on
    torch modules as before and the stock double is never asked for an acm_bnorm_* symbol."""
    fake = fake_lib.install(monkeypatch)
    from acm_gnn_amd import functional as AF
    from acm_gnn_amd.layers import MLP
    assert not hasattr(fake, "acm_bnorm_stats")
    mlp = MLP(6, 8, 8, 2, dropout=0).train()
    x = torch.randn(20, 6)
    assert not AF.residual_mlp_supported(x, mlp, True)
    out = mlp(x, input_tensor=True)
    assert out.grad_fn is not None and int(mlp.bns[0].num_batches_tracked) == 1


def test_library_exports_the_new_symbols_and_keeps_its_abi_number():
    from acm_gnn_amd import _lib, build
    lib = _lib.load()
    assert lib.acm_version() == 29 == _lib.ABI_VERSION
    for name in ("acm_bnorm_stats_workspace_bytes", "acm_bnorm_stats", "acm_bnorm_fold", "acm_bnorm_param_bwd",
                 "acm_bnorm_bwd_workspace_bytes", "acm_bnorm_bwd"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert "acm_bnorm.hip" in build.SOURCES
    import ctypes as C
    nbytes = C.c_size_t()
    assert lib.acm_bnorm_stats_workspace_bytes(1000, 257, C.byref(nbytes)) == 4          # ACM_EUNSUPPORTED
    assert lib.acm_bnorm_bwd_workspace_bytes(1000, 0, C.byref(nbytes)) == 4
    assert lib.acm_bnorm_stats_workspace_bytes(70001, 256, C.byref(nbytes)) == 0 and nbytes.value % 16 == 0
    assert lib.acm_bnorm_stats(1, 8, None, 8, None, None, 1e-5, 0.1, 1, None, None, None, None, None, 0, None) == 1   # ACM_EINVAL


@pytest.mark.parametrize("lifted", [True, False])
def test_a_redone_training_step_updates_the_buffers_once(monkeypatch, lifted):
    """TrainStep redoes its first eager pass on autograd when the Tape breaks (ACM-GCN++ adds its residual with a torch
    operation): the aborted forward's BatchNorm update must not count -- on the kernels and on the torch modules alike."""
    (R.install if lifted else fake_lib.install)(monkeypatch)
    from acm_gnn_amd import GCN, FusedAdamW, train as T
    low, high, un, _ = graph_tensors("geometric")
    n = low.shape[0]
    torch.manual_seed(0)
    model = GCN(12, 16, 3, 2, n, 0.5, "acmgcnpp", 0, init_layers_X=2)
    x, y = torch.randn(n, 12), torch.randint(0, 3, (n,))
    step = T.TrainStep(model, FusedAdamW(model.parameters(), lr=0.05), x, low, y, T.row_weights(torch.arange(0, n, 2), n), high, None,
                       use_graph=False, fused_dropout=True, small_step=False)
    for k in range(3):
        step()
        assert int(model.mlpX.bns[0].num_batches_tracked) == k + 1
    assert step._tape is False
