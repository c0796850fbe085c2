"""Deep mlpX stacks (init_layers_X > 1) on the acm_bnorm_* kernels, on the GPU: the statistics kernel alone, functional.residual_mlp
end to end, GCN("acmgcnpp", init_layers_X=2), the captured TrainStep and fit(keep_best=True).

The yardstick is float64 throughout: tests/mlp_stack_ref.py (pinned to the reference's module by tests/golden/mlp_stack_cases.npz),
never the code under test.  BatchNorm's r = 1 / sqrt(var + eps) amplifies rounding on narrow columns, so no number is fixed in
advance: every case also runs torch's own fp32 modules on the same device tensors, and the new route's error (in units of
max(1, |reference|)) may be at most FACTOR = 4 times torch's -- the summation orders differ: torch's GEMMs and its BatchNorm
reduce in other trees than acm_gemm and the (count, mean, M2) merge, and each of the up to three chained fp32 products re-rounds
-- but the bound never falls below the project's floors, 3e-5 forward and 1e-4 for gradients (tests/test_gpu_oracle.py:463-471).
Every test prints the two errors it compares.

A ReLU unit whose fp32 pre-activation lands on the other side of zero than the float64 one flips a whole gradient term; at
70001 x 256 (18 M units per layer) one or two do, in either route, which is why the gradient errors of that shape are 1e-3 where
the others are 1e-6 -- torch's modules show the same (below), and the factor rule absorbs it.

Measured on an MI355X, worst error over the quantities of a case, new route / torch's fp32 modules, in units of max(1, |ref|):
statistics kernel (mean, variance, r, a, c, running buffers): (2, 1, 1) 5.6e-8 / 2.5e-8; (63, 24, 25) 2.3e-5 / 1.5e-5;
(1000, 33, 40) 3.6e-5 / 4.0e-5; (70001, 256, 256) 2.6e-6 / 6.4e-6 (the largest are r on the 1000 + 0.1 noise column).  Relative
variance error of that column: 4.6e-5 / 3.1e-5, 7.3e-5 / 8.0e-5, 5.1e-6 / 1.2e-5.  Function, forward + evaluation + running
buffers: 2.0e-7 .. 5.0e-7 / 2.9e-7 .. 6.3e-7 over the eight cases; gradients: (400, 7, 64, 2) 7.5e-7 / 5.8e-7; (1000, 40, 200, 3)
8.2e-7 / 1.0e-6; (400, 300, 64, 2) CSR 7.4e-7 / 4.7e-7; (70001, 16, 256, 2) 2.2e-3 / 9.4e-3 without and 2.8e-6 / 1.0e-2 with the
outer dropout.  GCN end to end (n = 400): logits 2.5e-7 / 2.2e-7 (dense, p = 0.3) and 1.4e-7 / 2.0e-7 (CSR); the worst parameter
gradient 6.4e-7 / 3.7e-7 and 2.8e-7 / 5.5e-8 (both in mlpX.lins).
No case needed more than its floor except the statistics of the narrow 1000 + 0.1 noise column (ratio new / torch at most
1.5) and the gradients of the 70001-row shape (ratio below 1); below the floors the ratio reaches 3.0 (dgamma, CSR case), which
is rounding noise of either route.  FACTOR = 4 leaves the usual factor of two to a differently ordered fp32 sum, twice over
(the statistics and the product that consumes them)."""
import copy
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import mlp_stack_ref as R
from oracle import acm_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FACTOR, FLOOR_FWD, FLOOR_GRAD = 4.0, 3e-5, 1e-4
EPS = 1e-5


def _err(got, want):
    want = np.asarray(want, np.float64)
    got = got.detach().double().cpu().numpy() if isinstance(got, torch.Tensor) else np.asarray(got, np.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    return float(np.abs(got - want).max(initial=0.0)) / max(1.0, float(np.abs(want).max(initial=0.0)))


def _check(what, new, ref_err, floor):
    print(f"{what}: new route {new:.3e}, torch fp32 {ref_err:.3e}, bound {max(FACTOR * ref_err, floor):.3e}")
    assert new <= max(FACTOR * ref_err, floor), what


# ---------------------------------------------------------------------------------------------- the statistics kernel alone
def _stats_input(n, f, ld, seed):
    rng = np.random.default_rng(seed)
    h = np.maximum(rng.standard_normal((n, ld)) + 0.3, 0.0).astype(np.float32)
    dead = big = None
    if f >= 3:
        dead, big = 0, f - 1
        h[:, dead] = 0.0                                                      # a ReLU unit that never fires
        h[:, big] = (1000.0 + 0.1 * rng.standard_normal(n)).astype(np.float32)   # mean >> spread: a sum of squares loses every digit
    return h, dead, big


def _launch_stats(h, f, gamma, beta, rm, rv, nbt, momentum=0.1):
    from acm_gnn_amd.functional._launch import _vp, _workspace_sized, launch
    n = h.shape[0]
    stats = torch.empty(4, f, device=DEV)
    ws, nbytes = _workspace_sized(h.device, "acm_bnorm_stats_workspace_bytes", n, f)
    launch("acm_bnorm_stats", None, h.device, n, f, _vp(h), h.stride(0), _vp(gamma), _vp(beta), EPS, momentum, 1, _vp(rm), _vp(rv),
           _vp(nbt), _vp(stats), _vp(ws), nbytes)
    return stats


@pytest.mark.parametrize("n,f,ld", [(2, 1, 1), (63, 24, 25), (1000, 33, 40), (70001, 256, 256)])
def test_column_statistics_against_float64(n, f, ld):
    h_np, dead, big = _stats_input(n, f, ld, seed=n)
    rng = np.random.default_rng(1)
    gamma_np, beta_np = rng.uniform(0.5, 1.5, f).astype(np.float32), rng.uniform(-0.5, 0.5, f).astype(np.float32)
    h = torch.from_numpy(h_np).to(DEV)
    gamma, beta = torch.from_numpy(gamma_np).to(DEV), torch.from_numpy(beta_np).to(DEV)
    h64 = h_np[:, :f].astype(np.float64)
    mu, var = h64.mean(0), h64.var(0)
    r = 1.0 / np.sqrt(var + EPS)
    a = gamma_np.astype(np.float64) * r
    c = beta_np.astype(np.float64) - mu * a
    rm, rv, nbt = torch.zeros(f, device=DEV), torch.ones(f, device=DEV), torch.zeros((), dtype=torch.int64, device=DEV)
    first = _launch_stats(h, f, gamma, beta, rm, rv, nbt).clone()
    # torch's own fp32 statistics of the same device tensor
    bn = torch.nn.BatchNorm1d(f, eps=EPS).to(DEV).train()
    with torch.no_grad():
        bn(h[:, :f])
        t_var, t_mu = torch.var_mean(h[:, :f], 0, unbiased=False)
    _check(f"{n}x{f} mean", _err(first[0], mu), _err(t_mu, mu), FLOOR_FWD)
    got_var = 1.0 / first[1].double().cpu().numpy() ** 2 - EPS
    _check(f"{n}x{f} variance", _err(got_var, var), _err(t_var, var), FLOOR_FWD)
    t_mu64, t_r = t_mu.double().cpu().numpy(), 1.0 / np.sqrt(t_var.double().cpu().numpy() + EPS)
    t_a = gamma_np.astype(np.float64) * t_r
    for k, want, t_got in ((1, r, t_r), (2, a, t_a), (3, c, beta_np.astype(np.float64) - t_mu64 * t_a)):
        # per column relative to its own size (r reaches 316 on a dead column)
        rel = np.abs(first[k].double().cpu().numpy() - want) / np.maximum(1.0, np.abs(want))
        t_rel = np.abs(t_got - want) / np.maximum(1.0, np.abs(want))
        _check(f"{n}x{f} stats[{k}]", float(rel.max()), float(t_rel.max()), FLOOR_FWD)
    if dead is not None:
        got = first.cpu().numpy()
        assert got[0, dead] == 0.0 and abs(got[1, dead] * np.sqrt(EPS) - 1.0) < 1e-6 and got[3, dead] == beta_np[dead]     # v = 0
        # ... so that xhat = (H - mu) r = 0 and the normalised output a * H + c is beta on that column
        rel_new = abs(got_var[big] - var[big]) / var[big]
        rel_torch = abs(float(t_var[big]) - var[big]) / var[big]
        print(f"{n}x{f} column 1000 + 0.1 noise: relative variance error {rel_new:.3e} (torch {rel_torch:.3e})")
        # Merging a group of 8 rows whose mean lies D ~ sigma / sqrt(8) = 0.035 from the running mean adds D^2 to M2; both means
        # sit near 1000 and carry up to two ulp(1000) = 1.2e-4 of rounding, so D^2 is off by 2 * 1.2e-4 / D = 7e-3 relative, and
        # the between-group terms are 1/8 of M2: 8.6e-4 if every error had the same sign (the within-group differences x - mean
        # of nearby fp32 values are exact).  A sum of squares of the raw values is off by more than the variance itself.
        assert rel_new <= max(FACTOR * rel_torch, 1e-3)
    # two more calls: the same bits every time, the buffers follow the float64 recurrence, the counter counts
    for _ in range(2):
        again = _launch_stats(h, f, gamma, beta, rm, rv, nbt)
        assert torch.equal(again.view(torch.int32), first.view(torch.int32))
    want_rm, want_rv = np.zeros(f), np.ones(f)
    for _ in range(3):
        want_rm = 0.9 * want_rm + 0.1 * mu
        want_rv = 0.9 * want_rv + 0.1 * var * n / (n - 1)
    _check(f"{n}x{f} running_mean", _err(rm, want_rm), _err(bn.running_mean, 0.1 * mu), FLOOR_FWD)
    _check(f"{n}x{f} running_var", _err(rv, want_rv), _err(bn.running_var, 0.9 + 0.1 * var * n / (n - 1)), FLOOR_FWD)
    assert nbt.dtype == torch.int64 and int(nbt) == 3


# ---------------------------------------------------------------------------------------------- the Function end to end
def _philox_factors(state, p, tag, n, c):
    """The keep factors of the counter-based mask, regenerated on the host as tests/test_gpu_oracle.py::_philox_mask does."""
    import fake_lib

    class D:
        pass
    dd = D()
    dd.p, dd.tag, dd.seed, dd.row_offset = np.float32(p), tag, state.seed, 0
    host = np.array([int(state.step.item())], np.int64)
    dd.step = host.ctypes.data
    return fake_lib.dropout_factors(dd, n, c)


@functools.lru_cache(maxsize=None)
def _stack_case(n, f_in, hidden, n_lins, sparse):
    """Inputs and parameters of one shape (numpy, fp32 values): computed once, shared, never modified."""
    rng = np.random.default_rng(n + f_in)
    x = rng.standard_normal((n, f_in)).astype(np.float32)
    if sparse:
        x = x * (rng.random((n, f_in)) < 0.05)
    dims = [f_in] + [hidden] * n_lins
    lins = [((rng.uniform(-1, 1, (dims[i + 1], dims[i])) / np.sqrt(dims[i])).astype(np.float32),
             rng.uniform(-0.3, 0.3, dims[i + 1]).astype(np.float32)) for i in range(n_lins)]
    bns = [(rng.uniform(0.5, 1.5, hidden).astype(np.float32), rng.uniform(-0.5, 0.5, hidden).astype(np.float32)) for _ in range(n_lins - 1)]
    dy = rng.standard_normal((n, hidden)).astype(np.float32)
    for t in (x, dy) + tuple(t for p in lins + bns for t in p):
        t.setflags(write=False)
    return x, lins, bns, dy


def _device_mlp(f_in, hidden, lins, bns):
    from acm_gnn_amd.layers import MLP
    mlp = MLP(f_in, hidden, hidden, len(lins), dropout=0)
    with torch.no_grad():
        for lin, (w, b) in zip(mlp.lins, lins):
            lin.weight.copy_(torch.tensor(w))
            lin.bias.copy_(torch.tensor(b))
        for bn, (g, b) in zip(mlp.bns, bns):
            bn.weight.copy_(torch.tensor(g))
            bn.bias.copy_(torch.tensor(b))
    return mlp.to(DEV).train()


@pytest.mark.parametrize("p_drop", [0.0, 0.3])
@pytest.mark.parametrize("n,f_in,hidden,n_lins,sparse", [(400, 7, 64, 2, False), (1000, 40, 200, 3, False), (70001, 16, 256, 2, False),
                                                         (400, 300, 64, 2, True)])
def test_stack_forward_and_gradients(n, f_in, hidden, n_lins, sparse, p_drop):
    from acm_gnn_amd import SparseFeatures, functional as AF, tuning
    x_np, lins, bns, dy_np = _stack_case(n, f_in, hidden, n_lins, sparse)
    x, dy = torch.tensor(x_np, device=DEV), torch.tensor(dy_np, device=DEV)
    xin = SparseFeatures.from_torch(x) if sparse else x
    st = AF.DropoutState(torch.device(DEV), seed=77)
    st.step.fill_(3)
    fac = _philox_factors(st, p_drop, 2, n, hidden) if p_drop else None
    y_ref, cache, running = R.forward(x_np, lins, bns, True, [(np.zeros(hidden), np.ones(hidden))] * (n_lins - 1), factors=fac)
    _, d_lins, d_bns = R.backward(dy_np, lins, bns, cache, factors=fac)

    new = _device_mlp(f_in, hidden, lins, bns)
    assert AF.residual_mlp_supported(xin, new, True)
    y = AF.residual_mlp(xin, new, relu=True, drop=(p_drop, 2, st, 0) if p_drop else None)
    y.backward(dy)
    old = _device_mlp(f_in, hidden, lins, bns)                               # torch's own fp32 modules, same device tensors
    with tuning.override(mlp_stack=0):
        t = torch.relu(old(x, input_tensor=True))
    if fac is not None:
        t = t * torch.from_numpy(fac).float().to(DEV)
    t.backward(dy)
    tag = f"{n}x{f_in}x{hidden} L{n_lins}{' csr' if sparse else ''} p={p_drop}"
    _check(f"{tag} y", _err(y, y_ref), _err(t, y_ref), FLOOR_FWD)
    for i in range(n_lins):
        _check(f"{tag} dW{i}", _err(new.lins[i].weight.grad, d_lins[i][0]), _err(old.lins[i].weight.grad, d_lins[i][0]), FLOOR_GRAD)
        _check(f"{tag} db{i}", _err(new.lins[i].bias.grad, d_lins[i][1]), _err(old.lins[i].bias.grad, d_lins[i][1]), FLOOR_GRAD)
    for i in range(n_lins - 1):
        _check(f"{tag} dgamma{i}", _err(new.bns[i].weight.grad, d_bns[i][0]), _err(old.bns[i].weight.grad, d_bns[i][0]), FLOOR_GRAD)
        _check(f"{tag} dbeta{i}", _err(new.bns[i].bias.grad, d_bns[i][1]), _err(old.bns[i].bias.grad, d_bns[i][1]), FLOOR_GRAD)
        _check(f"{tag} running_mean{i}", _err(new.bns[i].running_mean, running[i][0]), _err(old.bns[i].running_mean, running[i][0]), FLOOR_FWD)
        _check(f"{tag} running_var{i}", _err(new.bns[i].running_var, running[i][1]), _err(old.bns[i].running_var, running[i][1]), FLOOR_FWD)
        assert int(new.bns[i].num_batches_tracked) == 1
    # evaluation mode: the running statistics folded, no gradient, nothing updated
    new.eval()
    with torch.no_grad():
        y_eval = AF.residual_mlp(xin, new, relu=True)
        t_eval = torch.relu(old.eval()(x, input_tensor=True))
    ref_eval, _, _ = R.forward(x_np, lins, bns, False, running)
    _check(f"{tag} eval", _err(y_eval, ref_eval), _err(t_eval, ref_eval), FLOOR_FWD)
    assert int(new.bns[0].num_batches_tracked) == 1


# ---------------------------------------------------------------------------------------------- the model
def _graph(n, seed, density=0.05):
    rng = np.random.default_rng(seed)
    a = sp.random(n, n, density=density, random_state=rng, format="csr")
    a = ((a + a.T) > 0).astype(np.float64).tolil()
    a[0, 1:] = 1.0
    a[1:, 0] = 1.0
    a[n - 1, :] = 0
    a[:, n - 1] = 0
    return sp.csr_matrix(a)


def _oracle_logits(params, x, low, high, p_drop, masks):
    """ACM-GCN++ with a deep mlpX in float64: the oracle's layer functions around the stack's restatement (models.py:150-165)."""
    kw = dict(model_type="acmgcnpp", variant=False, structure_info=0, attn_layernorm=True)
    p0 = {k[len("gcns.0."):]: v for k, v in params.items() if k.startswith("gcns.0.")}
    p1 = {k[len("gcns.1."):]: v for k, v in params.items() if k.startswith("gcns.1.")}
    n_lins = sum(1 for k in params if k.startswith("mlpX.lins.") and k.endswith(".weight"))
    lins = [(params[f"mlpX.lins.{i}.weight"], params[f"mlpX.lins.{i}.bias"]) for i in range(n_lins)]
    bns = [(params[f"mlpX.bns.{i}.weight"], params[f"mlpX.bns.{i}.bias"]) for i in range(n_lins - 1)]
    x = O._drop(x, p_drop, True, masks.get("x"))
    xx = O._drop(torch.relu(R.forward_torch(x, lins, bns)), p_drop, True, masks.get("xX"))
    fea = O._drop(torch.relu(O.layer_forward(p0, x, low, high, None, **kw)), p_drop, True, masks.get("hidden"))
    return O.layer_forward(p1, fea + xx, low, high, None, **kw)


@pytest.mark.parametrize("f_in,p_drop,sparse_x", [(7, 0.3, False), (300, 0.0, True)])
def test_acmgcnpp_with_a_deep_stack_matches_the_oracle(f_in, p_drop, sparse_x):
    """Training-mode logits and every parameter gradient against the float64 composition; the kernel labels show the acm_bnorm_*
    kernels ran and no bias_act_bwd did; CSR features no longer raise (this and the labels fail without the feature)."""
    from acm_gnn_amd import GCN, SparseFeatures, functional as AF, tuning
    from acm_gnn_amd.graph import clear_cache
    clear_cache()
    n = 400
    low, high, _ = O.filters_linkx(_graph(n, 9))
    g = torch.Generator().manual_seed(2)
    x = torch.randn(n, f_in, generator=g)
    if sparse_x:
        x = x * (torch.rand(n, f_in, generator=g) < 0.05)
    y = torch.randint(0, 3, (n,), generator=g)
    idx = torch.arange(0, n, 2)
    torch.manual_seed(5)
    model = GCN(f_in, 64, 3, 2, n, p_drop, "acmgcnpp", 0, variant=False, attn_layernorm=True, init_layers_X=2)
    with torch.no_grad():
        model.mlpX.bns[0].weight.uniform_(0.5, 1.5)
        model.mlpX.bns[0].bias.uniform_(-0.5, 0.5)
    params = {k: v.detach().cpu().double().clone().requires_grad_(True) for k, v in model.named_parameters() if k not in ("fea_param", "xX_param")}
    model = model.to(DEV).train()
    masks = {}
    if p_drop:
        model.fused_dropout, model.dropout_state = True, AF.DropoutState(DEV, seed=99)
        model.dropout_state.step.fill_(7)
        st = model.dropout_state
        masks = {k: torch.from_numpy(_philox_factors(st, p_drop, tag, n, w) > 0).double()
                 for k, tag, w in (("x", 0, f_in), ("hidden", 1, 64), ("xX", 2, 64))}
    ref = _oracle_logits(params, x.double(), low.double(), high.double(), p_drop, masks)
    O.nll_loss_on(ref, y, idx).backward()
    lowd, highd = low.to(DEV), high.to(DEV)

    def run(xin):
        model.zero_grad()
        for bn in model.mlpX.bns:
            bn.reset_running_stats()
        out = model(xin, lowd, highd, None)
        torch.nn.functional.nll_loss(torch.log_softmax(out, 1)[idx.to(DEV)], y.to(DEV)[idx.to(DEV)]).backward()
        return out.detach().clone(), {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}

    timer = AF.KernelTimer()
    AF.set_kernel_timer(timer)
    try:
        out, grads = run(SparseFeatures.from_torch(x.to(DEV)) if sparse_x else x.to(DEV))
    finally:
        AF.set_kernel_timer(None)
    used = set(k.split("/")[0] for k in timer.events)
    assert {"bnorm_stats", "bnorm_fold", "bnorm_param_bwd", "bnorm_bwd"} <= used and "bias_act_bwd" not in used, used
    assert ("bias_act" in used) == sparse_x and ("linear_fwd" in used), used
    assert int(model.mlpX.bns[0].num_batches_tracked) == 1
    with tuning.override(mlp_stack=0):                                      # torch's modules in the same model (dense features)
        t_out, t_grads = run(x.to(DEV))
    tag = f"acmgcnpp f_in={f_in} p={p_drop}"
    _check(f"{tag} logits", _err(out, ref.detach().numpy()), _err(t_out, ref.detach().numpy()), FLOOR_FWD)
    for k, v in params.items():
        if v.grad is None:
            assert k not in grads, k
            continue
        _check(f"{tag} {k}", _err(grads[k], v.grad.numpy()), _err(t_grads[k], v.grad.numpy()), FLOOR_GRAD)


# ---------------------------------------------------------------------------------------------- captured step, fit
@functools.lru_cache(maxsize=None)
def _problem():
    from acm_gnn_amd import synthetic as S
    g = S.generate_graph("random", 5, 80, degree_intra=2, edge_homo=0.3, seed=3, device=DEV)
    x = S.random_features(g.n, 32, seed=3, device=DEV)
    return g.operators(), x, g.labels, S.disassortative_splits(g.labels, 5, seed=3), g.n


def _fresh(seed=0, lr=0.05):
    import acm_gnn_amd
    from acm_gnn_amd import FusedAdam, functional as AF
    ops, x, y, sets, n = _problem()
    torch.manual_seed(100 + seed)
    model = acm_gnn_amd.GCN(32, 64, 5, 2, n, 0.5, "acmgcnpp", 0, init_layers_X=2).to(DEV)
    model.fused_dropout = True
    model.dropout_state = AF.DropoutState(torch.device(DEV), seed=4242 + seed)
    return model, FusedAdam(model.parameters(), lr=lr, weight_decay=5e-4)


def test_captured_train_step_equals_eager_steps_bit_for_bit():
    from acm_gnn_amd import functional as AF, train as T
    ops, x, y, sets, n = _problem()
    assert n == 400
    w = T.row_weights(sets[0], n, device=y.device)
    states = {}
    for use_graph in (False, True):
        model, opt = _fresh()
        timer = AF.KernelTimer()
        AF.set_kernel_timer(timer if not use_graph else None)
        try:
            step = T.TrainStep(model, opt, x, ops, y, w, use_graph=use_graph, small_step=False)
            for _ in range(5):
                step()
        finally:
            AF.set_kernel_timer(None)
        torch.cuda.synchronize()
        if not use_graph:
            assert "bnorm_stats" in set(k.split("/")[0] for k in timer.events)
        states[use_graph] = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert int(states[True]["mlpX.bns.0.num_batches_tracked"]) == 5          # (the capture warm-up left no trace)
    for k, v in states[False].items():
        assert torch.equal(v, states[True][k]), k
    assert not torch.equal(states[True]["mlpX.bns.0.running_mean"], torch.zeros_like(states[True]["mlpX.bns.0.running_mean"]))


def test_keep_best_returns_the_selected_epochs_statistics_too():
    """fit(keep_best=True, sync_every=4): the returned model's evaluation logits equal those of a model reloaded from a host
    copy of the state after the selected epoch (the same run cut short there: the loop is reproducible bit for bit)."""
    from select_ref import select_ref
    from acm_gnn_amd import train as T
    ops, x, y, sets, n = _problem()
    epochs = 40
    model, opt = _fresh()
    sel, hist = T.fit(model, opt, x, ops, y, *sets, epochs, rule="min_val_loss", early_stopping=0, use_graph=True, sync_every=4,
                      keep_best=True)
    best = select_ref(hist, "min_val_loss", 0)[2]
    print(f"selected epoch {best} of {len(hist)}")
    assert len(hist) == epochs and 0 <= best < epochs - 1, "the selected epoch must not be the last one for this test to mean anything"
    short, opt2 = _fresh()
    T.fit(short, opt2, x, ops, y, *sets, best + 1, rule="min_val_loss", early_stopping=0, use_graph=True)
    host = {k: v.detach().cpu().clone() for k, v in short.state_dict().items()}
    reloaded, _ = _fresh(seed=1)
    reloaded.load_state_dict(copy.deepcopy(host))
    with torch.no_grad():
        got = model.eval()(x, ops)
        want = reloaded.to(DEV).eval()(x, ops)
    assert torch.equal(got, want)
    for k, v in model.state_dict().items():
        if "num_batches_tracked" not in k:                                   # (an int64 counter: not part of the snapshot)
            assert torch.equal(v.cpu(), host[k]), k
