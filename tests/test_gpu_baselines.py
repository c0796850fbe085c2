"""The synthetic study's baselines on the MI355X: acm_gcn_fwd / acm_gcn_bwd against float64, the five models against the values
recorded from the study's own code, the execution forms of ``baselines.GCN`` and ``synthetic.disassortative_splits``.

Tolerances are the project's fp32 parity thresholds: forward 2e-5 * max(1, max |ref|), gradients 1e-4 * max(1, max |ref|)."""
import os

import numpy as np
import pytest
import torch

import baselines_ref as R
import fake_lib
import launch_forms as LF
from conftest import GOLDEN, load_npz

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FWD, GRAD = 2e-5, 1e-4


def _close(got, ref, tol, what=""):
    ref = np.asarray(ref.detach().cpu() if isinstance(ref, torch.Tensor) else ref, np.float64)
    got = np.asarray(got.detach().cpu() if isinstance(got, torch.Tensor) else got, np.float64)
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    bound = tol * max(1.0, float(np.abs(ref).max()) if ref.size else 0.0)
    err = float(np.abs(got - ref).max()) if ref.size else 0.0
    assert err <= bound, (what, err, bound)


# ---- operators of the kernel tests: computed once, never modified --------------------------------------------------------------
def _make_operator(n, explicit, chunk=256, density=None):
    """(CsrGraph, dense float64 matrix of what the handle multiplies by, row_scale or None).  n >= 300: node 0 is adjacent to
    every node (a row longer than ``chunk``: the split-row paths -- the fix-up launch at n = 1025, mean degree 8 and eight lanes
    per row; the in-LDS combine at n = 300, mean degree 20 and sixteen lanes; several windows of pieces at n = 2100 under
    chunk = 128); the pattern-only operators have an EMPTY row."""
    from acm_gnn_amd.graph import CsrGraph
    rng = np.random.RandomState(n + int(explicit))
    dense = (rng.rand(n, n) < (density or min(1.0, (6.0 if n in (63, 1025) else 20.0) / n))).astype(np.float64)
    if n >= 300:
        dense[0, :] = 1
        dense[:, 0] = 1
    if n > 1 and not explicit:
        dense[n // 2, :] = 0                                  # the empty row
    if n == 1:
        dense[0, 0] = 1
    if explicit:
        dense = dense * rng.uniform(0.2, 1.0, (n, n)).astype(np.float32).astype(np.float64)
    indptr = np.zeros(n + 1, np.int32)
    indptr[1:] = np.cumsum((dense != 0).sum(1))
    rows, cols = np.nonzero(dense)
    vals = torch.from_numpy(dense[rows, cols].astype(np.float32)).to(DEV) if explicit else None
    graph = CsrGraph.from_csr(torch.from_numpy(indptr).to(DEV), torch.from_numpy(cols.astype(np.int32)).to(DEV), vals, n, chunk=chunk)
    scale = None
    if not explicit:
        scale = torch.from_numpy((1.0 / np.maximum(dense.sum(1), 1.0)).astype(np.float32)).to(DEV)
        dense = scale.double().cpu().numpy()[:, None] * dense
    return graph, dense, scale


_OPERATORS = {}


def _operator(n, explicit, tune):
    tune(chunk=256)
    key = (n, explicit)
    if key not in _OPERATORS:
        _OPERATORS[key] = _make_operator(n, explicit)
    return _OPERATORS[key]


def _host_factors(state, p, tag, n, c):
    """The expected keep factors of an acm_dropout_t, regenerated on the host from the counter (fake_lib.dropout_factors)."""
    class D:
        pass
    dd = D()
    dd.p, dd.tag, dd.seed, dd.row_offset = np.float32(p), tag, state.seed, 0
    host = np.array([int(state.step.item())], np.int64)
    dd.step = host.ctypes.data
    return fake_lib.dropout_factors(dd, n, c)


WIDTHS = (1, 5, 8, 9, 32, 64, 130)


@pytest.mark.parametrize("explicit", [True, False], ids=["explicit", "implicit"])
@pytest.mark.parametrize("n", [1, 63, 300, 1025])
def test_gcn_fwd_against_float64(n, explicit, tune):
    """Y = drop(relu?(A Z)) and the ridden projection Z_next = Y W_next: every width class of the gather family, ReLU off / on,
    p in {0, 0.5} with the mask regenerated from the counter, f_next in {none, 2, 5, 8}; outputs written with a row pitch above
    their width leave the padding alone; two runs agree to the bit (the split row of the 1025-node hub included)."""
    from acm_gnn_amd import functional as AF
    graph, dense, scale = _operator(n, explicit, tune)
    if n == 1025:
        assert graph.n_long_rows >= 1                         # the epilogue runs on a combined sum
    state = AF.DropoutState(torch.device(DEV), seed=1234 + n)
    state.step.fill_(7)
    rng = np.random.RandomState(n)
    for width in WIDTHS:
        z = rng.standard_normal((n, width)).astype(np.float32)
        az = dense @ z.astype(np.float64)
        zd = torch.from_numpy(z).to(DEV)
        factors = _host_factors(state, 0.5, 3, n, width)
        for relu, p in ((False, 0.0), (True, 0.0), (True, 0.5), (False, 0.5)):
            ref = np.maximum(az, 0) if relu else az
            if p:
                ref = ref * factors
            spec = state.spec(p, 3) if p else None
            for f_next in (0, 2, 5, 8):
                w_next = rng.standard_normal((width, f_next)).astype(np.float32) if f_next else None
                buf = torch.full((n, width + 3), 7.0, device=DEV)
                nbuf = torch.full((n, f_next + 2), 7.0, device=DEV) if f_next else None
                wn = torch.from_numpy(w_next).to(DEV) if f_next else None
                y, zn = AF.gcn_fwd(graph, zd, row_scale=scale, relu=relu, drop=spec, w_next=wn, out=buf[:, :width],
                                   out_next=nbuf[:, :f_next] if f_next else None)
                what = (n, explicit, width, relu, p, f_next)
                _close(y, ref, FWD, what)
                assert bool((buf[:, width:] == 7.0).all()), what
                if f_next:
                    _close(zn, ref @ w_next.astype(np.float64), FWD, what)
                    assert bool((nbuf[:, f_next:] == 7.0).all()), what
                if f_next in (0, 5):
                    y2, zn2 = AF.gcn_fwd(graph, zd, row_scale=scale, relu=relu, drop=spec, w_next=wn)
                    assert torch.equal(y2, y) and (zn is None or torch.equal(zn2, zn)), what
                    ya, zna = AF.gcn_fwd(graph, zd, row_scale=scale, relu=relu, drop=spec, w_next=wn, fused=False)
                    _close(ya, ref, FWD, what)
                    if f_next:
                        _close(zna, ref @ w_next.astype(np.float64), FWD, what)


@pytest.mark.parametrize("explicit", [True, False], ids=["explicit", "pattern"])
@pytest.mark.parametrize("n", [1, 63, 300, 1025])
def test_gcn_bwd_against_float64(n, explicit, tune):
    """dZ = G dY, g = (dZ W2^T) * keep_scale [H > 0] with the masks read off an H that holds exact zeros, dW2 = H^T dZ: against
    float64, dW2 bit-identical between two fused runs and within the gradient tolerance of the composed arm."""
    from acm_gnn_amd import functional as AF
    graph, dense, scale = _operator(n, explicit, tune)
    if scale is not None:
        dense = dense / np.maximum(scale.double().cpu().numpy()[:, None], 1e-30)      # the pattern itself: the handle's own product
        dense = np.rint(dense)
    rng = np.random.RandomState(100 + n)
    for width in (1, 2, 5, 8):
        for hidden in (32, 64):
            dy = rng.standard_normal((n, width)).astype(np.float32)
            h = (np.maximum(rng.standard_normal((n, hidden)), 0) * (rng.rand(n, hidden) < 0.5) * 2.0).astype(np.float32)
            assert (h == 0).any()
            w2 = rng.standard_normal((hidden, width)).astype(np.float32)
            dz_ref = dense @ dy.astype(np.float64)
            dyd, hd, w2d = (torch.from_numpy(t).to(DEV) for t in (dy, h, w2))
            for relu, ks in ((True, 2.0), (True, 1.0), (False, 2.0)):
                mask = (h > 0) if relu else (h != 0)
                g_ref = (dz_ref @ w2.astype(np.float64).T) * mask * ks
                dw_ref = h.astype(np.float64).T @ dz_ref
                what = (n, explicit, width, hidden, relu, ks)
                g, dw, dz = AF.gcn_bwd(graph, dyd, hd, w2d, keep_scale=ks, relu=relu, want_dz=True)
                _close(dz, dz_ref, GRAD, what)
                _close(g, g_ref, GRAD, what)
                _close(dw, dw_ref, GRAD, what)
                g2, dw2, _ = AF.gcn_bwd(graph, dyd, hd, w2d, keep_scale=ks, relu=relu)
                assert torch.equal(dw2, dw) and torch.equal(g2, g), what
                ga, dwa, _ = AF.gcn_bwd(graph, dyd, hd, w2d, keep_scale=ks, relu=relu, fused=False)
                _close(dw, dwa, GRAD, what)
                _close(g, ga, GRAD, what)


def test_gcn_kernels_on_a_row_of_several_windows(tune):
    """A hub row of 2 100 entries under chunk = 128 is seventeen pieces: more than one window of the sixteen-lanes-per-row narrow
    gather, whose window sums meet in a launch of their own -- both epilogues once more on the combined sum."""
    from acm_gnn_amd import functional as AF
    tune(chunk=128)
    graph, dense, _ = _make_operator(2100, True, chunk=128)
    assert graph.n_long_rows >= 1 and graph.max_degree == 2100
    rng = np.random.RandomState(5)
    for width in (5, 32):
        z = rng.standard_normal((2100, width)).astype(np.float32)
        w_next = rng.standard_normal((width, 3)).astype(np.float32)
        y, zn = AF.gcn_fwd(graph, torch.from_numpy(z).to(DEV), relu=True, w_next=torch.from_numpy(w_next).to(DEV))
        ref = np.maximum(dense @ z.astype(np.float64), 0)
        _close(y, ref, FWD, width)
        _close(zn, ref @ w_next.astype(np.float64), FWD, width)
    dy, w2 = rng.standard_normal((2100, 5)).astype(np.float32), rng.standard_normal((32, 5)).astype(np.float32)
    h = np.maximum(rng.standard_normal((2100, 32)), 0).astype(np.float32)
    g, dw, dz = AF.gcn_bwd(graph, *(torch.from_numpy(t).to(DEV) for t in (dy, h, w2)), keep_scale=2.0, want_dz=True)
    dz_ref = dense @ dy.astype(np.float64)
    _close(dz, dz_ref, GRAD)
    _close(g, (dz_ref @ w2.astype(np.float64).T) * (h > 0) * 2.0, GRAD)
    _close(dw, h.astype(np.float64).T @ dz_ref, GRAD)


def test_gcn_fwd_wider_than_one_column_block(tune):
    """260 columns with a post-op: two column blocks, neither of 8 columns or fewer (the post-op kernels exist for wider blocks
    only), the mask a function of the GLOBAL column."""
    from acm_gnn_amd import functional as AF
    graph, dense, _ = _operator(63, True, tune)
    state = AF.DropoutState(torch.device(DEV), seed=77)
    state.step.fill_(2)
    z = np.random.RandomState(9).standard_normal((63, 260)).astype(np.float32)
    y, _ = AF.gcn_fwd(graph, torch.from_numpy(z).to(DEV), relu=True, drop=state.spec(0.5, 1))
    _close(y, np.maximum(dense @ z.astype(np.float64), 0) * _host_factors(state, 0.5, 1, 63, 260), FWD)


def test_gcn_bwd_defers_its_reduction(tune):
    """With a deferral list dW2 arrives with the flush, bit-identical to the immediate form."""
    from acm_gnn_amd import functional as AF
    graph, _, _ = _operator(300, True, tune)
    g = torch.Generator().manual_seed(3)
    dy, h, w2 = torch.randn(300, 5, generator=g).to(DEV), torch.randn(300, 32, generator=g).relu().to(DEV), torch.randn(32, 5, generator=g).to(DEV)
    _, now, _ = AF.gcn_bwd(graph, dy, h, w2)
    with AF.deferred_reductions() as d:
        _, later, _ = AF.gcn_bwd(graph, dy, h, w2, defer=d)
        assert d.pending == 1
        d.flush()
    assert torch.equal(now, later)


# ---- the five models on the recorded case -----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def case():
    return load_npz(os.path.join(GOLDEN, "baseline_cases.npz"))


@pytest.fixture(scope="module")
def a_low(case):
    return R.dense_operator(case["indptr"], case["indices"], case["vals"])


def _ops(case, implicit=True):
    from acm_gnn_amd.graph import CsrGraph, FilterOperators, as_implicit
    low = CsrGraph.from_csr(torch.from_numpy(case["indptr"]).to(DEV), torch.from_numpy(case["indices"]).to(DEV),
                            torch.from_numpy(case["vals"]).to(DEV), len(case["indptr"]) - 1)
    ops = FilterOperators(low)
    if implicit:
        ops = as_implicit(ops)
        assert ops.implicit
    return ops


def _model(case, mt, dropout=0.0):
    """baselines.GCN holding the recorded initial values: by state_dict for the baselines, by the shared names for the ACM types."""
    from acm_gnn_amd import baselines
    n, f_in = case["x"].shape
    model = baselines.GCN(f_in, int(case["hidden"]), int(case["classes"]), dropout, mt, nnodes=n if mt.startswith("acm") else None)
    recorded = R.case_params(case, mt)
    if not mt.startswith("acm"):
        model.load_state_dict({k: torch.from_numpy(v) for k, v in recorded.items()})
        return model.to(DEV)
    own = dict(model.named_parameters())
    with torch.no_grad():
        for name, v in recorded.items():
            if name in own and tuple(own[name].shape) == v.shape:
                own[name].copy_(torch.from_numpy(v))
    return model.to(DEV)


def _inputs(case):
    n = case["x"].shape[0]
    x, y = torch.from_numpy(case["x"]).to(DEV), torch.from_numpy(case["labels"]).to(DEV)
    idx = torch.from_numpy(case["train_idx"]).to(DEV)
    from acm_gnn_amd import train as T
    return x, y, idx, T.row_weights(idx, n, device=DEV)


@pytest.mark.parametrize("implicit", [True, False], ids=["implicit", "explicit"])
@pytest.mark.parametrize("mt", R.MODEL_TYPES)
def test_models_reproduce_the_recorded_reference(case, mt, implicit):
    """Eval logits, training loss and every gradient the study's own code produced; parameters it leaves without a gradient
    have none here either."""
    from acm_gnn_amd import functional as AF
    ops, model = _ops(case, implicit), _model(case, mt)
    x, y, idx, w = _inputs(case)
    model.eval()
    with torch.no_grad():
        _close(model(x, ops), case[f"{mt}/logits"], FWD, mt)
    model.train()
    loss = AF.masked_nll(model(x, ops), y, w)
    loss.backward()
    _close(loss, case[f"{mt}/loss"], FWD, mt)
    recorded = {k[len(f"{mt}/grad/"):] for k in case if k.startswith(f"{mt}/grad/")}
    for name, p in model.named_parameters():
        if name in recorded:
            _close(p.grad, case[f"{mt}/grad/{name}"], GRAD, (mt, name))
        elif not mt.startswith("acm"):
            assert p.grad is None, (mt, name)
    assert recorded <= set(dict(model.named_parameters()))


@pytest.mark.parametrize("mt", R.MODEL_TYPES)
def test_trajectories_reproduce_the_recorded_reference(case, mt):
    """Ten steps of TrainStep + FusedAdam(lr=0.05, weight_decay=5e-4) against the losses the study's loop recorded."""
    from acm_gnn_amd import FusedAdam, train as T
    ops, model = _ops(case), _model(case, mt)
    x, y, _, w = _inputs(case)
    opt = FusedAdam(model.parameters(), lr=0.05, weight_decay=5e-4)
    step = T.TrainStep(model, opt, x, ops, y, w)
    losses = [float(step()) for _ in range(len(case[f"{mt}/traj"]))]
    np.testing.assert_allclose(losses, case[f"{mt}/traj"], rtol=5e-5)


@pytest.mark.parametrize("sparse_x", [False, True], ids=["cached_P", "project_first"])
@pytest.mark.parametrize("mt", ["gcn", "mlp"])
def test_training_step_with_dropout_against_float64(case, a_low, mt, sparse_x):
    """One training step with p = 0.5: loss and gradients against baselines_ref fed the masks regenerated from the counter, with
    a dense x (gcn: the cached-P form) and with SparseFeatures (project first: the new forward kernel)."""
    from acm_gnn_amd import SparseFeatures, functional as AF
    ops, model = _ops(case), _model(case, mt, dropout=0.5)
    x, y, idx, w = _inputs(case)
    x = x * (torch.rand(x.shape, generator=torch.Generator().manual_seed(1)) < 0.7).to(DEV)       # exact zeros: a CSR structure
    xin = SparseFeatures.from_torch(x) if sparse_x else x
    model.fused_dropout, model.dropout_state = True, AF.DropoutState(torch.device(DEV), seed=99)
    model.dropout_state.step.fill_(4)
    model.train()
    loss = AF.masked_nll(model(xin, ops), y, w)
    loss.backward()
    hidden = int(case["hidden"])
    masks = {"hidden": _host_factors(model.dropout_state, 0.5, 1, x.shape[0], hidden)}
    ref_loss, ref_grads = R.loss_and_grads(R.case_params(case, mt), mt, x.cpu(), a_low, case["labels"], case["train_idx"], masks)
    _close(loss, ref_loss, FWD, mt)
    got = {k: p.grad for k, p in model.named_parameters() if p.grad is not None}
    assert set(got) == set(ref_grads)
    for name, g in ref_grads.items():
        _close(got[name], g, GRAD, (mt, name))
    if mt == "gcn":
        assert bool(model.gcns[0].held_entries()) == (not sparse_x)


@pytest.mark.parametrize("mt", ["gcn", "sgc"])
def test_captured_step_equals_eager_step(case, mt):
    from acm_gnn_amd import FusedAdam, functional as AF, train as T
    x, y, _, w = _inputs(case)

    def run(use_graph):
        ops, model = _ops(case), _model(case, mt, dropout=0.5)
        model.dropout_state = AF.DropoutState(torch.device(DEV), seed=17)
        opt = FusedAdam(model.parameters(), lr=0.05, weight_decay=5e-4)
        step = T.TrainStep(model, opt, x, ops, y, w, use_graph=use_graph)
        if use_graph and mt == "gcn":
            assert step._held                             # the captured step keeps the cached P alive
        return [float(step()) for _ in range(5)]

    np.testing.assert_allclose(run(True), run(False), rtol=2e-5)


def test_cached_p_is_computed_once_and_follows_the_input(case, a_low):
    """The second pass launches no gather for layer 1; an in-place edit of x (version bump) rebuilds P and the outputs follow."""
    from acm_gnn_amd import functional as AF
    ops, model = _ops(case), _model(case, "gcn")
    x = torch.from_numpy(case["x"]).to(DEV).clone()
    f_in = x.shape[1]
    model.eval()

    def gathers_of_the_input():
        probe = AF.KernelTimer()
        AF.set_kernel_timer(probe)
        try:
            with torch.no_grad():
                out = model(x, ops)
            counts = probe.summary()
        finally:
            AF.set_kernel_timer(None)
        return out, sum(k for label, (k, _) in counts.items() if label.startswith(f"gcn_fwd/W{f_in}") or label.startswith("spmm"))

    out1, first = gathers_of_the_input()
    out2, second = gathers_of_the_input()
    assert first == 1 and second == 0 and torch.equal(out1, out2)
    entry = model.gcns[0].held_entries()[0]
    assert entry[1] is x and entry[3] is ops
    x.add_(1.0)
    out3, third = gathers_of_the_input()
    assert third == 1
    _close(out3, R.forward(R.case_params(case, "gcn"), "gcn", x.cpu(), a_low), FWD)


@pytest.mark.parametrize("sparse_x", [False, True])
@pytest.mark.parametrize("mt", ["gcn", "sgc", "mlp"])
def test_relabelled_operators_give_the_same_logits(case, mt, sparse_x):
    from acm_gnn_amd import SparseFeatures
    from acm_gnn_amd.graph import relabel_by_degree
    ops, model = _ops(case), _model(case, mt)
    rel = relabel_by_degree(ops, force=True)
    assert rel.perm is not None
    x = torch.from_numpy(case["x"]).to(DEV)
    model.eval()
    with torch.no_grad():
        plain = model(SparseFeatures.from_torch(x) if sparse_x else x, ops)
        moved = model(SparseFeatures.from_torch(x) if sparse_x else x, rel)
        inside = model(x.index_select(0, rel.perm), rel, rows_permuted=True)
    _close(moved, plain, FWD, mt)
    _close(inside.index_select(0, rel.inv_perm), plain, FWD, mt)
    _close(plain, case[f"{mt}/logits"], FWD, mt)


@pytest.mark.parametrize("sparse_x", [False, True])
def test_three_hop_sgc_is_three_chained_products(case, sparse_x):
    from acm_gnn_amd import SparseFeatures, functional as AF
    ops, model = _ops(case), _model(case, "sgc")
    ops.hops = 3
    x = torch.from_numpy(case["x"]).to(DEV)
    model.eval()
    with torch.no_grad():
        out = model(SparseFeatures.from_torch(x) if sparse_x else x, ops)
        ref = x @ model.gcns[0].weight_low
        for _ in range(3):
            ref = AF.spmm(ops.low, ref, row_scale=ops.row_scale)
    _close(out, ref, FWD)
    model.train()
    out = model(x.clone().requires_grad_(True), ops)                  # an input that needs a gradient: project first, then gather
    _close(out, ref, FWD)


def test_row_sharded_operators_are_refused(case):
    ops, model = _ops(case), _model(case, "gcn")
    ops.group = object()
    assert ops.sharded
    with pytest.raises(NotImplementedError, match="row-sharded"):
        model(torch.from_numpy(case["x"]).to(DEV), ops)


# ---- the study's split -------------------------------------------------------------------------------------------------------
def _check_split(labels, c, split):
    n = labels.numel()
    tr, va, te = split
    per_class, n_val = int(round(0.6 * (n / c))), int(round(0.2 * n))
    counts = torch.bincount(labels, minlength=c)
    for t in split:
        assert t.dtype == torch.int64 and t.device == labels.device and bool((t[1:] > t[:-1]).all())
    both = torch.cat(split)
    assert both.numel() == n and torch.equal(torch.sort(both).values, torch.arange(n, device=labels.device))      # disjoint, covering
    assert torch.equal(torch.bincount(labels[tr], minlength=c), counts.clamp(max=per_class))                      # every class's share
    assert va.numel() == min(n_val, n - tr.numel()) and te.numel() == n - tr.numel() - va.numel()


def test_disassortative_splits():
    from acm_gnn_amd import synthetic as S
    g = S.generate_graph("regular", 5, 400, degree_intra=2, edge_homo=0.3, seed=1, device=DEV)
    skew = torch.from_numpy(np.repeat(np.arange(4), [700, 200, 90, 10])).to(DEV)       # a class below its training share
    skew = skew[torch.randperm(skew.numel(), generator=torch.Generator().manual_seed(0)).to(DEV)]
    for labels, c in ((g.labels, 5), (skew, 4)):
        a = S.disassortative_splits(labels, c, seed=5, split_index=0)
        _check_split(labels, c, a)
        again = S.disassortative_splits(labels, c, seed=5, split_index=0)
        assert all(torch.equal(p, q) for p, q in zip(a, again))
        other = S.disassortative_splits(labels, c, seed=5, split_index=1)
        _check_split(labels, c, other)
        assert not torch.equal(a[0], other[0])
    tr = S.disassortative_splits(g.labels, 5, seed=5)[0]
    assert tr.numel() == 5 * 240


def test_end_to_end_fit_on_a_generated_graph():
    """generate_graph -> operators -> disassortative_splits -> fit(baselines.GCN, rule="min_val_loss", use_graph=True)."""
    from acm_gnn_amd import FusedAdam, baselines, synthetic as S, train as T
    g = S.generate_graph("regular", 5, 400, degree_intra=2, edge_homo=0.3, seed=2, device=DEV)
    ops = g.operators()
    x = S.random_features(g.n, 64, seed=2, device=DEV)
    tr, va, te = S.disassortative_splits(g.labels, 5, seed=2)
    model = baselines.GCN(64, 32, 5, 0.5, "gcn").to(DEV)
    opt = FusedAdam(model.parameters(), lr=0.05, weight_decay=5e-4)
    acc, history = T.fit(model, opt, x, ops, g.labels, tr, va, te, epochs=30, rule="min_val_loss", early_stopping=200, use_graph=True)
    assert np.isfinite(acc) and len(history) == 30 and all(np.isfinite(row).all() for row in history)


# ---- launch forms no small case reaches: exact integers against scipy.sparse in int64 -------------------------------------------
# Unit-valued pattern operators and small integer operands: every product and every partial sum is an integer below 2^24, so
# any summation order and any slab assignment give the same bits and the comparisons are torch.equal.
EXACT = 2 ** 24


def _pattern_operator(n, tune, density=None):
    """(CsrGraph of a unit-valued pattern, the same pattern as a scipy int64 CSR matrix): the file's generator and its cache
    at the default density, a private draw of the same generator otherwise."""
    import scipy.sparse as sp
    if density is None:
        graph, dense, _ = _operator(n, False, tune)
    else:
        tune(chunk=256)
        key = (n, False, density)
        if key not in _OPERATORS:
            _OPERATORS[key] = _make_operator(n, False, density=density)
        graph, dense, _ = _OPERATORS[key]
    return graph, sp.csr_matrix((dense != 0).astype(np.int64))


def _sparse_pattern_operator(n, mean_degree, seed):
    """The same kind of operator at a size where the generator's dense n x n draw no longer fits a quick test: a random
    pattern of ``mean_degree`` entries per row, node 0 adjacent to every node, row n // 2 empty."""
    import scipy.sparse as sp
    from acm_gnn_amd.graph import CsrGraph
    rng = np.random.RandomState(seed)
    m = n * mean_degree
    a = sp.coo_matrix((np.ones(m + 2 * n, np.int64),
                       (np.concatenate([rng.randint(0, n, m), np.zeros(n, np.int64), np.arange(n)]),
                        np.concatenate([rng.randint(0, n, m), np.arange(n), np.zeros(n, np.int64)]))), shape=(n, n)).tocsr()
    a.data[:] = 1
    a = a.tolil()
    a[n // 2, :] = 0
    a = a.tocsr()
    a.eliminate_zeros()
    a.sort_indices()
    graph = CsrGraph.from_csr(torch.from_numpy(a.indptr.astype(np.int32)).to(DEV), torch.from_numpy(a.indices.astype(np.int32)).to(DEV),
                              None, n, chunk=256)
    return graph, a.astype(np.int64)


def _nan_padded(a, pad=3):
    """``a`` on the device as the leading columns of a NaN-filled wider buffer."""
    wide = torch.full((a.shape[0], a.shape[1] + pad), float("nan"), device=DEV)
    wide[:, :a.shape[1]] = torch.from_numpy(a).to(DEV)
    return wide[:, :a.shape[1]]


def _bwd_exact_case(pattern, hidden, width, seed):
    """(dy, h, w2 as fp32 integers, dz int64) with every partial sum of dz, of dz W2^T and of H^T dz below 2^24."""
    n = pattern.shape[0]
    rng = np.random.RandomState(seed)
    dy = rng.randint(-2, 3, (n, width)).astype(np.float32)
    w2 = rng.randint(-2, 3, (hidden, width)).astype(np.float32)
    h = (rng.randint(0, 4, (n, hidden)) * (rng.rand(n, hidden) < 0.6)).astype(np.float32)
    assert (h == 0).mean() >= 0.30
    dz = pattern @ dy.astype(np.int64)
    abs_dz = pattern @ np.abs(dy).astype(np.int64)
    assert abs_dz.max() < EXACT and 2 * (abs_dz @ np.abs(w2).astype(np.int64).T).max() < EXACT
    assert (h.astype(np.int64).T @ abs_dz).max() < EXACT
    return dy, h, w2, dz


def _bwd_refs(dz, h, w2, relu, ks):
    mask = (h > 0) if relu else (h != 0)
    g = (dz @ w2.astype(np.int64).T) * mask * int(ks)
    dw = h.astype(np.int64).T @ dz
    return (torch.from_numpy(t.astype(np.float32)) for t in (g, dw, dz))


BWD_MODES = ((True, 2.0), (True, 1.0), (False, 2.0))


def _check_bwd_exact(graph, pattern, hidden, width, seed, lanes):
    from acm_gnn_amd import functional as AF
    avg = pattern.nnz / pattern.shape[0]
    want_lanes = 8 if avg <= LF.T["NARROW_8_LANES_UP_TO"] else (16 if avg <= LF.T["NARROW_16_LANES_UP_TO"] else 32)
    if want_lanes == 16 and width >= 5:                       # (5..8 columns never take sixteen lanes)
        want_lanes = 32
    assert want_lanes == lanes, (avg, width)                  # the case runs the form it is listed for (acm_gcn.hip: gcn_bwd_plan)
    dy, h, w2, dz_ref = _bwd_exact_case(pattern, hidden, width, seed)
    dyd, hd, w2d = _nan_padded(dy), _nan_padded(h), _nan_padded(w2)
    for relu, ks in BWD_MODES:
        g_ref, dw_ref, dz_want = _bwd_refs(dz_ref, h, w2, relu, ks)
        g, dw, dz = AF.gcn_bwd(graph, dyd, hd, w2d, keep_scale=ks, relu=relu, want_dz=True)
        what = (pattern.shape[0], hidden, width, relu, ks)
        assert torch.equal(dz.cpu(), dz_want), what
        assert torch.equal(g.cpu(), g_ref), what
        assert torch.equal(dw.cpu(), dw_ref), what


@pytest.mark.parametrize("n,density,lanes", LF.GCN_BWD_OPERATORS)
def test_gcn_bwd_is_exact_on_integers(n, density, lanes, tune):
    """Every (hidden, width) whose dW2 slabs end in a partial group of 32, hidden below the lanes of a group and hidden at the
    limit, with 8, 16 and 32 lanes per work item; inputs are column slices of NaN-filled buffers."""
    graph, pattern = _pattern_operator(n, tune, density)
    if n >= 300:
        assert graph.n_long_rows >= 1
    for hidden, width in LF.GCN_BWD_SHAPES:
        _check_bwd_exact(graph, pattern, hidden, width, 7 * n + hidden + width, 32 if lanes == 16 and width >= 5 else lanes)


@pytest.mark.parametrize("n,mean_degree,hidden,width,lanes", LF.GCN_BWD_HELD_GRIDS)
def test_gcn_bwd_is_exact_with_the_gather_grid_at_its_cap(n, mean_degree, hidden, width, lanes, tune):
    """More work items than GCN_BWD_MAX_BLOCKS blocks of groups: a group adds several items into its slab."""
    if n <= 2500:
        graph, pattern = _pattern_operator(n, tune)
    else:
        tune(chunk=256)
        graph, pattern = _sparse_pattern_operator(n, mean_degree, n)
    assert graph.n_long_rows >= 1 and graph.n_items > LF.GCN_BWD_MAX_BLOCKS * (256 // lanes)
    _check_bwd_exact(graph, pattern, hidden, width, n, lanes)


@pytest.mark.parametrize("n,hidden,width", [(63, 33, 3), (300, 9, 5)])
def test_gcn_bwd_leaves_the_padding_of_its_outputs_alone(n, hidden, width, tune):
    """One raw acm_gcn_bwd call with ld_g, ld_dw2 and ld_dz above the widths: the guard columns survive, the rest is exact."""
    import ctypes as C
    from acm_gnn_amd import _lib
    from acm_gnn_amd.functional._launch import _vp, _workspace_sized, launch
    graph, pattern = _pattern_operator(n, tune)
    dy, h, w2, dz_ref = _bwd_exact_case(pattern, hidden, width, n)
    dyd, hd, w2d = _nan_padded(dy), _nan_padded(h), _nan_padded(w2)
    guard = -77.0
    g = torch.full((n, hidden + 2), guard, device=DEV)
    dw = torch.full((hidden, width + 3), guard, device=DEV)
    dz = torch.full((n, width + 1), guard, device=DEV)
    ws, nbytes = _workspace_sized(torch.device(DEV), "acm_gcn_bwd_workspace_bytes", graph.handle, width, hidden)
    p = _lib.GcnBwd()
    p.width, p.hidden, p.keep_scale, p.relu = width, hidden, 2.0, 1
    p.dy, p.ld_dy, p.h, p.ld_h, p.w2, p.ld_w2 = dyd.data_ptr(), dyd.stride(0), hd.data_ptr(), hd.stride(0), w2d.data_ptr(), w2d.stride(0)
    p.g, p.ld_g, p.d_w2, p.ld_dw2, p.dz, p.ld_dz = g.data_ptr(), g.stride(0), dw.data_ptr(), dw.stride(0), dz.data_ptr(), dz.stride(0)
    p.defer = None
    launch("acm_gcn_bwd", None, torch.device(DEV), graph.handle, C.byref(p), _vp(ws), nbytes)
    torch.cuda.synchronize()
    g_ref, dw_ref, dz_want = _bwd_refs(dz_ref, h, w2, True, 2.0)
    assert torch.equal(g[:, :hidden].cpu(), g_ref) and bool((g[:, hidden:] == guard).all())
    assert torch.equal(dw[:, :width].cpu(), dw_ref) and bool((dw[:, width:] == guard).all())
    assert torch.equal(dz[:, :width].cpu(), dz_want) and bool((dz[:, width:] == guard).all())


@pytest.mark.parametrize("n", [63, 1025])
def test_gcn_fwd_is_exact_on_integers(n, tune):
    """The ridden projection at every width class up to 256 and the column-block splits beyond (128 + rest, 256 + rest): integer
    z and W_next, keep factor exactly 2, the mask a function of the global column.  At n = 1025 the hub row takes the fix-up."""
    from acm_gnn_amd import functional as AF
    graph, pattern = _pattern_operator(n, tune)
    if n == 1025:
        assert graph.n_long_rows >= 1
    state = AF.DropoutState(torch.device(DEV), seed=4321 + n)
    state.step.fill_(5)
    rng = np.random.RandomState(n)
    cases = [(w, f) for w in LF.GCN_FWD_RIDDEN_WIDTHS for f in (1, 8)] + [(w, 0) for w in LF.GCN_FWD_SPLIT_WIDTHS]
    for width, f_next in cases:
        z = rng.randint(-2, 3, (n, width)).astype(np.float32)
        az = pattern @ z.astype(np.int64)
        assert (pattern @ np.abs(z).astype(np.int64)).max() < EXACT
        factors = _host_factors(state, 0.5, 3, n, width)
        assert set(np.unique(factors)) == {0.0, 2.0}
        w_next = rng.randint(-2, 3, (width, f_next)).astype(np.float32) if f_next else None
        zd = torch.from_numpy(z).to(DEV)
        wn = _nan_padded(w_next, 1) if f_next else None
        for relu, p in ((False, 0.0), (True, 0.0), (True, 0.5), (False, 0.5)):
            ref = np.maximum(az, 0) if relu else az
            if p:
                ref = ref * factors.astype(np.int64)
            buf = torch.full((n, width + 3), 7.0, device=DEV)
            nbuf = torch.full((n, f_next + 2), 7.0, device=DEV) if f_next else None
            y, zn = AF.gcn_fwd(graph, zd, relu=relu, drop=state.spec(p, 3) if p else None, w_next=wn, out=buf[:, :width],
                               out_next=nbuf[:, :f_next] if f_next else None)
            what = (n, width, f_next, relu, p)
            assert torch.equal(y.cpu(), torch.from_numpy(ref.astype(np.float32))), what
            assert bool((buf[:, width:] == 7.0).all()), what
            if f_next:
                assert (np.abs(ref) @ np.abs(w_next).astype(np.int64)).max() < EXACT
                assert torch.equal(zn.cpu(), torch.from_numpy((ref @ w_next.astype(np.int64)).astype(np.float32))), what
                assert bool((nbuf[:, f_next:] == 7.0).all()), what
