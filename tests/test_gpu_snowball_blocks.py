"""ACM-Snowball on CSR features on the MI355X: acm_proj_blocks_fwd / _bwd against float64, models.GCN("acmsnowball") handed
SparseFeatures against the oracle, explicit blocks against the concatenation, the memory the route never allocates, the
training step (eager, captured, relabelled) and the refusals."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

from oracle import acm_oracle as O
from test_gpu_oracle import _graph, _philox_mask
from test_snowball_blocks_cpu import sparse_features

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


# ---------------------------------------------------------------------------------------------- 1. the kernels against float64
def _channels(t, f, fb):
    return torch.cat([t[:, c * fb:c * fb + f] for c in range(3)], 1)


def _project_case(n, first, widths, f, relu, seed):
    """One forward + backward of AF.project_blocks on the device against the same products in float64 on the CPU, by the
    criterion of test_gpu_kernels.py::test_gemm_matches_fp64: err / (|A| |B| + 1e-30) < 2e-6 over the same terms.  ReLU on:
    entries whose float64 pre-activation lies within 1e-6 |A| |B| of zero take no part in the gradients (their upstream
    gradient is zero on both sides), at most 1 % of the entries.  Returns the device results of two identical calls."""
    from acm_gnn_amd import functional as AF
    from acm_gnn_amd.graph import SparseFeatures, clear_cache
    clear_cache()
    g = torch.Generator().manual_seed(seed)
    if first == "csr":
        xd = sparse_features(n, 300, seed)
    elif first == "empty":
        xd = torch.zeros(n, 300)
    else:
        xd = torch.randn(n, 11, generator=g)
    hs = [torch.randn(n, w, generator=g) for w in widths]
    f_in = xd.shape[1] + sum(widths)
    w3 = [torch.randn(f_in, f, generator=g) / 8 for _ in range(3)]
    gz = torch.randn(n, 3 * f, generator=g)
    fb = AF.blocks._chan_block(f)
    # float64 on the CPU
    xcat = torch.cat([xd] + hs, 1).double()
    wcat = torch.cat(w3, 1).double()
    pre = xcat @ wcat
    scale = xcat.abs() @ wcat.abs()
    if relu:
        near = pre.abs() <= 1e-6 * scale
        assert int(near.sum()) <= 0.01 * near.numel(), (int(near.sum()), near.numel())
        gz = gz * ~near
    ref = pre.clamp_min(0) if relu else pre
    dz = gz.double() * (pre > 0) if relu else gz.double()
    ref_dx, ref_dw = dz @ wcat.T, xcat.T @ dz
    sc_dx, sc_dw = dz.abs() @ wcat.abs().T, xcat.abs().T @ dz.abs()
    # the device, twice
    runs = []
    for _ in range(2):
        hd = [h.to(DEV).requires_grad_(True) for h in hs]
        wd = [w.to(DEV).requires_grad_(True) for w in w3]
        x0 = xd.to(DEV) if first == "dense" else SparseFeatures.from_torch(xd.to(DEV))
        z = AF.project_blocks([x0] + hd, wd, relu=relu)
        assert tuple(z.shape) == (n, 2 * fb + f)
        gzd = torch.zeros(n, 2 * fb + f, device=DEV)
        for c in range(3):
            gzd[:, c * fb:c * fb + f] = gz[:, c * f:(c + 1) * f].to(DEV)
        z.backward(gzd)
        runs.append((z.detach().clone(), [h.grad.clone() for h in hd], [w.grad.clone() for w in wd]))
    z, dh, dw = runs[0]
    err = (_channels(z, f, fb).cpu().double() - ref).abs()
    print(f"n={n} first={first} widths={widths} f={f} relu={relu}: Z {float((err / (scale + 1e-30)).max()):.3e}", end=" ")
    assert float((err / (scale + 1e-30)).max()) < 2e-6, float(err.max())
    if fb != f:
        assert float(z[:, f:fb].abs().max()) == 0.0 and float(z[:, fb + f:2 * fb].abs().max()) == 0.0
    col = xd.shape[1]
    for j, w in enumerate(widths):
        err = (dh[j].cpu().double() - ref_dx[:, col:col + w]).abs()
        print(f"dH{j} {float((err / (sc_dx[:, col:col + w] + 1e-30)).max()):.3e}", end=" ")
        assert float((err / (sc_dx[:, col:col + w] + 1e-30)).max()) < 2e-6, (j, float(err.max()))
        col += w
    for c in range(3):
        err = (dw[c].cpu().double() - ref_dw[:, c * f:(c + 1) * f]).abs()
        print(f"dW{c} {float((err / (sc_dw[:, c * f:(c + 1) * f] + 1e-30)).max()):.3e}", end=" ")
        assert float((err / (sc_dw[:, c * f:(c + 1) * f] + 1e-30)).max()) < 2e-6, (c, float(err.max()))
    print()
    # two calls on the same inputs: the same bits
    assert torch.equal(runs[0][0], runs[1][0])
    for a, b in zip(runs[0][1] + runs[0][2], runs[1][1] + runs[1][2]):
        assert torch.equal(a, b)


@pytest.mark.parametrize("relu", [False, True], ids=["id", "relu"])
@pytest.mark.parametrize("f", [24, 64, 4, 7])
@pytest.mark.parametrize("widths", [[24], [24, 24, 24], [64, 64, 64], [8]], ids=lambda w: "x".join(map(str, w)))
def test_project_blocks_matches_fp64(widths, f, relu):
    from acm_gnn_amd import functional as AF
    timer = AF.KernelTimer()
    AF.set_kernel_timer(timer)
    try:
        for n in (1, 15, 17, 350):
            _project_case(n, "csr", widths, f, relu, seed=n + 7 * f + sum(widths))
    finally:
        AF.set_kernel_timer(None)
    used = set(k.split("/")[0] for k in timer.events)
    assert {"proj_blocks_fwd", "proj_blocks_bwd"} <= used and not any(k.startswith("gemm") for k in used), used


@pytest.mark.parametrize("first", ["empty", "dense"])
@pytest.mark.parametrize("f,relu", [(24, True), (7, False)])
def test_project_blocks_other_first_blocks(first, f, relu):
    """A CSR matrix without a stored entry, and a dense first block of 11 columns (projected by acm_gemm, accumulated on)."""
    for n in (17, 350):
        _project_case(n, first, [24, 24, 24], f, relu, seed=n + f)


@pytest.mark.parametrize("widths", [[6], [68], [24, 6]], ids=lambda w: "x".join(map(str, w)))
@pytest.mark.parametrize("f,relu", [(24, False), (4, True)])
def test_widths_outside_the_envelope_take_the_composed_form(widths, f, relu):
    from acm_gnn_amd import functional as AF
    timer = AF.KernelTimer()
    AF.set_kernel_timer(timer)
    try:
        for n in (17, 350):
            _project_case(n, "csr", widths, f, relu, seed=n + f + sum(widths))
    finally:
        AF.set_kernel_timer(None)
    used = set(k.split("/")[0] for k in timer.events)
    assert "proj_blocks_fwd" not in used and "proj_blocks_bwd" not in used and any(k.startswith("gemm") for k in used), used


# ---------------------------------------------------------------------------------------------- 2. the model against the oracle
def _snowball_case(n=350, seed=6):
    adj = _graph(n, 12)
    low, high, _ = O.filters_linkx(adj)
    x = sparse_features(n, 300, seed)
    y = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(seed))
    return low, high, x, y, torch.arange(1, n, 2)


@pytest.mark.parametrize("variant,nlayers,p_drop", [(0, 2, 0.0), (1, 3, 0.0), (0, 2, 0.35)])
def test_snowball_on_csr_features_matches_oracle(variant, nlayers, p_drop):
    """The cases and bounds of test_gpu_oracle.py::test_snowball_matches_oracle with 300 sparse features handed over as
    SparseFeatures; the reference is the oracle on the densified x.  The input mask is one value per STORED entry ([nnz, 1], tag 0)
    scattered to its dense position."""
    from acm_gnn_amd import GCN, functional as AF
    from acm_gnn_amd.graph import SparseFeatures, clear_cache
    clear_cache()
    n = 350
    low, high, x, y, idx = _snowball_case(n)
    torch.manual_seed(8)
    model = GCN(300, 24, 4, nlayers, n, p_drop, "acmsnowball", 0, variant=bool(variant))
    params = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in model.named_parameters()
              if k not in ("fea_param", "xX_param")}
    model = model.to(DEV)
    xs = SparseFeatures.from_torch(x.to(DEV))
    masks = None
    if p_drop:
        model.fused_dropout, model.dropout_state = True, AF.DropoutState(DEV, seed=5)
        model.dropout_state.step.fill_(3)
        st = model.dropout_state
        ip, ix, _ = xs.csr.arrays()
        ip, ix = ip.cpu().long(), ix.cpu().long()
        rows = torch.repeat_interleave(torch.arange(n), ip[1:] - ip[:-1])
        mx = torch.ones(n, 300)
        mx[rows, ix] = _philox_mask(st, p_drop, 0, int(ip[-1]), 1).reshape(-1)
        masks = {"x": mx}
        masks.update({f"h{k}": _philox_mask(st, p_drop, 1 + k, n, 24) for k in range(nlayers)})
    model.train()
    timer = AF.KernelTimer()
    AF.set_kernel_timer(timer)
    try:
        out = model(xs, low.to(DEV), high.to(DEV), None)
        loss = F.nll_loss(torch.log_softmax(out, 1)[idx.to(DEV)], y.to(DEV)[idx.to(DEV)])
        loss.backward()
    finally:
        AF.set_kernel_timer(None)
    used = set(k.split("/")[0] for k in timer.events)
    assert {"proj_blocks_fwd", "proj_blocks_bwd"} <= used, used
    ref = O.snowball_forward(params, x, low, high, nlayers=nlayers, variant=bool(variant), dropout=p_drop, training=True,
                             masks=masks)
    O.nll_loss_on(ref, y, idx).backward()
    assert float((out.detach().cpu() - ref.detach()).abs().max()) < 3e-5 * max(1.0, float(ref.detach().abs().max()))
    for k, p in model.named_parameters():
        if k in params and params[k].grad is not None:
            rg = params[k].grad
            assert p.grad is not None, k
            assert float((p.grad.cpu() - rg).abs().max()) < 1e-4 * max(1.0, float(rg.abs().max())), k


# ---------------------------------------------------------------------------------------------- 3. blocks = concatenation
@pytest.mark.parametrize("variant", [0, 1])
def test_explicit_blocks_equal_the_concatenation(variant):
    from acm_gnn_amd import GraphConvolution
    from acm_gnn_amd.graph import clear_cache
    clear_cache()
    n = 350
    low, high, _ = O.filters_linkx(_graph(n, 12))
    low, high = low.to(DEV), high.to(DEV)
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, 11, generator=g).to(DEV)
    hs = [torch.randn(n, 24, generator=g).to(DEV) for _ in range(2)]
    gout = torch.randn(n, 24, generator=g).to(DEV)
    torch.manual_seed(5)
    layer = GraphConvolution(11 + 48, 24, n, "acmsnowball", variant=bool(variant)).to(DEV)
    res = {}
    for form in ("blocks", "cat"):
        layer.zero_grad()
        h = [t.clone().requires_grad_(True) for t in hs]
        out = layer([x] + h if form == "blocks" else torch.cat([x] + h, 1), low, high, None)
        out.backward(gout)
        res[form] = (out.detach(), {k: p.grad.clone() for k, p in layer.named_parameters() if p.grad is not None},
                     [t.grad.clone() for t in h])
    a, b = res["blocks"], res["cat"]
    assert float((a[0] - b[0]).abs().max()) < 3e-5 * max(1.0, float(b[0].abs().max()))
    assert set(a[1]) == set(b[1])
    for k, rg in b[1].items():
        assert float((a[1][k] - rg).abs().max()) < 1e-4 * max(1.0, float(rg.abs().max())), k
    for j, rg in enumerate(b[2]):
        assert float((a[2][j] - rg).abs().max()) < 1e-4 * max(1.0, float(rg.abs().max())), f"h{j}"


# ---------------------------------------------------------------------------------------------- 4. memory
def test_nothing_of_the_dense_width_is_allocated():
    """n = 8192, F_in = 16 384 (8 stored values per row), nhid 64, two hidden layers: one dense copy of the input is 536 870 912
    bytes; a forward + backward of the CSR route stays below half of that above what is allocated before it.  (Measured on the
    MI355X: see EXPERIMENTS.md, "ACM-Snowball on CSR features".)"""
    from acm_gnn_amd import GCN
    from acm_gnn_amd.graph import CsrGraph, FilterOperators, SparseFeatures, clear_cache
    from acm_gnn_amd import data as D
    clear_cache()
    n, f_in = 8192, 16384
    rng = np.random.default_rng(0)
    cols = rng.integers(0, f_in, size=(n, 8))
    feats = sp.csr_matrix((np.ones(n * 8, np.float32), (np.repeat(np.arange(n), 8), cols.reshape(-1))), shape=(n, f_in))
    feats.sum_duplicates()
    a = sp.random(n, n, density=4.0 / n, random_state=rng, format="csr")
    adj = ((a + a.T) > 0).astype(np.float64).tocsr()
    low, _ = D.build_filters(adj)
    ops = FilterOperators(CsrGraph.from_scipy(low, DEV))
    xs = SparseFeatures.from_scipy(feats, DEV)
    y = torch.from_numpy(rng.integers(0, 4, n)).to(DEV)
    torch.manual_seed(0)
    model = GCN(f_in, 64, 4, 2, n, 0.0, "acmsnowball", 0).to(DEV)
    model.train()

    def step():
        model.zero_grad(set_to_none=True)
        out = model(xs, ops, None, None)
        F.nll_loss(torch.log_softmax(out, 1), y).backward()
        return out

    step()                                                     # warm-up: the transposed CSR, workspaces
    torch.cuda.synchronize()
    model.zero_grad(set_to_none=True)
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    out = step()
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - before
    print(f"peak above the resident state: {peak} bytes ({peak / 2**20:.1f} MiB)")
    assert torch.isfinite(out).all()
    assert peak < n * f_in * 4 // 2 == 268435456, peak


# ---------------------------------------------------------------------------------------------- 5. the training step
def _train_losses(use_graph, p_drop, steps, lr=0.01):
    from acm_gnn_amd import GCN, FusedAdam, train as T
    from acm_gnn_amd.graph import SparseFeatures, clear_cache
    clear_cache()
    n = 350
    low, high, x, y, idx = _snowball_case(n)
    torch.manual_seed(8)
    model = GCN(300, 24, 4, 2, n, p_drop, "acmsnowball", 0).to(DEV)
    opt = FusedAdam(model.parameters(), lr=lr)
    state = {k: v.clone() for k, v in model.state_dict().items()}
    w = T.row_weights(idx.to(DEV), n)
    step = T.TrainStep(model, opt, SparseFeatures.from_torch(x.to(DEV)), low.to(DEV), y.to(DEV), w, high.to(DEV), None,
                       use_graph=use_graph)
    assert isinstance(step.x, SparseFeatures)
    if p_drop:
        assert model.fused_dropout
    if use_graph:                                              # the capture warm-up advanced weights, moments and the counter
        model.load_state_dict(state)
        for stt in opt.state.values():
            for v in stt.values():
                if torch.is_tensor(v):
                    v.zero_()
        if p_drop:
            model.dropout_state.step.zero_()
    losses = [float(step()) for _ in range(steps)]
    step.grads = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    return losses, step


def test_training_step_eager_and_captured_give_the_same_bits():
    eager, _ = _train_losses(False, 0.35, 5)
    graph, _ = _train_losses(True, 0.35, 5)
    print("eager", eager, "captured", graph)
    assert all(np.isfinite(eager)) and len(set(eager)) == 5
    assert eager == graph


def test_training_step_on_relabelled_operators():
    """The same check with the rows relabelled by degree (x.permute_rows): eager and captured steps agree bit for bit, and the
    loss is within 1e-6 of the unpermuted run (the bound of test_host_stack_cpu.py:1250, which -- as there -- is taken without
    dropout: the counter-based masks are functions of the row's position, so a permuted run with p > 0 draws other masks).  The
    parameter gradients of that step -- the permuted backward against the unpermuted one -- agree within the oracle
    comparison's gradient bound, 1e-4 max(1, |grad|_inf); no parameter of this model is indexed by row."""
    from acm_gnn_amd import tuning
    plain, plain_step = _train_losses(False, 0.0, 1, lr=0.0)
    with tuning.override(relabel=1):
        eager, step = _train_losses(False, 0.35, 5)
        assert step._permuted
        graph, _ = _train_losses(True, 0.35, 5)
        assert eager == graph, (eager, graph)
        relabelled, step = _train_losses(False, 0.0, 1, lr=0.0)
        assert step._permuted
    print("plain", plain, "relabelled", relabelled)
    assert abs(plain[0] - relabelled[0]) < 1e-6, (plain, relabelled)
    assert set(plain_step.grads) == set(step.grads) and len(step.grads) >= 18
    for k, rg in plain_step.grads.items():
        err = float((step.grads[k] - rg).abs().max())
        print(k, err, float(rg.abs().max()))
        assert err < 1e-4 * max(1.0, float(rg.abs().max())), k


def test_fit_with_graphs_runs_five_epochs():
    from acm_gnn_amd import GCN, FusedAdam, train as T
    from acm_gnn_amd.graph import SparseFeatures, clear_cache
    clear_cache()
    n = 350
    low, high, x, y, idx = _snowball_case(n)
    torch.manual_seed(8)
    model = GCN(300, 24, 4, 2, n, 0.35, "acmsnowball", 0).to(DEV)
    opt = FusedAdam(model.parameters(), lr=0.01)
    sets = [idx.to(DEV), torch.arange(0, n, 4).to(DEV), torch.arange(2, n, 4).to(DEV)]
    sel, hist = T.fit(model, opt, SparseFeatures.from_torch(x.to(DEV)), low.to(DEV), y.to(DEV), *sets, epochs=5, adj_high=high.to(DEV),
                      use_graph=True)
    assert len(hist) == 5 and np.isfinite(sel)
    assert np.isfinite(np.asarray(hist, dtype=np.float64)).all(), hist


# ---------------------------------------------------------------------------------------------- 6. refusals
def test_refusals(monkeypatch):
    from acm_gnn_amd import GCN, GraphConvolution
    from acm_gnn_amd.graph import SparseFeatures, clear_cache, operators_for
    clear_cache()
    n = 60
    low, high, _ = O.filters_linkx(_graph(n, 4, density=0.1))
    low, high = low.to(DEV), high.to(DEV)
    layer = GraphConvolution(11 + 24, 8, n, "acmsnowball").to(DEV)
    x, h = torch.randn(n, 11, device=DEV), torch.randn(n, 24, device=DEV)
    with pytest.raises(ValueError, match="block 1"):
        layer([x, torch.randn(n, 20, device=DEV)], low, high, None)
    with pytest.raises(ValueError, match="block 1.*cpu"):
        layer([x, h.cpu()], low, high, None)
    with pytest.raises(ValueError, match="block 1.*float32"):
        layer([x, h.half()], low, high, None)
    with pytest.raises(ValueError, match="block 1.*rows"):
        layer([x, torch.randn(n - 1, 24, device=DEV)], low, high, None)
    ops = operators_for(low, high, None)
    monkeypatch.setattr(type(ops), "sharded", property(lambda self: True))
    with pytest.raises(NotImplementedError, match="row-sharded"):
        layer([x, h], ops, None, None)
    model = GCN(300, 8, 3, 2, n, 0.0, "acmsnowball", 0).to(DEV)
    with pytest.raises(NotImplementedError, match="row-sharded"):
        model(SparseFeatures.from_torch(sparse_features(n, 300, 1).to(DEV)), ops, None, None)
