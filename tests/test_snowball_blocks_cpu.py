"""ACM-Snowball on CSR features, host side: block inputs through functional.project_blocks, layers.GraphConvolution and
models.GCN on the numpy test double (tests/fake_lib.py + tests/fake_lib_blocks.py), and the real library's new symbols."""
import numpy as np
import pytest
import scipy.sparse as sp
import torch
import torch.nn.functional as F

import fake_lib_blocks
from oracle import acm_oracle as O


def _graph(n, seed, density=0.05, hub=True):
    """(the helper of tests/test_gpu_oracle.py)"""
    rng = np.random.default_rng(seed)
    a = sp.random(n, n, density=density, random_state=rng, format="csr")
    a = ((a + a.T) > 0).astype(np.float64).tolil()
    if hub:
        a[0, 1:] = 1.0
        a[1:, 0] = 1.0
    a[n - 1, :] = 0
    a[:, n - 1] = 0
    a[3, 3] = 1.0
    return sp.csr_matrix(a)


def sparse_features(n, cols, seed, density=0.02):
    """[n, cols] features with about ``density`` of the entries stored and some rows empty."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, cols, generator=g) * (torch.rand(n, cols, generator=g) < density)
    x[::7] = 0.0
    return x


def _grads(model):
    return {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}


@pytest.mark.parametrize("variant,nlayers", [(0, 2), (1, 3)])
def test_snowball_on_csr_features_matches_oracle(variant, nlayers, monkeypatch):
    """models.GCN("acmsnowball") handed SparseFeatures: layer 0 takes them, the layers behind it the list [x, h_0, ...];
    against the oracle's restatement of the reference forward on the densified features (bounds of
    test_gpu_oracle.py::test_snowball_matches_oracle)."""
    fake_lib_blocks.install(monkeypatch)
    from acm_gnn_amd import GCN, functional as AF
    from acm_gnn_amd.graph import SparseFeatures
    n = 350
    low, high, _ = O.filters_linkx(_graph(n, 12))
    x = sparse_features(n, 300, 6)
    y = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(6))
    idx = torch.arange(1, n, 2)
    torch.manual_seed(8)
    model = GCN(300, 24, 4, nlayers, n, 0.0, "acmsnowball", 0, variant=bool(variant))
    params = {k: v.detach().clone().requires_grad_(True) for k, v in model.named_parameters() if k not in ("fea_param", "xX_param")}
    model.train()
    seen = []
    monkeypatch.setattr(AF.blocks, "launch", lambda name, *a, _l=AF.blocks.launch, **k: (seen.append(name), _l(name, *a, **k))[1])
    monkeypatch.setattr(torch, "cat", lambda ts, *a, _c=torch.cat, **k: _no_wide_cat(_c(ts, *a, **k), 300))
    out = model(SparseFeatures.from_torch(x), low, high, None)
    F.nll_loss(torch.log_softmax(out, 1)[idx], y[idx]).backward()
    assert seen.count("acm_proj_blocks_fwd") == nlayers and seen.count("acm_proj_blocks_bwd") == nlayers, seen
    monkeypatch.undo()
    ref = O.snowball_forward(params, x, low, high, nlayers=nlayers, variant=bool(variant), dropout=0.0, training=True, masks=None)
    O.nll_loss_on(ref, y, idx).backward()
    assert float((out.detach() - ref.detach()).abs().max()) < 3e-5 * max(1.0, float(ref.detach().abs().max()))
    for k, p in model.named_parameters():
        if k in params and params[k].grad is not None:
            rg = params[k].grad
            assert p.grad is not None, k
            assert float((p.grad - rg).abs().max()) < 1e-4 * max(1.0, float(rg.abs().max())), k


def _no_wide_cat(t, nfeat):
    assert t.dim() != 2 or t.shape[0] < 300 or t.shape[1] < nfeat or t.shape[0] == t.shape[1], f"a concatenation of {tuple(t.shape)}"
    return t


@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("out_features", [24, 4])
def test_explicit_blocks_equal_the_concatenation(variant, out_features, monkeypatch):
    """GraphConvolution fed [x, h0, h1] against the same layer fed torch.cat of them: outputs and every gradient, those into h0 and
    h1 included (bounds of the oracle comparison)."""
    fake_lib_blocks.install(monkeypatch)
    from acm_gnn_amd import GraphConvolution
    n = 350
    low, high, _ = O.filters_linkx(_graph(n, 12))
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, 11, generator=g)
    hs = [torch.randn(n, 24, generator=g) for _ in range(2)]
    gout = torch.randn(n, out_features, generator=g)
    torch.manual_seed(5)
    layer = GraphConvolution(11 + 48, out_features, n, "acmsnowball", variant=bool(variant))
    res = {}
    for form in ("blocks", "cat"):
        layer.zero_grad()
        h = [t.clone().requires_grad_(True) for t in hs]
        out = layer([x] + h if form == "blocks" else torch.cat([x] + h, 1), low, high, None)
        out.backward(gout)
        res[form] = (out.detach(), _grads(layer), [t.grad.clone() for t in h])
    a, b = res["blocks"], res["cat"]
    assert float((a[0] - b[0]).abs().max()) < 3e-5 * max(1.0, float(b[0].abs().max()))
    assert set(a[1]) == set(b[1])
    for k, rg in b[1].items():
        assert float((a[1][k] - rg).abs().max()) < 1e-4 * max(1.0, float(rg.abs().max())), k
    for j, rg in enumerate(b[2]):
        assert float((a[2][j] - rg).abs().max()) < 1e-4 * max(1.0, float(rg.abs().max())), f"h{j}"


@pytest.mark.parametrize("variant", [0, 1])
def test_blocks_equal_the_concatenation_on_relabelled_operators_with_post_scale(variant, monkeypatch):
    """The layer translates at its boundary when the operators are relabelled and the caller is not (rows_permuted=False): the
    blocks, ``post_scale`` and the result are rows of the caller's numbering.  Blocks against their concatenation, both against
    the unrelabelled layer: outputs, parameter gradients and the gradients into h0, h1."""
    fake_lib_blocks.install(monkeypatch)
    from acm_gnn_amd import GraphConvolution, graph, tuning
    n = 350
    low, high, _ = O.filters_linkx(_graph(n, 12))
    g = torch.Generator().manual_seed(3)
    x = torch.randn(n, 11, generator=g)
    hs = [torch.randn(n, 24, generator=g) for _ in range(2)]
    gout = torch.randn(n, 24, generator=g)
    scale = (torch.rand(n, 24, generator=g) < 0.6).float() / 0.6
    torch.manual_seed(5)
    layer = GraphConvolution(11 + 48, 24, n, "acmsnowball", variant=bool(variant))
    res = {}
    for relabel in (0, 1):
        with tuning.override(relabel=relabel):
            graph.clear_cache()
            ops = graph.operators_for(low, high, None)
            assert (ops.perm is not None) == bool(relabel)
            for form in ("blocks", "cat"):
                layer.zero_grad()
                h = [t.clone().requires_grad_(True) for t in hs]
                out = layer([x] + h if form == "blocks" else torch.cat([x] + h, 1), ops, None, None, post_relu=True, post_scale=scale)
                out.backward(gout)
                res[relabel, form] = (out.detach(), _grads(layer), [t.grad.clone() for t in h])
    graph.clear_cache()
    ref = res[0, "cat"]
    assert float((ref[0] * (scale == 0)).abs().max()) == 0.0 and float(ref[0].abs().max()) > 0
    for key in ((0, "blocks"), (1, "blocks"), (1, "cat")):
        a = res[key]
        assert float((a[0] - ref[0]).abs().max()) < 3e-5 * max(1.0, float(ref[0].abs().max())), key
        assert set(a[1]) == set(ref[1])
        for k, rg in ref[1].items():
            assert float((a[1][k] - rg).abs().max()) < 1e-4 * max(1.0, float(rg.abs().max())), (key, k)
        for j, rg in enumerate(ref[2]):
            assert float((a[2][j] - rg).abs().max()) < 1e-4 * max(1.0, float(rg.abs().max())), (key, f"h{j}")


@pytest.mark.parametrize("widths,f,relu", [([24], 24, False), ([24, 24, 24], 7, True), ([6], 4, False), ([68, 8], 5, True)])
@pytest.mark.parametrize("first", ["csr", "dense11", "dense8"])
def test_project_blocks_against_float64(widths, f, relu, first, monkeypatch):
    """functional.project_blocks (kernel route and the composed one for widths the kernels refuse) against the same products in
    float64: Z in the channel-block layout, every dH_j, the three dW."""
    fake_lib_blocks.install(monkeypatch)
    from acm_gnn_amd import functional as AF
    from acm_gnn_amd.graph import SparseFeatures
    n = 37
    g = torch.Generator().manual_seed(11)
    xd = sparse_features(n, 300, 2, density=0.05) if first == "csr" else torch.randn(n, int(first[5:]), generator=g)
    hs = [torch.randn(n, w, generator=g).requires_grad_(True) for w in widths]
    f_in = xd.shape[1] + sum(widths)
    w3 = [torch.randn(f_in, f, generator=g).requires_grad_(True) for _ in range(3)]
    z = AF.project_blocks([SparseFeatures.from_torch(xd) if first == "csr" else xd] + hs, w3, relu=relu)
    fb = AF.blocks._chan_block(f)
    assert tuple(z.shape) == (n, 2 * fb + f)
    gz = torch.randn(n, 3 * f, generator=g)
    zc = torch.cat([z[:, c * fb:c * fb + f] for c in range(3)], 1)
    (zc * gz).sum().backward()
    h64 = [h.detach().double().requires_grad_(True) for h in hs]
    w64 = [w.detach().double().requires_grad_(True) for w in w3]
    ref = torch.cat([xd.double()] + h64, 1) @ torch.cat(w64, 1)
    ref = torch.relu(ref) if relu else ref
    (ref * gz.double()).sum().backward()
    assert float((zc.detach().double() - ref.detach()).abs().max()) < 1e-5 * max(1.0, float(ref.detach().abs().max()))
    if fb != f:
        assert float(z.detach()[:, f:fb].abs().max()) == 0.0 and float(z.detach()[:, fb + f:2 * fb].abs().max()) == 0.0
    for a, b in list(zip(hs, h64)) + list(zip(w3, w64)):
        assert float((a.grad.double() - b.grad).abs().max()) < 1e-5 * max(1.0, float(b.grad.abs().max()))


def test_refusals(monkeypatch):
    """A width sum that does not match in_features, a block on another device, a non-fp32 block, a wrong row count: ValueError
    naming the block; row-sharded operators: NotImplementedError that says so."""
    fake_lib_blocks.install(monkeypatch)
    from acm_gnn_amd import GCN, GraphConvolution
    from acm_gnn_amd.graph import SparseFeatures, operators_for
    n = 60
    low, high, _ = O.filters_linkx(_graph(n, 4, density=0.1))
    layer = GraphConvolution(11 + 24, 8, n, "acmsnowball")
    x, h = torch.randn(n, 11), torch.randn(n, 24)
    with pytest.raises(ValueError, match="block 1"):
        layer([x, torch.randn(n, 20)], low, high, None)
    with pytest.raises(ValueError, match="block 1.*float32"):
        layer([x, h.double()], low, high, None)
    with pytest.raises(ValueError, match="block 1.*meta"):
        layer([x, h.to("meta")], low, high, None)
    with pytest.raises(ValueError, match="block 1.*rows"):
        layer([x, torch.randn(n - 1, 24)], low, high, None)
    with pytest.raises(ValueError, match="block 1"):
        layer([x, SparseFeatures.from_torch(h)], low, high, None)
    ops = operators_for(low, high, None)
    monkeypatch.setattr(type(ops), "sharded", property(lambda self: True))
    with pytest.raises(NotImplementedError, match="row-sharded"):
        layer([x, h], ops, None, None)
    model = GCN(300, 8, 3, 2, n, 0.0, "acmsnowball", 0)
    with pytest.raises(NotImplementedError, match="row-sharded"):
        model(SparseFeatures.from_torch(sparse_features(n, 300, 1)), ops, None, None)


def _train(monkeypatch, p_drop, steps, lr, relabel, tape=True):
    from acm_gnn_amd import GCN, FusedAdam, graph, train as T, tuning
    from acm_gnn_amd.graph import SparseFeatures
    n = 120
    low, high, _ = O.filters_linkx(_graph(n, 12, density=0.08))
    x = sparse_features(n, 300, 6)
    y = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(6))
    with tuning.override(relabel=relabel):
        graph.clear_cache()
        torch.manual_seed(8)
        model = GCN(300, 24, 4, 2, n, p_drop, "acmsnowball", 0)
        opt = FusedAdam(model.parameters(), lr=lr)
        step = T.TrainStep(model, opt, SparseFeatures.from_torch(x), low, y, T.row_weights(torch.arange(1, n, 2), n), high, None, tape=tape)
        assert step._permuted == bool(relabel) and isinstance(step.x, SparseFeatures)
        losses = [float(step()) for _ in range(steps)]
    graph.clear_cache()
    return losses, step


def test_training_step_and_fit_on_the_double(monkeypatch):
    """train.TrainStep on a snowball model handed SparseFeatures: the step's own tape carries the hidden blocks that several
    Functions consume (same losses as on autograd), fused dropout on the stored values, relabelled operators
    (x.permute_rows) within 1e-6 of the unpermuted loss, and fit() over five epochs."""
    fake_lib_blocks.install(monkeypatch)
    from acm_gnn_amd import GCN, FusedAdam, train as T
    from acm_gnn_amd.graph import SparseFeatures
    taped, step = _train(monkeypatch, 0.35, 4, 0.01, 0)
    assert step._tape and step._tape_proven and step.model.fused_dropout
    auto, step = _train(monkeypatch, 0.35, 4, 0.01, 0, tape=False)
    assert all(np.isfinite(taped)) and len(set(taped)) == 4
    np.testing.assert_allclose(taped, auto, rtol=1e-6)
    plain, sp_ = _train(monkeypatch, 0.0, 1, 0.0, 0)
    relabelled, sr = _train(monkeypatch, 0.0, 1, 0.0, 1)
    assert abs(plain[0] - relabelled[0]) < 1e-6, (plain, relabelled)
    for (k, a), (_, b) in zip(sp_.model.named_parameters(), sr.model.named_parameters()):      # the permuted backward
        assert (a.grad is None) == (b.grad is None), k
        if a.grad is not None:
            assert float((a.grad - b.grad).abs().max()) < 1e-4 * max(1.0, float(a.grad.abs().max())), k
    n = 120
    low, high, _ = O.filters_linkx(_graph(n, 12, density=0.08))
    y = torch.randint(0, 4, (n,), generator=torch.Generator().manual_seed(6))
    torch.manual_seed(8)
    model = GCN(300, 24, 4, 2, n, 0.35, "acmsnowball", 0)
    sets = [torch.arange(1, n, 2), torch.arange(0, n, 4), torch.arange(2, n, 4)]
    sel, hist = T.fit(model, FusedAdam(model.parameters(), lr=0.01), SparseFeatures.from_torch(sparse_features(n, 300, 6)), low, y, *sets,
                      epochs=5, adj_high=high)
    assert len(hist) == 5 and np.isfinite(np.asarray(hist, dtype=np.float64)).all() and np.isfinite(sel)


def test_library_exports_the_new_symbols_and_keeps_its_abi_number():
    import ctypes as C
    from acm_gnn_amd import _lib, build
    lib = _lib.load()
    assert lib.acm_version() == 29 == _lib.ABI_VERSION
    for name in ("acm_proj_blocks_fwd", "acm_proj_blocks_bwd_workspace_bytes", "acm_proj_blocks_bwd"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert "acm_proj_blocks.hip" in build.SOURCES
    w = (C.c_float * 64)()
    p = _lib.ProjBlocks()
    p.n_blocks, p.f, p.f_block, p.f_in, p.ldw = 1, 24, 24, 400, 24
    p.w_low = p.w_high = p.w_mlp = C.addressof(w)
    p.h[0], p.ld_h[0], p.width[0], p.row0[0] = C.addressof(w), 128, 24, 300
    nbytes = C.c_size_t()
    assert lib.acm_proj_blocks_bwd_workspace_bytes(350, C.byref(p), C.byref(nbytes)) == 0
    assert nbytes.value == 6 * (24 * 72) * 4                 # ceil(350 / 64) slabs of 24 x 72 floats (a multiple of 32)
    for width in (6, 68):                                    # outside the envelope: ACM_EUNSUPPORTED from every entry point
        p.width[0] = width
        assert lib.acm_proj_blocks_bwd_workspace_bytes(350, C.byref(p), C.byref(nbytes)) == 4
        assert lib.acm_proj_blocks_fwd(350, C.byref(p), C.addressof(w), 72, 0, 0, None) == 4
    p.width[0], p.row0[0] = 24, 377                          # rows beyond the weights: ACM_ESHAPE, nothing is touched
    assert lib.acm_proj_blocks_fwd(350, C.byref(p), C.addressof(w), 72, 0, 0, None) == 2
    assert lib.acm_proj_blocks_bwd_workspace_bytes(350, C.byref(p), C.byref(nbytes)) == 2
    p.row0[0], p.f, p.f_block, p.ldw = 300, 65, 65, 65
    assert lib.acm_proj_blocks_fwd(350, C.byref(p), C.addressof(w), 195, 0, 0, None) == 4
    assert lib.acm_proj_blocks_fwd(350, None, C.addressof(w), 72, 0, 0, None) == 1          # ACM_EINVAL
