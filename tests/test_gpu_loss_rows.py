"""The output layer over the loss rows alone (acm_csr_build_loss_rows, acm_conv_fwd_tail_rows) against the full entry point on
the same inputs, each followed by the same acm_conv_bwd_spmm: EQUAL under torch.equal, not close.  Every kept row keeps its
work items, pieces and order of summation, and what is left out are terms that were zeros (x + 0 = x in fp32; only the sign
of a zero may differ, which torch.equal does not see)."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CHUNK = 128
_GRAPHS = {}


def _graph(kind):
    """Symmetric pattern with self loops, heavy-tailed degrees, mean about 40, n no multiple of 64: "tail" = 3 000 rows (several
    rows of more than CHUNK neighbours: pieces that meet in LDS), "hub" = 12 288 + 1 rows one of which has 9 000 neighbours
    (more than 64 x CHUNK: several windows and the second launch that adds them).  Made once per kind, never modified."""
    if kind in _GRAPHS:
        return _GRAPHS[kind]
    n = 3000 if kind == "tail" else 12289
    rng = np.random.default_rng(7 if kind == "tail" else 11)
    m = n * 20
    w = 1.0 / (np.arange(n) + 4.0) ** 0.75
    r, c = rng.choice(n, m, p=w / w.sum()), rng.integers(0, n, m)
    if kind == "hub":
        hub = np.full(9000, 5, np.int64)
        r, c = np.concatenate([r, hub]), np.concatenate([c, rng.choice(n, 9000, replace=False)])
    adj = sp.csr_matrix((np.ones(r.size, np.float32), (r, c)), shape=(n, n))
    adj = ((adj + adj.T + sp.identity(n, dtype=np.float32, format="csr")) > 0).astype(np.float32).tocsr()
    adj.sort_indices()
    deg = np.asarray(adj.sum(1)).reshape(-1)
    assert n % 64 and 30 < adj.nnz / n < 60 and (deg > CHUNK).sum() >= 3
    assert (deg.max() > 64 * CHUNK) == (kind == "hub")
    # a row all of whose neighbours (itself included) can be dropped while it is kept makes no sense with a self loop: take
    # the self loop out of ONE short row, so that "a kept row all of whose neighbours are dropped" exists
    lone = int(np.argmin(deg + (deg < 3) * 10 ** 6))
    adj = adj.tolil()
    adj[lone, lone] = 0
    adj = adj.tocsr()
    adj.eliminate_zeros()
    adj.sort_indices()
    _GRAPHS[kind] = (adj, lone, int(np.argmax(deg)))
    return _GRAPHS[kind]


def _handles(adj, implicit):
    """(handle the forward walks, handle the backward walks, row_scale or None) with CHUNK neighbours per work item."""
    from acm_gnn_amd.graph import CsrGraph
    n = adj.shape[0]
    ip = torch.from_numpy(adj.indptr.astype(np.int32)).to(DEV)
    ix = torch.from_numpy(adj.indices.astype(np.int32)).to(DEV)
    inv = torch.from_numpy((1.0 / np.asarray(adj.sum(1)).reshape(-1)).astype(np.float32)).to(DEV)
    if implicit:
        g = CsrGraph.from_csr(ip, ix, None, n, chunk=CHUNK)
        return g, g, inv
    vals = inv[torch.repeat_interleave(torch.arange(n, device=DEV), (ip[1:] - ip[:-1]).long())]
    g = CsrGraph.from_csr(ip, ix, vals, n, chunk=CHUNK)
    return g, g.transpose(), None


def _mask(kind, adj, lone, hub, seed=0):
    n = adj.shape[0]
    rng = np.random.default_rng(seed)
    keep = rng.random(n) < 0.5
    if kind == "all":
        keep[:] = True
    elif kind == "none":
        keep[:] = False
    elif kind == "hub_kept":
        keep[hub] = True
    elif kind == "hub_dropped":
        keep[hub] = False
    elif kind == "lone":                         # a kept row all of whose neighbours are dropped
        keep[lone] = True
        keep[adj.indices[adj.indptr[lone]:adj.indptr[lone + 1]]] = False
        assert keep[lone]
    return keep


class _Layer:
    """The inputs of one output layer (three channels, f classes) in the package's layout -- [Z_L | Z_H] and [G_L | G_H] as
    channel blocks of fb columns -- or, ``aligned=False``, as 2 f unpadded columns (f = 3: rows the vector fetch cannot take)."""

    def __init__(self, n, f, layernorm, aligned=True, seed=0):
        g = torch.Generator().manual_seed(100 + seed)
        self.n, self.f = n, f
        self.fb = (2 if f <= 2 else 4) if aligned else f
        self.layernorm = layernorm
        r = lambda *s: torch.randn(*s, generator=g).to(DEV)      # noqa: E731
        self.zlh = torch.zeros(n, 2 * self.fb, device=DEV)
        self.zlh[:, :f], self.zlh[:, self.fb:self.fb + f] = r(n, f), r(n, f)
        self.zi = r(n, f)
        self.vec, self.lnw, self.lnb = [r(f) for _ in range(3)], [1 + 0.1 * r(f) for _ in range(3)], [0.1 * r(f) for _ in range(3)]
        self.mix = r(3, 3).contiguous()
        self.y = torch.randint(0, f, (n,), generator=g).to(DEV)


def _run(layer, fwd_h, bwd_h, row_scale, weights, rows):
    """acm_conv_fwd_tail[_rows] then acm_conv_bwd_spmm on fresh NaN-filled outputs; everything the two calls write."""
    from acm_gnn_amd import _lib
    from acm_gnn_amd.graph import _stream
    lib = _lib.load()
    n, f, fb, k = layer.n, layer.f, layer.fb, 3
    nan = lambda *s: torch.full(s, float("nan"), device=DEV)      # noqa: E731
    out, att, pre, dlog = nan(n, f), nan(n, 4), nan(n, 2 * f), nan(n, f)
    gtab, dz, loss = nan(n, 2 * fb), nan(n, 3 * f), nan(1)
    d_vec, d_lnw, d_lnb, d_mix = [nan(f) for _ in range(3)], [nan(f) for _ in range(3)], [nan(f) for _ in range(3)], nan(9)
    arr = lambda ts: (C.c_void_p * 4)(*[t.data_ptr() for t in ts], None)      # noqa: E731

    p = _lib.ConvFwd()
    p.f_out, p.n_channels, p.relu_after, p.relu_mlp, p.layernorm, p.scale = f, k, 0, 0, int(layer.layernorm), 3.0
    p.g_low, p.ld_g_low = layer.zlh.data_ptr(), 2 * fb
    p.g_high, p.ld_g_high = layer.zlh.data_ptr() + 4 * fb, 2 * fb
    p.s_high, p.ld_s_high = layer.zlh.data_ptr() + 4 * fb, 2 * fb
    p.s_mlp, p.ld_s_mlp = layer.zi.data_ptr(), f
    p.att_vec, p.ln_weight, p.ln_bias, p.att_mix = arr(layer.vec), arr(layer.lnw), arr(layer.lnb), layer.mix.data_ptr()
    p.out, p.ld_out, p.pre, p.ld_pre, p.att = out.data_ptr(), f, pre.data_ptr(), 2 * f, att.data_ptr()
    if row_scale is not None:
        p.row_scale = row_scale.data_ptr()
    lo = _lib.Loss()
    lo.n_classes, lo.labels, lo.row_weight = f, layer.y.data_ptr(), weights.data_ptr()
    lo.loss, lo.dlogits, lo.ld_dlogits = loss.data_ptr(), dlog.data_ptr(), f
    q = _lib.ConvBwdLocal()
    q.f_out, q.n_channels, q.relu_after, q.relu_mlp, q.layernorm, q.scale = f, k, 0, 0, int(layer.layernorm), 3.0
    q.grad_out, q.ld_grad_out, q.pre, q.ld_pre, q.s_mlp, q.ld_s_mlp = dlog.data_ptr(), f, pre.data_ptr(), 2 * f, layer.zi.data_ptr(), f
    q.att_vec, q.ln_weight, q.ln_bias, q.att_mix = arr(layer.vec), arr(layer.lnw), arr(layer.lnb), layer.mix.data_ptr()
    q.g_low, q.ld_g_low, q.g_high, q.ld_g_high = gtab.data_ptr(), 2 * fb, gtab.data_ptr() + 4 * fb, 2 * fb
    q.g_mlp, q.ld_g_mlp = dz.data_ptr() + 8 * f, 3 * f
    q.d_att_vec, q.d_ln_weight, q.d_ln_bias, q.d_att_mix = arr(d_vec), arr(d_lnw), arr(d_lnb), d_mix.data_ptr()
    if row_scale is not None:
        q.g_scale = row_scale.data_ptr()
    self_scale = (1.0 / row_scale) if row_scale is not None else None
    r = _lib.ConvBwdSpmm()
    r.f_out = f
    r.g_low, r.ld_g_low, r.g_high, r.ld_g_high = gtab.data_ptr(), 2 * fb, gtab.data_ptr() + 4 * fb, 2 * fb
    r.s_high, r.ld_s_high = gtab.data_ptr() + 4 * fb, 2 * fb
    r.dz_low, r.ld_dz_low, r.dz_high, r.ld_dz_high = dz.data_ptr(), 3 * f, dz.data_ptr() + 4 * f, 3 * f
    if self_scale is not None:
        r.self_scale = self_scale.data_ptr()

    nb = C.c_size_t()
    _lib.check(lib.acm_conv_fwd_tail_workspace_bytes(n, f, k, C.byref(nb)), "tail workspace")
    wt = torch.empty(max(nb.value // 4, 1), device=DEV)
    slots = max(fwd_h.n_partial_slots, bwd_h.n_partial_slots) + 64
    if rows:
        info = (C.c_int64 * 4)()
        _lib.check(lib.acm_csr_loss_rows_info(fwd_h.handle, info), "info")
        slots = max(slots, int(info[2]))
    ws = torch.empty(max(slots * 2 * f, 1), device=DEV)
    fwd = lib.acm_conv_fwd_tail_rows if rows else lib.acm_conv_fwd_tail
    bwd = lib.acm_conv_bwd_spmm
    st_f = fwd(fwd_h.handle, C.byref(p), C.byref(lo), C.byref(q), ws.data_ptr(), ws.numel() * 4, wt.data_ptr(), nb.value, _stream())
    if st_f:
        return st_f
    _lib.check(bwd(bwd_h.handle, C.byref(r), ws.data_ptr(), ws.numel() * 4, _stream()), "bwd_spmm")
    torch.cuda.synchronize()
    return dict(loss=loss, dlogits=dlog, dz=dz, out=out, att=att, pre=pre, d_mix=d_mix,
                **{f"d_vec{c}": d_vec[c] for c in range(3)}, **{f"d_lnw{c}": d_lnw[c] for c in range(3)},
                **{f"d_lnb{c}": d_lnb[c] for c in range(3)})


def _compare(full, rows, keep_t, layernorm):
    kept = keep_t.bool()
    for name in ("loss", "dlogits", "dz", "d_mix", "d_vec0", "d_vec1", "d_vec2") + \
            (("d_lnw0", "d_lnw1", "d_lnw2", "d_lnb0", "d_lnb1", "d_lnb2") if layernorm else ()):
        assert not torch.isnan(rows[name]).any(), name
        assert torch.equal(full[name], rows[name]), (name, float((full[name] - rows[name]).abs().max()))
    for name in ("out", "att", "pre"):
        assert torch.equal(full[name][kept], rows[name][kept]), name
    assert not rows["out"][~kept].any() and not rows["att"][~kept].any() and not rows["dlogits"][~kept].any()


@pytest.mark.parametrize("implicit", [True, False], ids=["implicit", "explicit"])
@pytest.mark.parametrize("f,aligned", [(2, True), (3, True), (3, False)], ids=["f2", "f3", "f3-unaligned"])
def test_entry_points_equal_their_full_counterparts_bit_for_bit(implicit, f, aligned):
    """"explicit": the operator with a value stream (the gather multiplies by vals[k], no row scale in the epilogues) and a
    transposed handle of its own for the unchanged backward; "implicit": the pattern-only operator, one handle both ways."""
    adj, lone, hub = _graph("tail")
    fwd_h, bwd_h, row_scale = _handles(adj, implicit)
    assert fwd_h.chunk == CHUNK and fwd_h.n_long_rows >= 3 and bwd_h.n_long_rows >= 3
    n = adj.shape[0]
    layer = _Layer(n, f, layernorm=(f == 2), aligned=aligned, seed=f)
    for kind in ("half", "all", "none", "lone"):
        keep = _mask(kind, adj, lone, hub, seed=3)
        keep_t = torch.from_numpy(keep.astype(np.uint8)).to(DEV)
        weights = torch.where(keep_t.bool(), torch.rand(n, device=DEV) + 0.5, torch.zeros(n, device=DEV)) / max(int(keep.sum()), 1)
        full = _run(layer, fwd_h, bwd_h, row_scale, weights, rows=False)
        i_f = fwd_h.build_loss_rows(keep_t)
        assert i_f["kept_rows"] == int(keep.sum()) and i_f["kept_edges"] == int(np.diff(adj.indptr)[keep].sum())
        rows = _run(layer, fwd_h, bwd_h, row_scale, weights, rows=True)
        assert isinstance(rows, dict), f"status {rows}"
        _compare(full, rows, keep_t, layer.layernorm)
        if kind == "none":
            assert float(rows["loss"]) == 0.0 and not rows["dz"].any() and not rows["d_mix"].any() and not rows["d_vec0"].any()
        if kind == "lone":
            assert rows["out"][lone].any()                       # the kept row is finished from its own terms


@pytest.mark.parametrize("kind", ["hub_kept", "hub_dropped"])
def test_a_row_of_several_windows_kept_or_dropped(kind):
    """12 289 rows, one of 9 000 neighbours (> 64 x chunk): its pieces fill whole windows and spmm_fixup_windows_kernel adds
    them -- over the row list's own slots."""
    adj, lone, hub = _graph("hub")
    fwd_h, bwd_h, row_scale = _handles(adj, True)
    n = adj.shape[0]
    assert fwd_h.max_degree > 64 * CHUNK
    layer = _Layer(n, 2, layernorm=True, seed=9)
    keep = _mask(kind, adj, lone, hub, seed=5)
    keep_t = torch.from_numpy(keep.astype(np.uint8)).to(DEV)
    weights = keep_t.float() / float(keep.sum())
    full = _run(layer, fwd_h, bwd_h, row_scale, weights, rows=False)
    fwd_h.build_loss_rows(keep_t)
    rows = _run(layer, fwd_h, bwd_h, row_scale, weights, rows=True)
    assert isinstance(rows, dict), f"status {rows}"
    _compare(full, rows, keep_t, True)
    assert rows["dz"][hub].any()                                 # (the hub has kept neighbours either way)


def test_five_classes_are_unsupported_and_the_step_takes_the_full_path(monkeypatch):
    from acm_gnn_amd import FusedAdamW, GCN, data as D, train as T, tuning
    from acm_gnn_amd.distributed import make_sharded_operators
    adj, lone, hub = _graph("tail")
    fwd_h, bwd_h, row_scale = _handles(adj, True)
    n = adj.shape[0]
    keep_t = torch.from_numpy(_mask("half", adj, lone, hub).astype(np.uint8)).to(DEV)
    fwd_h.build_loss_rows(keep_t)
    layer = _Layer(n, 5, layernorm=False, aligned=False)
    layer.fb = 8
    layer.zlh = torch.randn(n, 16, device=DEV)
    assert _run(layer, fwd_h, bwd_h, row_scale, keep_t.float(), rows=True) == 4          # ACM_EUNSUPPORTED
    # ... and a five-class TrainStep builds the attachment, never calls a _rows entry point, and trains like the full path
    names = []
    import acm_gnn_amd.functional.conv_literal as CL
    real = CL.launch
    monkeypatch.setattr(CL, "launch", lambda name, *a, **kw: (names.append(name), real(name, *a, **kw))[1])
    pat = adj.copy()
    pat.setdiag(0)
    pat.eliminate_zeros()
    low, deg = D.build_filters(pat)
    losses = {}
    for switch in (1, 0):
        with tuning.override(loss_rows=switch):
            ops = make_sharded_operators(low, deg, DEV)
            torch.manual_seed(0)
            model = GCN(7, 64, 5, 2, n, 0.0, "acmgcnp", 0).to(DEV)
            g = torch.Generator().manual_seed(1)
            x, y = torch.randn(n, 7, generator=g).to(DEV), torch.randint(0, 5, (n,), generator=g).to(DEV)
            w = T.row_weights(torch.arange(0, n, 2, device=DEV), n)
            step = T.TrainStep(model, FusedAdamW(model.parameters(), lr=0.01), x, ops, y, w)
            assert (step.loss_rows is not None) == bool(switch)
            losses[switch] = [float(step()) for _ in range(3)]
    assert "acm_conv_bwd_spmm" in names and not any(nm.endswith("_rows") for nm in names), sorted(set(names))
    assert losses[1] == losses[0]


@pytest.fixture(scope="module")
def step_case():
    """9 000 rows, mean degree about 40, relabelled operators, 7 dense input features: the headline's step in small."""
    from acm_gnn_amd import data as D, tuning
    from acm_gnn_amd.distributed import make_sharded_operators
    n = 9000
    rng = np.random.default_rng(21)
    m = n * 20
    w = 1.0 / (np.arange(n) + 10.0) ** 0.6
    r, c = rng.choice(n, m, p=w / w.sum()), rng.integers(0, n, m)
    adj = sp.csr_matrix((np.ones(m, np.float32), (r, c)), shape=(n, n))
    adj = ((adj + adj.T) > 0).astype(np.float32).tocsr()
    adj.setdiag(0)
    adj.eliminate_zeros()
    low, deg = D.build_filters(adj)
    g = torch.Generator().manual_seed(2)
    x, y = torch.randn(n, 7, generator=g).to(DEV), torch.randint(0, 2, (n,), generator=g).to(DEV)
    train_idx = torch.randperm(n, generator=g)[: n // 2].to(DEV)

    def ops():
        with tuning.override(relabel=1):
            return make_sharded_operators(low, deg, DEV, relabel=True)
    return ops, x, y, train_idx, n


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_train_step_with_loss_rows_equals_the_full_step_bit_for_bit(step_case, use_graph, monkeypatch):
    """Five steps (eager, or captured and replayed) with the attachment against five without: the same losses and the same
    parameters, bit for bit -- and the step with it really ran the _rows entry point, under today's launch label."""
    import acm_gnn_amd.functional.conv_literal as CL
    from acm_gnn_amd import FusedAdamW, GCN, functional as AF, train as T, tuning
    make_ops, x, y, train_idx, n = step_case
    names, real = {1: [], 0: []}, CL.launch
    got = {}
    for switch in (1, 0):
        monkeypatch.setattr(CL, "launch", lambda name, label, *a, _s=switch, **kw: (names[_s].append((name, label)), real(name, label, *a, **kw))[1])
        with tuning.override(relabel=1, loss_rows=switch):
            ops = make_ops()
            torch.manual_seed(0)
            model = GCN(7, 64, 2, 2, n, 0.1, "acmgcnp", 0).to(DEV)
            model.dropout_state = AF.DropoutState(DEV, seed=5)
            w = T.row_weights(train_idx, n)
            step = T.TrainStep(model, FusedAdamW(model.parameters(), lr=0.01, weight_decay=1e-3), x, ops, y, w, use_graph=use_graph)
            assert step.pipe is not None and step.small is None and ops.perm is not None
            if switch:
                assert step.loss_rows, step.loss_rows_refused
                assert step.loss_rows.fwd["kept_rows"] == n // 2
            else:
                assert step.loss_rows is None and "loss_rows=0" in step.loss_rows_refused
            losses = [float(step()) for _ in range(5)]
            got[switch] = (losses, [p.detach().clone() for p in model.parameters()])
    assert ("acm_conv_fwd_tail_rows", "conv_fwd_tail/F2k3") in names[1] and ("acm_conv_bwd_spmm", "conv_bwd_spmm/F2k3") in names[1]
    assert not any(nm == "acm_conv_fwd_tail" for nm, _ in names[1]), sorted(set(names[1]))
    assert ("acm_conv_fwd_tail", "conv_fwd_tail/F2k3") in names[0] and not any(nm.endswith("_rows") for nm, _ in names[0])
    assert np.isfinite(got[1][0]).all() and got[1][0] == got[0][0], (got[1][0], got[0][0])
    for a, b in zip(got[1][1], got[0][1]):
        assert torch.equal(a, b)
