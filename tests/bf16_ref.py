"""References for the bf16 gather path that read THE SAME bf16 TABLES the kernels read (tests/test_gpu_bf16_exact.py on the
device, tests/test_bf16_ref_cpu.py against tests/fake_lib.py): a table is widened exactly (bits << 16) and every product is
taken in fp64, so the rounding of the operand drops out of the error and the fp32 tolerances of the neighbouring tests apply.
Importable without a GPU; every runner takes the device it works on."""
import ctypes as C
import json
import os

import numpy as np
import scipy.sparse as sp
import torch

# ---- the cast ----
LOW_HALVES = (0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF)


def cast_patterns():
    """Every high half-word with six low half-words: 393 216 fp32 bit patterns (every exponent, both signs, denormals, the
    ties and their neighbours, the largest finite's overflow to inf, +-0, +-inf, every NaN prefix)."""
    hi = np.arange(65536, dtype=np.uint32) << 16
    return (hi[:, None] | np.array(LOW_HALVES, np.uint32)[None, :]).reshape(-1)


def f32_from_bits(bits):
    return torch.from_numpy(np.ascontiguousarray(bits, dtype=np.uint32).view(np.float32).copy())


def bits_bf16(t):
    return t.detach().cpu().contiguous().view(torch.int16).numpy().view(np.uint16)


def bits_f32(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32)


def widen(t):
    """bf16 tensor -> float64 array, exactly."""
    return (bits_bf16(t).astype(np.uint32) << 16).view(np.float32).astype(np.float64)


def cast_mismatches(src, dst):
    """(source bits, got, wanted) of every element of ``dst`` (bf16) that is not the rounding of ``src`` (fp32): a non-NaN input
    must be bit-equal to torch's CPU conversion, a NaN input must give a NaN of the same sign."""
    s, g = bits_f32(src).reshape(-1), bits_bf16(dst).reshape(-1)
    w = bits_bf16(src.detach().cpu().to(torch.bfloat16)).reshape(-1)
    assert s.shape == g.shape
    nan = (s & 0x7FFFFFFF) > 0x7F800000
    ok = np.where(nan, ((g & 0x7FFF) > 0x7F80) & ((g >> 15) == (s >> 31)), g == w)
    bad = np.nonzero(~ok)[0]
    return [(hex(int(s[i])), hex(int(g[i])), hex(int(w[i]))) for i in bad]


# ---- worst error / tolerance per part ----
RATIOS = {}


def note(part, err, tol):
    r = float(err) / float(tol)
    RATIOS[part] = max(RATIOS.get(part, 0.0), r)
    return r


def dump_ratios():
    """Write the ratios as bf16_exact.json into the directory ACM_EVIDENCE_DIR names (the run that collects profiles/ sets it);
    without it nothing is written."""
    out_dir = os.environ.get("ACM_EVIDENCE_DIR")
    if not out_dir:
        return
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, "bf16_exact.json"), "w") as fh:
        json.dump({"worst_error_over_tolerance": RATIOS}, fh, indent=1, sort_keys=True)


# ---- the operators ----
LADDER = (0, 1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 200)


class Operator:
    """CSR arrays of a test operator (``vals`` None: pattern-only), the chunk its work list is built with, the columns no stored
    entry references (``dead``: their table rows may hold anything) and the shape figures the tests pin."""

    def __init__(self, name, indptr, indices, vals, n_cols, chunk):
        self.name, self.chunk, self.n_cols = name, chunk, int(n_cols)
        self.indptr, self.indices = indptr.astype(np.int32), indices.astype(np.int32)
        self.vals = None if vals is None else vals.astype(np.float32)
        self.n_rows = len(indptr) - 1
        self.lengths = np.diff(self.indptr)
        self.dead = np.setdiff1d(np.arange(self.n_cols), self.indices)

    def matrix(self):
        """float64 scipy CSR; repeated columns add up in a product, as they do in the kernels."""
        v = np.ones(len(self.indices)) if self.vals is None else self.vals.astype(np.float64)
        return sp.csr_matrix((v, self.indices.copy(), self.indptr.copy()), shape=(self.n_rows, self.n_cols))   # (scipy edits in place)

    def unit(self):
        """Pattern-only twin with the first stored column of every non-empty row repeated (the multigraph encoding of a raw
        self-loop)."""
        rep = np.ones(len(self.indices), np.int64)
        rep[self.indptr[:-1][self.lengths > 0]] = 2
        per_row = self.lengths + (self.lengths > 0)
        ip = np.concatenate([[0], np.cumsum(per_row)])
        return Operator(self.name + "-unit", ip, np.repeat(self.indices, rep), None, self.n_cols, self.chunk)

    def transposed(self):
        m = self.matrix()
        if self.vals is None:                       # keep the multiplicities as repeated entries
            rows = np.repeat(np.arange(self.n_rows), self.lengths)
            order = np.lexsort((rows, self.indices))
            cols_t, rows_t = self.indices[order], rows[order]
            ip = np.concatenate([[0], np.cumsum(np.bincount(cols_t, minlength=self.n_cols))])
            return Operator(self.name + "-T", ip, rows_t, None, self.n_rows, self.chunk)
        t = sp.csr_matrix(m.T)
        t.sort_indices()
        assert t.nnz == m.nnz                       # (no stored zero was dropped)
        return Operator(self.name + "-T", t.indptr, t.indices, t.data, self.n_rows, self.chunk)

    def handle(self, dev):
        from acm_gnn_amd.graph import CsrGraph
        dev = torch.device(dev)
        return CsrGraph.from_csr(torch.from_numpy(self.indptr).to(dev), torch.from_numpy(self.indices).to(dev),
                                 None if self.vals is None else torch.from_numpy(self.vals).to(dev), self.n_cols, chunk=self.chunk)

    def check_shape(self, g):
        """The figures the neighbouring tests pin, so that the shapes cannot drift."""
        assert g.chunk == self.chunk and (g.n_rows, g.n_cols, g.nnz) == (self.n_rows, self.n_cols, len(self.indices)), g
        assert g.max_degree == int(self.lengths.max()), (g, int(self.lengths.max()))
        assert g.n_long_rows == int((self.lengths > self.chunk).sum()), (g, int((self.lengths > self.chunk).sum()))
        assert g.n_partial_slots % 16 == 0 and (g.n_long_rows == 0) == (g.n_partial_slots == 0), g


def _random_values(rng, nnz):
    """+-U(0.25, 1.5): no stored zero (a kernel may skip one)."""
    return (rng.uniform(0.25, 1.5, nnz) * rng.choice([-1.0, 1.0], nnz)).astype(np.float32)


def ladder_operator(chunk=16, name="ladder"):
    """Operator (a): 333 x 333, chunk 16.  The first rows' lengths are the ladder -- the edges of the 64-id batch, the pair
    kernel's odd last neighbour, the vector kernel's step of four, the unroll of 2 / 4 / 8 steps -- the rest are short random
    rows; every row above 16 neighbours is a split long row.  Columns 0, 100 and 332 are never referenced.
    (``chunk=256``: the same operator with every row ONE work item -- chunk 16 cuts the rows into items of at most 16 neighbours,
    so only there does a wave walk 63 / 64 / 65 / 129 / 200 ids and cross the 64-id batch.)"""
    n = 333
    rng = np.random.default_rng(5)
    lens = np.concatenate([LADDER, rng.integers(1, 13, n - len(LADDER))])
    live = np.setdiff1d(np.arange(n), [0, 100, n - 1])
    cols = [np.sort(rng.choice(live, int(k), replace=False)) for k in lens]
    indices = np.concatenate(cols)
    op = Operator(name, np.concatenate([[0], np.cumsum(lens)]), indices, _random_values(rng, len(indices)), n, chunk)
    assert set(op.dead) >= {0, 100, n - 1}
    return op


def hub_operator():
    """Operator (b): the low-pass pattern of the 700-node graph of test_gpu_oracle._graph(700, 31, 0.04, hub=True) with chunk 8
    (its hub takes three windows of pieces), the column ids shifted by one in a 700 x 702 operator so that table rows 0 and 701
    are never referenced; explicit random values."""
    from test_gpu_oracle import _graph
    adj = _graph(700, 31, density=0.04, hub=True)
    pat = sp.csr_matrix(sp.identity(700) + adj)
    pat.sort_indices()
    rng = np.random.default_rng(6)
    op = Operator("hub", pat.indptr, pat.indices + 1, _random_values(rng, pat.nnz), 702, 8)
    assert int(op.lengths.max()) >= 699 and set(op.dead) == {0, 701}
    return op


_OPS = {}


def operators():
    """name -> Operator: both operators, both value kinds, and the transposes of all four."""
    if not _OPS:
        for base in (ladder_operator(), hub_operator()):
            for op in (base, base.unit()):
                _OPS[op.name] = op
                t = op.transposed()
                _OPS[t.name] = t
        _OPS["ladder-whole"] = ladder_operator(256, "ladder-whole")
    return _OPS


BASE_OPS = ("ladder", "ladder-unit", "hub", "hub-unit")
FORWARD_OPS = BASE_OPS + ("ladder-whole",)
TRANSPOSED_OPS = tuple(nm + "-T" for nm in BASE_OPS) + ("ladder-whole",)     # (square: K4 walks it like any transposed operator)
_HANDLES = {}


def handle_of(name, dev):
    """The device handle of an operator, built once per device and checked against the operator's figures."""
    key = (name, str(dev))
    if key not in _HANDLES:
        op = operators()[name]
        g = op.handle(dev)
        op.check_shape(g)
        if name.startswith("hub") and not name.endswith("-T"):
            assert g.n_items >= 700 + 48 - 1, g            # the hub alone: 48 pieces in 3 windows
        _HANDLES[key] = g
    return _HANDLES[key]


def forget_handles():
    _HANDLES.clear()


def _stream():
    from acm_gnn_amd import graph
    return graph._stream()


NONFINITE = (float("nan"), float("inf"), float("-inf"))


def bf16_table(values, ld, dead, dev):
    """The bf16 table [rows, ld] of an fp32 array through functional.cast_bf16 (the rounding the layers apply): the pad columns
    beyond the width and the rows in ``dead`` hold NaN / +-inf.  Returns (the table, its widened fp64 values with the dead rows
    zeroed)."""
    from acm_gnn_amd.functional import cast_bf16
    rows, width = values.shape
    tb = cast_bf16(torch.from_numpy(values).to(dev))
    table = torch.full((rows, ld), float("nan"), dtype=torch.bfloat16, device=dev)
    table[:, :width] = tb
    for i, r in enumerate(dead):
        table[int(r), :] = NONFINITE[i % 3]
    ref = widen(table[:, :width])
    ref[np.asarray(dead, dtype=np.int64)] = 0.0
    return table, ref


# ---- part 2: acm_spmm_ex ----
def run_spmm_ex(name, width, ld, full, dev, seed=0):
    """One acm_spmm_ex call with a bf16 operand of pitch ``ld`` over operator ``name``: plain, or (``full``) with
    row_scale + sub + sub_scale + relu; the output starts as NaN (every row must be written).  Returns (error, tolerance)."""
    from acm_gnn_amd import _lib
    op, g = operators()[name], handle_of(name, dev)
    rng = np.random.default_rng(seed + width)
    table, t64 = bf16_table(rng.standard_normal((op.n_cols, width)).astype(np.float32), ld, op.dead, dev)
    assert table.data_ptr() % 4 == 0 and ld % 2 == 0 and table.shape == (op.n_cols, ld)
    sub = rng.standard_normal((op.n_rows, width)).astype(np.float32)
    rs = rng.uniform(0.1, 2.0, op.n_rows).astype(np.float32)
    ss = rng.uniform(0.1, 2.0, op.n_rows).astype(np.float32)
    sub_d, rs_d, ss_d = (torch.from_numpy(t).to(dev) for t in (sub, rs, ss))
    o = _lib.SpmmOpts()
    o.g_bf16 = 1
    if full:
        o.row_scale, o.sub, o.ld_sub, o.sub_scale, o.relu = rs_d.data_ptr(), sub_d.data_ptr(), width, ss_d.data_ptr(), 1
    y = torch.full((op.n_rows, width), float("nan"), device=dev)
    ws = g.workspace(width)
    st = _lib.load().acm_spmm_ex(g.handle, table.data_ptr(), ld, width, y.data_ptr(), width, C.byref(o), ws.data_ptr(),
                                 ws.numel() * 4, _stream())
    _lib.check(st, "acm_spmm_ex")
    ref = spmm_ex_ref(op.matrix(), t64, rs if full else None, sub if full else None, ss if full else None, full)
    got = y.cpu().numpy()
    assert np.isfinite(got).all(), (name, width, ld, full, "non-finite output")
    return float(np.abs(got - ref).max()), 3e-5 * max(1.0, float(np.abs(ref).max()))


def spmm_ex_ref(a64, t64, row_scale, sub, sub_scale, relu):
    ref = a64 @ t64
    if row_scale is not None:
        ref = row_scale.astype(np.float64)[:, None] * ref
    if sub is not None:
        ref = ref - (sub_scale.astype(np.float64)[:, None] if sub_scale is not None else 1.0) * sub.astype(np.float64)
    return np.maximum(ref, 0.0) if relu else ref


def spmm_ex_status(name, width, ld, dev):
    """The status of acm_spmm_ex with g_bf16 = 1 at ``width`` (valid buffers of the full extent; nothing is asserted)."""
    from acm_gnn_amd import _lib
    op, g = operators()[name], handle_of(name, dev)
    table = torch.zeros(op.n_cols, ld, dtype=torch.bfloat16, device=dev)
    y = torch.zeros(op.n_rows, width, device=dev)
    o = _lib.SpmmOpts()
    o.g_bf16 = 1
    ws = g.workspace(min(width, 256))
    return _lib.load().acm_spmm_ex(g.handle, table.data_ptr(), ld, width, y.data_ptr(), width, C.byref(o), ws.data_ptr(),
                                   ws.numel() * 4, _stream())


# ---- part 3: acm_conv_bwd_spmm ----
def conv_bwd_inputs(name, f, dev, seed=1, ld_extra=0):
    """Tables and self terms of one K4 problem over the transposed operator ``name``: [G_L | G_H] in one bf16 table, G_S in its
    own; fp32 self terms, scales and masks (+-U(0.1, 1): the kernel lets a column through where its mask is positive)."""
    op = operators()[name]
    rng = np.random.default_rng(seed + f)
    n, nc = op.n_rows, op.n_cols
    glh, glh64 = bf16_table(rng.standard_normal((nc, 2 * f)).astype(np.float32), 2 * f + ld_extra, op.dead, dev)
    gs, gs64 = bf16_table(rng.standard_normal((nc, f)).astype(np.float32), f + ld_extra, op.dead, dev)
    host = dict(s_high=rng.standard_normal((n, f)), s_struc=rng.standard_normal((n, f)), self_scale=rng.uniform(0.5, 2.0, n),
                inv_deg=rng.uniform(0.05, 1.0, n), mask_low=rng.uniform(0.1, 1.0, (n, f)) * rng.choice([-1.0, 1.0], (n, f)),
                mask_high=rng.uniform(0.1, 1.0, (n, f)) * rng.choice([-1.0, 1.0], (n, f)))
    host = {k: v.astype(np.float32) for k, v in host.items()}
    return dict(op=op, f=f, glh=glh, gs=gs, glh64=glh64, gs64=gs64, host=host, a64=op.matrix(),
                devt={k: torch.from_numpy(v).to(dev) for k, v in host.items()})


def conv_bwd_ref(inp, struc, masks, self_scale, inv_deg):
    """fp64: dz_low = m_L (A^T G_L), dz_high = m_H (self_scale s_high - A^T G_H), d_struc = A^T G_S - s_struc inv_deg (``a64`` is
    the transposed operator itself)."""
    f, h, a = inp["f"], {k: v.astype(np.float64) for k, v in inp["host"].items()}, inp["a64"]
    dl = a @ inp["glh64"][:, :f]
    dh = (h["self_scale"][:, None] if self_scale else 1.0) * h["s_high"] - a @ inp["glh64"][:, f:]
    if masks:
        dl, dh = np.where(h["mask_low"] > 0, dl, 0.0), np.where(h["mask_high"] > 0, dh, 0.0)
    ds = a @ inp["gs64"] - h["s_struc"] * (h["inv_deg"][:, None] if inv_deg else 1.0) if struc else None
    return dl, dh, ds


def conv_bwd_struct(inp, struc, masks, self_scale, inv_deg, dev):
    """(acm_conv_bwd_spmm_t, the outputs [dZ_L | dZ_H | -] and d_struc -- NaN until written --, what must stay alive)."""
    from acm_gnn_amd import _lib
    f, d, n = inp["f"], inp["devt"], inp["op"].n_rows
    glh, gs = inp["glh"], inp["gs"]
    dz = torch.full((n, 3 * f), float("nan"), device=dev)
    d_struc = torch.full((n, f), float("nan"), device=dev)
    r = _lib.ConvBwdSpmm()
    r.f_out, r.row_offset, r.gather_bf16 = f, 0, 1
    r.g_low, r.ld_g_low = glh.data_ptr(), glh.stride(0)
    r.g_high, r.ld_g_high = glh.data_ptr() + 2 * f, glh.stride(0)
    r.s_high, r.ld_s_high = d["s_high"].data_ptr(), f
    if struc:
        r.g_struc, r.ld_g_struc = gs.data_ptr(), gs.stride(0)
        r.s_struc, r.ld_s_struc = d["s_struc"].data_ptr(), f
        r.d_struc, r.ld_d_struc = d_struc.data_ptr(), f
        if inv_deg:
            r.inv_deg = d["inv_deg"].data_ptr()
    if self_scale:
        r.self_scale = d["self_scale"].data_ptr()
    if masks:
        r.mask_low, r.ld_mask_low = d["mask_low"].data_ptr(), f
        r.mask_high, r.ld_mask_high = d["mask_high"].data_ptr(), f
    r.dz_low, r.ld_dz_low = dz.data_ptr(), 3 * f
    r.dz_high, r.ld_dz_high = dz.data_ptr() + 4 * f, 3 * f
    return r, dz, d_struc


def run_conv_bwd(name, inp, struc, masks, self_scale, inv_deg, dev, ref=None):
    """One acm_conv_bwd_spmm call with bf16 tables.  Returns (worst error / tolerance over its outputs, the reference)."""
    from acm_gnn_amd import _lib
    g = handle_of(name, dev)
    f = inp["f"]
    r, dz, d_struc = conv_bwd_struct(inp, struc, masks, self_scale, inv_deg, dev)
    ws = g.workspace((3 if struc else 2) * f)
    st = _lib.load().acm_conv_bwd_spmm(g.handle, C.byref(r), ws.data_ptr(), ws.numel() * 4, _stream())
    _lib.check(st, "acm_conv_bwd_spmm")
    ref = ref if ref is not None else conv_bwd_ref(inp, struc, masks, self_scale, inv_deg)
    got = [dz[:, :f].cpu().numpy(), dz[:, f:2 * f].cpu().numpy(), d_struc.cpu().numpy() if struc else None]
    worst = 0.0
    for nm, a, b in zip(("dz_low", "dz_high", "d_struc"), got, ref):
        if b is None:
            continue
        assert np.isfinite(a).all(), (name, f, nm, "non-finite output")
        err, tol = float(np.abs(a - b).max()), 1e-4 * max(1.0, float(np.abs(b).max()))
        assert err < tol, (name, f, nm, struc, masks, self_scale, inv_deg, err, tol)
        worst = max(worst, err / tol)
    return worst, ref


# ---- parts 4 and 5: the layer against the tables it recorded ----
def record_casts(monkeypatch):
    """Wrap cast_bf16 in every module that binds it; the returned list receives (source.clone(), result) per call."""
    from acm_gnn_amd.functional import _conv_shared, conv_agg, conv_literal, ops
    real, log = ops.cast_bf16, []

    def recording(src):
        out = real(src)
        log.append((src.detach().clone(), out))
        return out

    for mod in (ops, conv_literal, conv_agg, _conv_shared):
        monkeypatch.setattr(mod, "cast_bf16", recording)
    return log


def layer_graph(n=333, seed=17, density=0.05):
    from test_gpu_oracle import _graph
    return _graph(n, seed, density=density, hub=True)


def _filters64(adj):
    """(A_low as float64 scipy CSR with the float32 values the layer is given, P = I + A, deg = rowsum(P))."""
    from oracle import acm_oracle as O
    low, high, un = O.filters_linkx(adj)
    lc = low.coalesce()
    idx = lc.indices().numpy()
    a64 = sp.csr_matrix((lc.values().numpy().astype(np.float64), (idx[0], idx[1])), shape=tuple(low.shape))
    pat = sp.csr_matrix(sp.identity(adj.shape[0]) + adj)
    return (low, high, un), a64, pat, np.asarray(pat.sum(1)).reshape(-1)


def make_layer(f_in, f_out, n, model_type, variant, s, ln, seed, dev):
    from acm_gnn_amd import GraphConvolution
    torch.manual_seed(seed)
    layer = GraphConvolution(f_in, f_out, n, model_type, variant=variant, structure_info=s, attn_layernorm=ln, gather_dtype="bf16")
    with torch.no_grad():
        for nm in ("low", "high", "mlp", "struc_low"):
            getattr(layer, f"layer_norm_{nm}").weight.uniform_(0.5, 1.5)
            getattr(layer, f"layer_norm_{nm}").bias.uniform_(-0.5, 0.5)
    params = {k: v.detach().cpu().double().clone() for k, v in layer.named_parameters()}
    return layer.to(dev), params


# casts of one forward by route: the literal form rounds [Z_L | Z_H] (+ the struc_low rows); aggregate-first and the ACMII
# recompute gather the fp32 INPUT for the filterbank channels and round the struc_low rows alone
def expected_casts(route, s):
    return (1 if route == "literal" else 0) + int(bool(s))


def run_layer_forward(case, adj, dev, monkeypatch, tune):
    """Forward of one GraphConvolution(gather_dtype="bf16") against the fp64 reference that uses the recorded tables for every
    product with a gathered operand.  ``case``: (model_type, variant, s, ln, f_in, f_out, implicit, wide_form, agg_first, route).
    Returns the worst error / tolerance."""
    from acm_gnn_amd.graph import clear_cache
    from oracle import acm_oracle as O
    model_type, variant, s, ln, f_in, f_out, implicit, form, agg, route = case
    tune(agg_first=int(agg), acmii_recompute=1, acmii_mask=1)
    tune(implicit=int(implicit), wide_form=int(form))
    clear_cache()
    n, f = adj.shape[0], f_out
    (low, high, un), a64, _, deg = _filters64(adj)
    layer, p = make_layer(f_in, f_out, n, model_type, variant, s, ln, 3, dev)
    x = torch.randn(n, f_in, generator=torch.Generator().manual_seed(4))
    log = record_casts(monkeypatch)
    out = layer(x.to(dev), low.to(dev), high.to(dev), un.to(dev) if s else None)
    # (i) the number of casts is what the route implies -- and at least one: a silent fall-back to fp32 cannot pass
    assert len(log) == expected_casts(route, s) >= 1, (case, [tuple(a.shape) for a, _ in log])
    worst = 0.0
    # (ii) every table is the bit-exact rounding of its source
    for src, tab in log:
        assert tab.dtype == torch.bfloat16 and cast_mismatches(src, tab) == [], case
    tabs = {int(src.shape[1]): (src.cpu().double().numpy(), widen(tab)) for src, tab in log}
    x64 = x.double()
    zl, zh, zm = (x64 @ p[k] for k in ("weight_low", "weight_high", "weight_mlp"))
    sgc = model_type == "acmsgc"
    if variant and not sgc:
        zl, zh = torch.relu(zl), torch.relu(zh)
    tl, th = zl.numpy(), zh.numpy()
    # (iii) every source is the fp64 value it stands for
    if route == "literal":
        src, t64 = tabs[2 * f]
        want = np.concatenate([tl, th], 1)
        tol = 2e-5 * max(1.0, float(np.abs(want).max()))
        assert float(np.abs(src - want).max()) < tol, case
        worst = max(worst, note("4 layer forward: table source", float(np.abs(src - want).max()), tol))
        tl, th = t64[:, :f], t64[:, f:]
    h_low = torch.from_numpy(a64 @ tl)
    h_high = zh - torch.from_numpy(a64 @ th)
    if not sgc and not variant:
        h_low, h_high = torch.relu(h_low), torch.relu(h_high)
    chans = [h_low, h_high, zm if sgc else torch.relu(zm)]
    plus = model_type in ("acmgcnp", "acmgcnpp")
    if s:
        src, t64 = tabs[f]
        want = p["struc_low"].numpy()
        tol = 2e-5 * max(1.0, float(np.abs(want).max()))
        assert src.shape == want.shape and float(np.abs(src - want).max()) < tol, case
        chans.append(torch.relu(torch.from_numpy(deg[:, None] * (a64 @ t64)) - p["struc_low"]))
    att = O.attention(p, chans, bool(ln) and plus and not sgc)
    ref = (1 if s else 3) * sum(att[:, c:c + 1] * h for c, h in enumerate(chans))
    # (iv) the output and the mixing weights
    tol = 2e-5 * max(1.0, float(ref.abs().max()))
    err = float((out.detach().cpu().double() - ref).abs().max())
    assert err < tol, (case, err, tol)
    worst = max(worst, note("4 layer forward: out", err, tol))
    got_att = [layer.att_low, layer.att_high, layer.att_mlp] + ([layer.att_struc_vec_low] if s else [])
    err = float((torch.cat([t.detach().cpu().double().reshape(n, 1) for t in got_att], 1) - att).abs().max())
    assert err < 2e-5, (case, err)
    worst = max(worst, note("4 layer forward: mixing weights", err, 2e-5))
    return worst


def run_sgc_backward(f_in, f_out, x_grad, implicit, adj, dev, monkeypatch, tune):
    """acmsgc (no ReLU: nothing can flip) forward + backward with bf16 tables against an fp64 autograd reference whose gather is
    a custom Function: forward A [T_L | T_H] with the recorded forward table, backward A^T with the recorded backward table.
    Pins the offsets and gates of the literal backward's table plumbing.  Returns the worst error / tolerance."""
    from acm_gnn_amd.graph import clear_cache
    from oracle import acm_oracle as O
    tune(agg_first=0)
    tune(implicit=int(implicit))
    clear_cache()
    n, f = adj.shape[0], f_out
    (low, high, _), a64, pat, deg = _filters64(adj)
    layer, p = make_layer(f_in, f_out, n, "acmsgc", 0, 0, False, 5, dev)
    gen = torch.Generator().manual_seed(6)
    x, gout = torch.randn(n, f_in, generator=gen), torch.randn(n, f, generator=gen)
    log = record_casts(monkeypatch)
    xd = x.clone().to(dev).requires_grad_(x_grad)
    out = layer(xd, low.to(dev), high.to(dev), None)
    assert len(log) == 1 and tuple(log[0][0].shape) == (n, 2 * f), [tuple(a.shape) for a, _ in log]
    out.backward(gout.to(dev))
    assert len(log) == 2 and tuple(log[1][0].shape) == (n, 2 * f), [tuple(a.shape) for a, _ in log]
    for src, tab in log:
        assert cast_mismatches(src, tab) == []
    t_fwd, t_bwd = widen(log[0][1]), widen(log[1][1])
    # pattern-only operator: the backward gathers D^-1 G over P^T = (I + A)^T; explicit: G over A_low^T
    bwd_op = sp.csr_matrix(pat.T if implicit else a64.T)
    g_scale = (1.0 / deg)[:, None] if implicit else 1.0
    sign = np.concatenate([np.ones(f), -np.ones(f)])[None, :]
    seen = {}

    class Gather(torch.autograd.Function):
        @staticmethod
        def forward(ctx, zcat):
            return torch.from_numpy(a64 @ t_fwd)

        @staticmethod
        def backward(ctx, g):
            seen["g"] = g.numpy().copy()
            return torch.from_numpy((bwd_op @ t_bwd) * sign)

    pr = {k: v.clone().requires_grad_(True) for k, v in p.items()}
    xr = x.double().detach().requires_grad_(x_grad)
    zl, zh, zm = (xr @ pr[k] for k in ("weight_low", "weight_high", "weight_mlp"))
    prod = Gather.apply(torch.cat([zl, zh], 1))
    chans = [prod[:, :f], zh - prod[:, f:]]
    chans.append(zm)
    att = O.attention(pr, chans, False)
    ref = 3 * sum(att[:, c:c + 1] * h for c, h in enumerate(chans))
    ref.backward(gout.double())
    worst = 0.0
    tol = 2e-5 * max(1.0, float(ref.detach().abs().max()))
    err = float((out.detach().cpu().double() - ref.detach()).abs().max())
    assert err < tol, (err, tol)
    worst = max(worst, note("5 sgc backward: out", err, tol))
    # the forward table's source is [Z_L | Z_H]; the backward table's source is the reference's upstream gradient [G_L | G_H]
    want = torch.cat([zl, zh], 1).detach().numpy()
    tol = 2e-5 * max(1.0, float(np.abs(want).max()))
    assert float(np.abs(log[0][0].cpu().double().numpy() - want).max()) < tol
    want = seen["g"] * sign * g_scale
    tol = 1e-4 * max(1.0, float(np.abs(want).max()))
    err = float(np.abs(log[1][0].cpu().double().numpy() - want).max())
    assert err < tol, (err, tol)
    worst = max(worst, note("5 sgc backward: table source", err, tol))
    for k, prm in layer.named_parameters():
        rg = pr[k].grad
        if rg is None:
            assert prm.grad is None, k
            continue
        assert prm.grad is not None, k
        tol = 1e-4 * max(1.0, float(rg.abs().max()))
        err = float((prm.grad.cpu().double() - rg).abs().max())
        assert err < tol, (k, err, tol)
        worst = max(worst, note("5 sgc backward: gradients", err, tol))
    if x_grad:
        tol = 1e-4 * max(1.0, float(xr.grad.abs().max()))
        err = float((xd.grad.cpu().double() - xr.grad).abs().max())
        assert err < tol, (err, tol)
        worst = max(worst, note("5 sgc backward: gradients", err, tol))
    else:
        assert xd.grad is None
    return worst
