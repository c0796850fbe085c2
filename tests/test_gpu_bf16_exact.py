"""The bf16 gather path (gather_dtype="bf16": cast_bf16_kernel, spmm_pair_kernel<.., true>, spmm_vec_kernel<.., 1, .., true> under
every epilogue, and the pointer arithmetic around them) against fp64 references that read THE VERY bf16 TABLE the kernel read,
widened exactly (tests/bf16_ref.py).  The rounding of the operand drops out of the error, so the bounds are the fp32 ones of
the neighbouring tests -- 3e-5 (acm_spmm_ex), 1e-4 (gradients), 2e-5 (layer output, mixing weights) of max(1, |ref|max) --
instead of the 2e-2 .. 0.35 of the range that a comparison against fp32 needs (test_gpu_bf16_sweep.py).  A dropped tail
neighbour, the wrong half of a packed pair, a mis-addressed channel or a lost piece of a split row is far outside them.
The worst error / tolerance per part is written as bf16_exact.json where ACM_EVIDENCE_DIR says (-> profiles/bf16_exact.json)."""
import numpy as np
import pytest
import torch

import bf16_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WIDTHS = tuple(range(10, 65, 2))                     # the whole envelope: every even width 8 < F <= 64


@pytest.fixture(autouse=True)
def _ratios():
    yield
    R.dump_ratios()


# ---- 1. the cast, bit for bit ----
def _cast_checked(src_dev):
    from acm_gnn_amd.functional import cast_bf16
    dst = cast_bf16(src_dev)
    assert dst.dtype == torch.bfloat16 and dst.is_contiguous() and tuple(dst.shape) == tuple(src_dev.shape)
    bad = R.cast_mismatches(src_dev, dst)
    assert bad == [], (len(bad), bad[:16])
    R.RATIOS.setdefault("1 cast_bf16: elements that differ (bit for bit)", 0.0)
    return dst


def test_cast_every_high_half_word_bit_for_bit():
    """All 65536 high half-words x the low half-words 0x0000, 0x0001, 0x7FFF, 0x8000, 0x8001, 0xFFFF against torch's CPU
    float32 -> bfloat16: non-NaN inputs bit-equal, NaN inputs a NaN of the same sign.  (The parent's kernel carried NaNs
    0x7F800001 .. 0x7F808000 into +inf and 0x7FFF8000 .. 0x7FFFFFFF into -0, the sign-mirrored ranges into -inf and +0.)"""
    bits = R.cast_patterns()
    assert bits.shape == (393216,)
    _cast_checked(R.f32_from_bits(bits).reshape(-1, 3).to(DEV))                 # an odd column count


def test_cast_of_a_column_slice_reads_only_the_slice():
    """ld_src > n_cols: the patterns as columns 3 .. 10 of a 13-column tensor whose other columns hold other values; and a finite
    slice between infinite columns, none of which may show up in the (contiguous, wrapper-allocated) destination."""
    bits = R.cast_patterns()
    wide = torch.full((len(bits) // 8, 13), 12345.0)
    wide[:, 3:11] = R.f32_from_bits(bits).reshape(-1, 8)
    part = wide.to(DEV)[:, 3:11]
    assert part.stride(0) == 13 and part.shape[1] == 8
    _cast_checked(part)
    wall = torch.full((257, 21), float("inf"))
    wall[:, 5:16] = torch.randn(257, 11, generator=torch.Generator().manual_seed(0))
    dst = _cast_checked(wall.to(DEV)[:, 5:16])
    assert bool(torch.isfinite(dst.float()).all())


def test_cast_smallest_shapes_and_the_second_grid_stride_trip():
    """1 x 1, no rows, and just above 4096 blocks x 256 elements (the grid cap): the loop's second trip."""
    for v in (1.00390625, float("nan"), -float("inf")):
        _cast_checked(torch.tensor([[v]], device=DEV))
    assert tuple(_cast_checked(torch.empty(0, 5, device=DEV)).shape) == (0, 5)
    rows, cols = 1025, 1031
    assert 4096 * 256 < rows * cols < 4096 * 256 + 16384
    bits = np.resize(R.cast_patterns()[::-1], rows * cols)
    _cast_checked(R.f32_from_bits(bits).reshape(rows, cols).to(DEV))


# ---- 2. acm_spmm_ex with a bf16 operand, over the whole envelope ----
@pytest.mark.parametrize("width", WIDTHS)
@pytest.mark.parametrize("name", R.FORWARD_OPS)
def test_spmm_ex_bf16_against_the_table_it_read(name, width, tune):
    """Every even width 10 .. 64 on both operators and both value kinds; the pair kernel (wide_form 1) and, where F % 4 == 0,
    the 8-byte vector kernel (2); plain and row_scale + sub + sub_scale + relu; a contiguous and a pitched table.  Table rows no
    stored entry references -- row 0 among them, which idle slots and idle lanes fetch -- and the pad columns hold NaN / inf:
    the result must be finite and within 3e-5 max(1, |ref|max) of A.astype(float64) @ widen(table)."""
    for form in (1, 2) if width % 4 == 0 else (1,):
        tune(wide_form=form)
        for ld in (width, width + (4 if form == 2 else 2)):        # (the vector kernel needs 8-byte rows: a pitch of 4 k)
            for full in (False, True):
                err, tol = R.run_spmm_ex(name, width, ld, full, DEV)
                print(f"{name} F{width} form{form} ld{ld} full{int(full)}: err {err:.3e} tol {tol:.3e}")
                R.note("2 acm_spmm_ex", err, tol)
                assert err < tol, (name, width, form, ld, full, err, tol)


@pytest.mark.parametrize("width", [8, 11, 33, 66])
def test_bf16_outside_the_envelope_is_refused_and_spmm_falls_back(width):
    """No bf16 kernel outside even 8 < F <= 64: the C ABI answers an error status, functional.spmm(..., bf16=True) the fp32
    result bit for bit."""
    from acm_gnn_amd import functional as AF
    ld = width + (width % 2)
    assert R.spmm_ex_status("ladder", width, ld, DEV) != 0
    g = R.handle_of("ladder", DEV)
    dense = torch.randn(g.n_cols, width, generator=torch.Generator().manual_seed(width)).to(DEV)
    timer = AF.KernelTimer()
    AF.set_kernel_timer(timer)
    try:
        a, b = AF.spmm(g, dense, bf16=True), AF.spmm(g, dense)
    finally:
        AF.set_kernel_timer(None)
    assert torch.equal(a, b) and not any(k.startswith("cast_bf16") for k in timer.events), list(timer.events)


# ---- 3. acm_conv_bwd_spmm with bf16 tables, at the kernel ----
@pytest.mark.parametrize("f", [10, 12, 18, 32, 34, 62, 64])
@pytest.mark.parametrize("name", R.TRANSPOSED_OPS)
def test_conv_bwd_spmm_bf16_against_the_tables_it_read(name, f, tune):
    """dz_low = m_L (A^T G_L), dz_high = m_H (self_scale S_H - A^T G_H), d_struc = A^T G_S - S_S inv_deg in fp64 over the
    widened tables, 1e-4 max(1, |ref|max): two and three gathered channels fused (EpiBwd), one channel per pass
    (bwd_split = 1: EpiBwdLow / High / Struc), the pair and the vector kernel, masks / self_scale / inv_deg present and absent,
    on the transposes of both operators and both value kinds."""
    inp = R.conv_bwd_inputs(name, f, DEV)
    for struc in (False, True):
        for masks, self_scale, inv_deg in ((1, 1, 1), (0, 0, 0), (0, 1, 0), (1, 0, 1)):
            ref = None
            for split in (0, 1):
                for form in (1, 2) if f % 4 == 0 else (1,):
                    tune(bwd_split=split, wide_form=form)
                    worst, ref = R.run_conv_bwd(name, inp, struc, masks, self_scale, inv_deg, DEV, ref)
                    print(f"{name} F{f} k{3 + struc} split{split} form{form} opts{masks}{self_scale}{inv_deg}: err/tol {worst:.3f}")
                    R.note("3 acm_conv_bwd_spmm", worst, 1.0)


@pytest.mark.parametrize("split", [0, 1])
def test_conv_bwd_spmm_refuses_an_odd_pitch(split, tune):
    """bf16 tables are 4-byte aligned with an even pitch; an odd one is an error status and nothing runs."""
    import ctypes as C
    from acm_gnn_amd import _lib
    tune(bwd_split=split)
    name = "ladder-T"
    g = R.handle_of(name, DEV)
    inp = R.conv_bwd_inputs(name, 12, DEV, ld_extra=1)
    assert inp["glh"].stride(0) == 25 and inp["gs"].stride(0) == 13
    r, dz, d_struc = R.conv_bwd_struct(inp, True, True, True, True, DEV)
    ws = g.workspace(36)
    st = _lib.load().acm_conv_bwd_spmm(g.handle, C.byref(r), ws.data_ptr(), ws.numel() * 4, R._stream())
    torch.cuda.synchronize()
    assert st != 0
    assert bool(torch.isnan(dz).all()) and bool(torch.isnan(d_struc).all())


# ---- 4. the layer, forward, against the recorded tables ----
# (model_type, variant, structure_info, LayerNorm, f_in, f_out, implicit, wide_form, agg_first, route)
LAYER_CASES = [
    ("acmgcn", 0, 0, False, 20, 10, 1, 1, 0, "literal"), ("acmgcn", 1, 0, False, 20, 16, 0, 2, 0, "literal"),
    ("acmgcnp", 0, 0, True, 24, 18, 1, 1, 0, "literal"), ("acmgcnp", 0, 1, True, 24, 34, 1, 3, 0, "literal"),
    ("acmgcnp", 1, 1, True, 40, 62, 0, 1, 0, "literal"), ("acmgcnp", 1, 0, False, 40, 64, 1, 2, 0, "literal"),
    ("acmgcnp", 0, 1, False, 33, 64, 0, 3, 0, "literal"), ("acmgcnpp", 0, 1, True, 20, 16, 1, 2, 0, "literal"),
    ("acmgcnpp", 1, 0, True, 20, 10, 1, 1, 0, "literal"), ("acmgcnp", 0, 0, True, 40, 64, 1, 2, 0, "literal"),
    ("acmsgc", 0, 0, False, 30, 64, 1, 2, 0, "literal"), ("acmsgc", 0, 0, False, 30, 34, 0, 1, 0, "literal"),
    # aggregate-first with the structure channel: sg_bf16 (conv_agg.py)
    ("acmgcnp", 0, 1, True, 7, 64, 1, 2, 1, "agg"), ("acmgcnp", 0, 1, False, 7, 18, 1, 1, 1, "agg"),
    ("acmgcnp", 0, 1, True, 16, 62, 0, 1, 1, "agg"), ("acmgcnpp", 0, 1, True, 4, 16, 1, 3, 1, "agg"),
    ("acmgcnp", 0, 1, True, 12, 34, 1, 2, 1, "agg"),
    # the ACMII first layer: spmm(..., bf16=...) of its structure channel (conv_literal.py), mask form and the fp32 recompute
    ("acmgcnp", 1, 1, True, 7, 64, 1, 2, 1, "acmii"), ("acmgcnp", 1, 1, False, 8, 64, 1, 1, 1, "acmii"),
    ("acmgcnp", 1, 1, True, 7, 64, 0, 2, 1, "acmii"),
]
ROUTE_LABELS = {"literal": {"conv_fwd"}, "agg": {"conv_agg_fwd", "conv_agg_epi"}, "acmii": {"conv_acmii_fwd", "conv_acmii_v_fwd"}}


def _forward_case(case, adj, monkeypatch, tune):
    from acm_gnn_amd import functional as AF
    timer = AF.KernelTimer()
    AF.set_kernel_timer(timer)
    try:
        worst = R.run_layer_forward(case, adj, DEV, monkeypatch, tune)
    finally:
        AF.set_kernel_timer(None)
    used = set(k.split("/")[0] for k in timer.events)
    route = case[-1]
    assert "cast_bf16" in used and used & ROUTE_LABELS[route], (case, used)
    for other, labels in ROUTE_LABELS.items():
        assert other == route or not (used & labels), (case, used)
    if route == "acmii":                               # pattern-only operator, input without gradient: the mask form
        assert ("conv_acmii_v_fwd" in used) == bool(case[6]) and any(k.startswith("spmm/W64b") for k in timer.events), (case, used)
    print(f"{case}: worst err/tol {worst:.3f}")


@pytest.mark.parametrize("case", LAYER_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_layer_forward_against_its_recorded_tables(case, monkeypatch, tune):
    """GraphConvolution(..., gather_dtype="bf16") with cast_bf16 wrapped in every module that binds it: the number of casts is
    what the route implies (at least one), every table is the bit-exact rounding of its source, every source is the fp64 value
    it stands for (2e-5), and the output and the mixing weights are within 2e-5 of the fp64 oracle formulas with each gathered
    operand replaced by its recorded table.  The forward has no discontinuity: no seed picking."""
    _forward_case(case, R.layer_graph(), monkeypatch, tune)


def test_layer_forward_on_rows_of_several_windows(monkeypatch, tune):
    """The same on the 700-node graph with chunk 8 (its hub takes three windows of pieces), four channels."""
    from test_gpu_oracle import _graph
    tune(chunk=8)
    _forward_case(("acmgcnp", 0, 1, True, 24, 64, 1, 2, 0, "literal"), _graph(700, 31, density=0.04, hub=True), monkeypatch, tune)


# ---- 5. the layer, backward plumbing, where nothing can flip ----
@pytest.mark.parametrize("implicit", [1, 0])
@pytest.mark.parametrize("x_grad", [False, True])
@pytest.mark.parametrize("f_out", [10, 64])
def test_sgc_backward_gathers_the_recorded_gradient_tables(f_out, x_grad, implicit, monkeypatch, tune):
    """acmsgc has no ReLU.  Forward and backward with bf16 tables against an fp64 autograd reference whose gather is a custom
    Function (forward A widen(T_fwd), backward A^T widen(T_bwd) with the recorded backward table): the backward table's source
    is the reference's upstream gradient (1e-4), every parameter gradient and x.grad are within 1e-4 max(1, |ref|max) -- the
    table offsets and the gate of the literal backward; the kernels themselves are pinned by part 3."""
    from acm_gnn_amd import functional as AF
    timer = AF.KernelTimer()
    AF.set_kernel_timer(timer)
    try:
        worst = R.run_sgc_backward(30, f_out, x_grad, implicit, R.layer_graph(), DEV, monkeypatch, tune)
    finally:
        AF.set_kernel_timer(None)
    used = set(k.split("/")[0] for k in timer.events)
    assert {"cast_bf16", "conv_fwd", "conv_bwd_spmm"} <= used, used
    print(f"acmsgc F{f_out} x_grad{int(x_grad)} implicit{implicit}: worst err/tol {worst:.3f}")
