"""The references and the recording wrapper of tests/bf16_ref.py against the CPU twin (tests/fake_lib.py): a mistake in a
reference shows here, without a GPU.  Also the twin's own bf16 cast over the patterns the device test runs."""
import numpy as np
import pytest
import torch

import bf16_ref as R
import fake_lib


def test_fake_cast_rounds_every_pattern_like_torch_and_keeps_nan(monkeypatch):
    """The twin's acm_cast_bf16 over all 65536 high half-words x six low half-words: non-NaN inputs bit-equal to torch's CPU
    float32 -> bfloat16, NaN inputs a NaN of the same sign."""
    fake_lib.install(monkeypatch)
    from acm_gnn_amd.functional import cast_bf16
    bits = R.cast_patterns()
    assert bits.shape == (393216,) and len(np.unique(bits)) == 393216
    src = R.f32_from_bits(bits).reshape(-1, 3)
    assert R.cast_mismatches(src, cast_bf16(src)) == []
    wide = R.f32_from_bits(bits[:6 * 4096]).reshape(-1, 12)
    part = wide[:, 3:10]
    assert part.stride(0) == 12 and R.cast_mismatches(part, cast_bf16(part)) == []
    assert tuple(cast_bf16(torch.empty(0, 5)).shape) == (0, 5)


def test_mismatch_report_sees_the_carry_that_loses_a_nan():
    """The check itself: the parent formula (one carry for every input) is reported for exactly the NaN patterns it turns into
    inf or zero, and for nothing else."""
    bits = R.cast_patterns()
    b = bits.astype(np.uint64)
    old = (((b + 0x7FFF + ((b >> 16) & 1)) >> 16) & 0xFFFF).astype(np.uint16)
    bad = R.cast_mismatches(R.f32_from_bits(bits), torch.from_numpy(old.view(np.int16)).view(torch.bfloat16))
    # 0x7F800001 .. 0x7F808000 carry into +inf, 0x7FFF8000 .. 0x7FFFFFFF into -0; the sign-mirrored ranges into -inf and +0
    lost = {s for s in bits.tolist() if 0x7F800001 <= (s & 0x7FFFFFFF) <= 0x7F808000 or (s & 0x7FFFFFFF) >= 0x7FFF8000}
    assert len(lost) == 12 and {int(s, 16) for s, _, _ in bad} == lost
    assert {g for _, g, _ in bad} == {"0x7f80", "0xff80", "0x0", "0x8000"}


def test_operator_ladder_and_value_kinds():
    ops = R.operators()
    lad = ops["ladder"]
    assert tuple(lad.lengths[:len(R.LADDER)]) == R.LADDER and lad.n_rows == lad.n_cols == 333 and lad.chunk == 16
    assert (lad.vals != 0).all() and {0, 100, 332} <= set(lad.dead)
    unit = ops["ladder-unit"]
    assert unit.vals is None and (unit.lengths == lad.lengths + (lad.lengths > 0)).all()
    m = unit.matrix()
    m.sum_duplicates()
    assert m.data.max() == 2.0 and (m.data == 2.0).sum() == (lad.lengths > 0).sum()
    hub = ops["hub"]
    assert hub.chunk == 8 and hub.lengths.max() >= 699 and set(hub.dead) == {0, 701}
    for nm in R.BASE_OPS:
        a, t = ops[nm].matrix(), ops[nm + "-T"].matrix()
        assert np.abs(a.toarray().T - t.toarray()).max() == 0 and ops[nm + "-T"].n_rows == ops[nm].n_cols
    whole = ops["ladder-whole"]
    assert whole.chunk == 256 and (whole.indices == lad.indices).all() and (whole.vals == lad.vals).all()
    assert 0 in ops["ladder-T"].dead                     # row 0 of the ladder is empty: the transposed gather never reads it


@pytest.mark.parametrize("name,width,ld,full", [("ladder", 10, 12, True), ("hub-unit", 64, 64, False)])
def test_spmm_ex_reference_against_the_twin(name, width, ld, full, monkeypatch):
    fake_lib.install(monkeypatch)
    R.forget_handles()
    err, tol = R.run_spmm_ex(name, width, ld, full, "cpu")
    assert err < tol, (err, tol)
    assert R.spmm_ex_status(name, 8, 8, "cpu") != 0 and R.spmm_ex_status(name, 11, 12, "cpu") != 0
    R.forget_handles()


@pytest.mark.parametrize("name,f,struc,on", [("ladder-T", 10, True, True), ("hub-unit-T", 64, False, False)])
def test_conv_bwd_reference_against_the_twin(name, f, struc, on, monkeypatch):
    fake_lib.install(monkeypatch)
    R.forget_handles()
    inp = R.conv_bwd_inputs(name, f, "cpu")
    worst, _ = R.run_conv_bwd(name, inp, struc, on, on, on, "cpu")
    assert worst < 1.0
    R.forget_handles()


@pytest.mark.parametrize("case", [("acmgcnp", 0, 1, True, 24, 18, 1, 1, 0, "literal"), ("acmgcn", 1, 0, False, 20, 10, 0, 1, 0, "literal"),
                                  ("acmgcnp", 0, 1, True, 7, 16, 1, 1, 1, "agg")], ids=lambda c: "-".join(str(v) for v in c))
def test_layer_forward_reference_against_the_twin(case, monkeypatch, tune):
    fake_lib.install(monkeypatch)
    assert R.run_layer_forward(case, R.layer_graph(120, 17, 0.08), "cpu", monkeypatch, tune) < 1.0


@pytest.mark.parametrize("f_out,x_grad,implicit", [(10, True, 1), (64, False, 0)])
def test_sgc_backward_reference_against_the_twin(f_out, x_grad, implicit, monkeypatch, tune):
    fake_lib.install(monkeypatch)
    assert R.run_sgc_backward(30, f_out, x_grad, implicit, R.layer_graph(120, 17, 0.08), "cpu", monkeypatch, tune) < 1.0
