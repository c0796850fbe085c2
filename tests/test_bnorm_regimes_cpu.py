"""tests/bnorm_regimes.py without a GPU: every case reaches the regimes it is named after and keeps its ReLUs off rounding noise
(statements on the float64 restatement alone), and the comparison rule has teeth.  The library's CPU double computes in float32
(every product one chain of additions in k order, as the matrix pipe forms it) with either algebra:

* the centred one the package takes (acm_bnorm_fold_centred, acm_linear_fwd_shift, acm_gemm_shift, acm_bnorm_param_bwd_centred)
  stays within the rule on every case;
* the uncentred one -- a H + c, M a + s c, r (q - mu dbeta): the stack's first form, which the package still takes where a library
  lacks the centred symbols (the double hides them for this) -- is up to 62 units off on the pieces of the off-centre
  columns (dW_1[k, :] of OFF10, L = 3) where the centred one is 2 off at most, and breaks the rule on four cases of eight (every
  L = 3 case: 29, 62, 22, 22 units; the L = 2 cases measure 4.5 .. 12);
* a forgotten shift in the backward product is hundreds of units off on dgamma and dW_{i+1} of exactly the OFF columns, while
  the pieces of a DEAD column beside them stay within the rule: no pooling hides a column behind its neighbours;
* without an edited column both algebras pass.

The uncentred figures are far below the 290 / 193 units a rig with H as an exact float32 INPUT gives (there the float32 textbook
form loses almost nothing on an off-centre column).  In a stack H is itself the float32 result of x W^T + b: it carries
2^-24 mean / spread of its spread whatever happens next, the float32 textbook form -- the unit -- loses that too, and the uncentred
algebra's cancellation is the same size again times what its longer sums accumulate.  That is what an MI355X measured as well
(tests/test_gpu_bnorm_regimes.py: 32.1 against 7.1 units on the same cases)."""
import numpy as np
import pytest

import bnorm_regimes as B
import mlp_stack_ref as R

IDS = [f"{h}-L{L}-p{p}" for h, L, p in B.case_ids()]


@pytest.mark.parametrize("case", B.all_cases(), ids=IDS + ["big"])
def test_cases_reach_their_regimes_and_keep_their_masks(case):
    cov = B.coverage(case)
    assert len(cov) == (case.n_lins - 1) * len(case.cols)
    for what, (value, holds) in cov.items():
        print(f"{what}: {value}")
        assert holds, (what, value)
    safety = B.mask_safety(case)
    print(f"mask safety {safety:.2f}")
    assert safety >= 1.0
    for t in (case.x, case.dy) + tuple(t for p in case.lins + case.bns for t in p):
        assert t.dtype == np.float32 and not t.flags.writeable


def test_the_float32_restatement_is_the_float64_one_in_float32():
    """The unit's source: the same functions, every intermediate in float32 (the golden pin of the float64 form is
    tests/test_mlp_stack_cpu.py's)."""
    case = B.case_of(33, 2, 0.0, names=())
    y32, cache32, _ = R.forward(case.x, case.lins, case.bns, dtype=np.float32)
    y64, cache64, _ = R.forward(case.x, case.lins, case.bns)
    assert y32.dtype == np.float32 and all(t.dtype == np.float32 for c in cache32 for t in c if t is not None)
    assert 0 < np.abs(y32 - y64).max() < 1e-5
    dx32, d_lins32, d_bns32 = R.backward(case.dy, case.lins, case.bns, cache32, dtype=np.float32)
    dx64, d_lins64, d_bns64 = R.backward(case.dy, case.lins, case.bns, cache64)
    assert dx32.dtype == d_lins32[0][0].dtype == d_bns32[0][0].dtype == np.float32
    assert 0 < np.abs(d_bns32[0][0] - d_bns64[0][0]).max() < 1e-4


def _double_table(monkeypatch, case, **switches):
    fake = R.install(monkeypatch)
    fake.fp32 = True
    for k, v in switches.items():
        setattr(fake, k, v)
    ref64, floors, _ = B.reference(case.key, np.float64)
    ref32, _, _ = B.reference(case.key, np.float32)
    return B.ratios(B.run_stack(case, "cpu"), ref64, floors, ref32)


def _worst_off(case, table):
    return max(v for (kind, cls), v in B.worst_by_class(case, table).items() if cls.startswith("OFF"))


def test_the_rule_tells_the_centred_algebra_from_the_uncentred_one(monkeypatch):
    old_off, new_off, broken = [], [], 0
    for cid in B.case_ids():
        case = B.case_of(*cid)
        old = _double_table(monkeypatch, case, centred=False)
        new = _double_table(monkeypatch, case, centred=True)
        worst_old, worst_new = max(v[2] for v in old.values()), max(v[2] for v in new.values())
        print(f"{cid}: uncentred {worst_old:.1f} (OFF columns {_worst_off(case, old):.1f}), centred {worst_new:.1f} (OFF columns {_worst_off(case, new):.1f})")
        assert worst_new <= B.M, (cid, worst_new)
        old_off.append(_worst_off(case, old))
        new_off.append(_worst_off(case, new))
        broken += worst_old > B.M
    # (the centred double's own largest figure is 9.3: dgamma of an ordinary column behind two BatchNorms)
    assert max(old_off) > 3 * B.M and max(old_off) >= 16 * max(new_off) and broken >= 4, (old_off, new_off, broken)


@pytest.mark.parametrize("cid", B.case_ids(), ids=IDS)
def test_a_forgotten_shift_shows_on_its_own_columns_only(monkeypatch, cid):
    case = B.case_of(*cid)
    table = _double_table(monkeypatch, case, bwd_shift=False)
    worst = B.worst_by_class(case, table)
    for kind in ("dgamma", "dW[:,k]"):
        for cls in ("OFF100", "OFF1000"):
            print(f"{cid} {kind} {cls}: {worst[(kind, cls)]:.0f} units")
            assert worst[(kind, cls)] >= 4 * B.M, (kind, cls, worst[(kind, cls)])
    k = case.cols["DEAD"]                              # mu = 0: the forgotten shift changes nothing there, and nothing leaks in
    last = case.n_lins - 2                             # (the last BatchNorm: the pieces in front of it inherit the wrong dgamma)
    for piece in (f"dgamma{last}[{k}]", f"dW{last + 1}[:,{k}]", f"dbeta{last}[{k}]", "y", "y_eval"):
        assert table[piece][2] <= B.M, (piece, table[piece])


@pytest.mark.parametrize("cid", [(33, 2, 0.0), (64, 3, B.P_DROP)], ids=["33-L2", "64-L3-p0.3"])
def test_without_an_edited_column_both_algebras_pass(monkeypatch, cid):
    case = B.case_of(*cid, names=())
    assert not case.cols and B.mask_safety(case) >= 1.0
    for centred in (False, True):
        worst = max(v[2] for v in _double_table(monkeypatch, case, centred=centred).values())
        print(f"{cid} plain, {'centred' if centred else 'uncentred'}: {worst:.1f}")
        assert worst <= B.M
