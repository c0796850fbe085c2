"""What tests/head_regimes.py states about its stressed cases, asserted on the CPU oracle alone for every case that
tests/test_gpu_head_regimes.py uses -- the regimes each case reaches, that none of its ReLUs sits on rounding noise, that the
float32 oracle is a usable yardstick on it -- and the comparison rule's own test: a head with one term of its backward altered
must be rejected by the rule and is accepted by the 1e-4 max(1, .) rule of the existing oracle tests.

How far the altered heads exceed the rule (err / unit of the worst tensor, unit = max(e32, 2^-23 max|ref|); the rule allows M = 32),
on the default-regime case of ``test_the_rule_rejects_an_altered_term_that_the_absolute_floor_accepts``:
    sigmoid g (1 - g) -> g                                   1.5e7   (d layer_norm_low.bias)
    / k dropped in the backward                               1.5e7   (d layer_norm_struc_low.weight)
    LayerNorm backward without xhat mean(dxhat xhat)          7.3e4   (dX)
and on the stressed case of the same shape 1.7e8, 7.6e6 and 8.6e4 (there the existing rule rejects them too: its tolerance is
relative once a gradient exceeds 1).  Each test prints its figure."""
import pytest
import torch

import head_regimes as H

F64, F32 = torch.float64, torch.float32
SANITY = 1e-4                # float32 oracle within this of float64, relative to the tensor's largest element: a bound on the
                             # inputs (a flipped ReLU or a cancelled sum would break it), not on any kernel


def _rel32(ref64, ref32):
    return {k: float((ref32[k].double() - ref64[k]).abs().max()) / max(float(ref64[k].abs().max()), 1e-300) for k in ref64}


def test_every_gpu_case_has_a_seed_and_a_distinct_name():
    cases = H.layer_cases()
    assert len(cases) == len({c.id for c in cases}) >= 70
    assert set(H.builder_args()) | set(H.NLL_ARGS) | set(H.TAIL_ARGS) <= set(H.SEEDS)
    routes = {c.route for c in cases}
    assert {"literal", "agg-fused", "agg-two-stage-rows16", "agg-two-stage-rows4", "agg-two-stage-rows4-epilogue", "agg-wide-fused",
            "acmii-recompute", "acmii-mask", "acmii-literal", "acmsgc-agg", "acmsgc-literal"} <= routes


@pytest.mark.parametrize("args", H.builder_args(), ids=lambda a: "-".join(str(v) for v in a))
def test_layer_case_reaches_its_regimes_and_is_mask_safe(args):
    case = H.case_of(args)
    assert case.n == 203 and case.n % 16 != 0
    # the graph: a hub joined to every connected node, one raw self-loop, the last three nodes isolated
    deg = case.adj.getnnz(1)
    assert case.adj[0, 1:case.n - 3].getnnz() == case.n - 4 and case.adj[3, 3] == 1.0 and list(deg[-3:]) == [0, 0, 0]
    assert float(case.x[list(H.ZERO_ROWS)].abs().max()) == 0.0 and deg[H.ZERO_ROWS[2]] > 0
    cov, att = H.coverage(case)
    for what, (count, need) in cov.items():
        assert count >= need, (what, count, need)
    ref64, ref32 = H.oracle_run(case.key, F64), H.oracle_run(case.key, F32)
    # (the restated channels of head_regimes.pre_activations are the oracle's: they give its mixing weights bit for bit)
    assert torch.equal(att, ref64["att"])
    assert H.mask_safety(case) >= H.MASK_MARGIN
    # the rows that are exactly zero: every channel of an isolated zero row is exactly 0, and so is the output
    assert float(ref64["out"][list(H.ZERO_ROWS[:2])].abs().max()) == 0.0
    rel = _rel32(ref64, ref32)
    assert max(rel.values()) <= SANITY, max(rel.items(), key=lambda kv: kv[1])
    assert all(bool(torch.isfinite(v).all()) for v in ref32.values())


@pytest.mark.parametrize("name", list(H.SMALL_CONFIGS))
def test_two_layer_case_reaches_its_regimes_in_both_heads(name):
    """The model of the small-graph step: both heads leave the centre (the second layer's input is the first layer's output, so
    the variance / saturation statements are the first layer's; the second adds logits of a per-row range beyond 100)."""
    small = H.build_small(name)
    layers = H.small_layers(small, F64)
    for li, (p, x) in enumerate(layers):
        cov, _ = H.coverage(small.layer, p, x)
        for what, (count, need) in cov.items():
            if li == 0 or "alpha" in what:
                assert count >= need, (li, what, count, need)
        assert H.mask_safety(small.layer, p, x) >= H.MASK_MARGIN, li
    ref64, ref32 = H.small_reference(name, F64), H.small_reference(name, F32)
    z = ref64["logits"]
    assert int(((z.max(1).values - z.min(1).values) > 100).sum()) >= 5
    rel = _rel32(ref64, ref32)
    assert max(rel.values()) <= SANITY, max(rel.items(), key=lambda kv: kv[1])
    # without the gains the same draws stay in the centre (the other slot of the batched run)
    plain = H.small_layers(H.build_small(name, False), F64)
    assert H.coverage(small.layer, *plain[0])[0]["rows with max alpha > 0.9"][0] == 0


@pytest.mark.parametrize("args", sorted(set(H.NLL_ARGS) | set(H.TAIL_ARGS)), ids=lambda a: "-".join(str(v) for v in a))
def test_loss_cases_have_wide_rows_and_unlabelled_rows(args):
    case = H.case_of(args)
    y, w = H.loss_rows(case.n, case.f_out, case.seed)
    assert int((y < 0).sum()) >= 20 and float(w[y < 0].abs().max()) == 0.0 and abs(float(w.sum()) - 1.0) < 1e-5
    z = H.oracle_run(case.key, F64)["out"]
    wide = ((z.max(1).values - z.min(1).values) > 100) & (w > 0)
    assert int(wide.sum()) >= 5
    for ref in (H.nll_reference, H.tail_reference) if args in H.TAIL_ARGS else (H.nll_reference,):
        r64, r32 = ref(args, F64), ref(args, F32)
        rel = _rel32(r64, r32)
        assert max(rel.values()) <= SANITY, max(rel.items(), key=lambda kv: kv[1])
        assert float(r64["dlogits"][w == 0].abs().max()) == 0.0


# ---- the comparison rule's own test ------------------------------------------------------------------------------------------
MUTANT_ARGS = ("acmgcnp", 0, 1, True, 7, 64)          # four channels with LayerNorm: every altered term is live
# d-logits of a mean NLL are at most 1 / |train|: 1e-5 on the graph bench.py trains on (84 000 training rows).  At that scale
# every gradient is far below 1, and the existing rule's max(1, .) makes its tolerance an absolute 1e-4.
MEAN_LOSS_SCALE = 1e-5


def test_the_rule_accepts_the_unaltered_head():
    """The oracle's head restated with hand-written backward terms (what the altered heads are made from) in float64: inside
    the rule by many orders of magnitude, on the default-regime case and on the stressed one."""
    for stressed in (False, True):
        key = H.build_case(*MUTANT_ARGS, H.SEEDS[MUTANT_ARGS], stressed).key
        ref64, ref32 = H.oracle_run(key, F64), H.oracle_run(key, F32)
        table = H.compare(H.oracle_run(key, F64, H.UNALTERED), ref64, ref32, 1e-3)
        assert len(table) == len(ref64) >= 20


@pytest.mark.parametrize("name", list(H.MUTANTS))
def test_the_rule_rejects_an_altered_term_that_the_absolute_floor_accepts(name):
    """Inputs in the regime of the existing oracle tests (default initialisation, randn features), upstream gradient at the scale
    of a mean loss: a head whose backward has one term altered passes 1e-4 max(1, max|ref|) on every tensor -- and is outside the
    rule by a factor of 1e3 at the least, because the rule has no absolute floor."""
    key = H.build_case(*MUTANT_ARGS, H.SEEDS[MUTANT_ARGS], False).key
    ref64, ref32 = H.oracle_run(key, F64, None, MEAN_LOSS_SCALE), H.oracle_run(key, F32, None, MEAN_LOSS_SCALE)
    got = H.oracle_run(key, F64, H.MUTANTS[name], MEAN_LOSS_SCALE)
    assert H.old_rule_accepts(got, ref64)
    assert H.old_rule_accepts(H.oracle_run(key, F32, None, MEAN_LOSS_SCALE), ref64)
    with pytest.raises(AssertionError):
        H.compare(got, ref64, ref32, H.M)
    table = H.ratios(got, ref64, ref32)
    worst = max(table, key=lambda k: table[k][2])
    print(f"{name}: err / unit = {table[worst][2]:.3g} on {worst} (M = {H.M})")
    assert table[worst][2] > 1e3 * H.M
    # the forward is untouched: the altered term is found in the gradients alone
    assert table["out"][2] < 1e-3 and table["att"][2] < 1e-3


@pytest.mark.parametrize("name", list(H.MUTANTS))
def test_the_rule_rejects_an_altered_term_on_the_stressed_case(name):
    key = H.case_of(MUTANT_ARGS).key
    ref64, ref32 = H.oracle_run(key, F64), H.oracle_run(key, F32)
    table = H.ratios(H.oracle_run(key, F64, H.MUTANTS[name]), ref64, ref32)
    worst = max(table, key=lambda k: table[k][2])
    print(f"{name}: err / unit = {table[worst][2]:.3g} on {worst} (M = {H.M})")
    assert table[worst][2] > 1e3 * H.M


def test_the_rule_has_no_absolute_floor_and_pools_nothing():
    ref64 = {"a": torch.tensor([1e-6, -2e-6], dtype=F64), "b": torch.tensor([1e3], dtype=F64)}
    ref32 = {k: v.float() for k, v in ref64.items()}
    ok = {"a": ref64["a"].float(), "b": ref64["b"].float()}
    H.compare(ok, ref64, ref32, 1)
    off = dict(ok, a=ok["a"] * 1.001)                 # 0.1 % on a tensor of 1e-6: 2e-9 absolute, far inside any absolute floor
    assert H.old_rule_accepts(off, ref64)
    with pytest.raises(AssertionError):
        H.compare(off, ref64, ref32, H.M)
    nan = dict(ok, b=torch.tensor([float("nan")]))
    with pytest.raises(AssertionError):
        H.compare(nan, ref64, ref32, H.M)
