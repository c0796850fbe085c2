"""The statements tests/adam_regimes.py makes, none of which needs a GPU: the drawn elements reach every regime it names, the
kernel's operation order restated in float32 stays within K units of the float64 reference on all of them, every altered update
exceeds K, the rule of tests/test_gpu_optim.py accepts two of those altered updates on its own kind of input, and the CPU double's
acm_adam_step is within K units with distinct counters."""
import ctypes as C

import numpy as np
import pytest
import torch

import adam_regimes as A
import fake_lib

N = 20000
CASES = [(name, step) for name in A.SETTINGS for step in A.STEPS]


@pytest.fixture(scope="module")
def drawn():
    """{(setting, step): (inputs, float64 reference)}: computed once, never modified."""
    out = {}
    for i, (name, step) in enumerate(CASES):
        hp = A.SETTINGS[name]
        inputs = A.draw(N, 100 + i, hp, step)
        out[name, step] = (inputs, A.reference(*inputs, step, hp))
    return out


@pytest.mark.parametrize("name,step", CASES)
def test_the_drawn_elements_reach_every_regime(name, step, drawn):
    _, ref = drawn[name, step]
    shares = A.assert_coverage(ref, A.SETTINGS[name], step, (name, step))
    print(f"ADAMREG coverage {name} step {step} | " + " | ".join(f"{k}: {100 * s:.1f} %" for k, s in shares.items()))


def test_the_restatement_is_within_k_units_everywhere(drawn):
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for (name, step), (inputs, ref) in drawn.items():
        r = A.ratios(A.restated32(*inputs, step, A.SETTINGS[name]), ref)
        print(f"ADAMREG restated32 {name} step {step} | " + " | ".join(f"{q}' {r[q]:.2f}" for q in "mvp"))
        worst = {q: max(worst[q], r[q]) for q in worst}
    print("ADAMREG restated32 largest | " + " | ".join(f"{q}' {worst[q]:.2f}" for q in "mvp"))
    assert max(worst.values()) <= A.K, worst


@pytest.mark.parametrize("mutant", list(A.MUTANTS))
def test_every_altered_update_exceeds_k(mutant, drawn):
    worst, where = 0.0, None
    for (name, step), (inputs, ref) in drawn.items():
        r = max(A.ratios(A.MUTANTS[mutant](*inputs, step, A.SETTINGS[name]), ref).values())
        if r > worst:
            worst, where = r, (name, step)
    print(f"ADAMREG mutant {mutant} | largest ratio {worst:.3g} at {where}")
    assert worst > A.K, (mutant, worst)


# tests/test_gpu_optim.py::_shapes() without its three tensors above 4099 elements: every size a parameter of the models here has
# except the [n, 64] structure parameter
OLD_RULE_SHAPES = [(7, 64), (64, 1), (3, 3), (64,), (1, 1), (4099,)] + [(5, i + 1) for i in range(36)]


def _old_rule_misses(update, hp, steps=12):
    """tests/test_gpu_optim.py::test_fused_adam_matches_torch with ``update`` in place of the kernel: cold state, every counter
    equal, gradients randn * (1 + it), torch's single-tensor fp32 optimizer as the reference, rtol = 3e-6 and atol = 3e-6 of the
    tensor's largest element (of max(1, that) for the parameter).  Returns the number of elements the rule refuses."""
    lr, b1, b2, eps, wd, decoupled = hp
    gen = torch.Generator().manual_seed(0)
    init = [torch.randn(*s, generator=gen) for s in OLD_RULE_SHAPES]
    ref = [torch.nn.Parameter(t.clone()) for t in init]
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(ref, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    mine = [(t.numpy().reshape(-1).copy(), np.zeros(t.numel(), np.float32), np.zeros(t.numel(), np.float32)) for t in init]
    for it in range(steps):
        for i, q in enumerate(ref):
            q.grad = torch.randn(q.shape, generator=gen) * (1.0 + it)
            p, m, v = mine[i]
            mine[i] = update(p, q.grad.numpy().reshape(-1), m, v, it, hp, neighbour=it)        # the neighbour's counter: the same
        opt.step()
    refused = 0
    for (p, m, v), q in zip(mine, ref):
        st = opt.state[q]
        for got, want, floor in ((p, q.detach(), 1.0), (m, st["exp_avg"], 0.0), (v, st["exp_avg_sq"], 0.0)):
            want = want.numpy().reshape(-1)
            tol = 3e-6 * np.abs(want) + 3e-6 * max(floor, float(np.abs(want).max()))
            refused += int((~(np.abs(got - want) <= tol)).sum())
    return refused


def test_the_old_tolerance_accepts_altered_updates():
    """The gap.  On test_gpu_optim.py's kind of input -- randn gradients, cold state, equal counters, its three settings, twelve
    steps, its 42 tensors of up to 4099 elements -- its per-tensor tolerance refuses no element of an update that reads its
    neighbour's counter (at equal counters no alteration at all) on any setting, and none of an update with eps inside the bias
    correction on two of the three (one element of 10 000 on the third).  Measured once with that test's three larger tensors as
    well: the 1.3 M-element one does refuse eps-inside, on 184 elements whose FIRST gradient happened to fall below 1e-3 -- a
    protection by sample size alone, which the flush and small-graph routes (a few thousand elements) do not have."""
    misses = {}
    for name in ("adam", "adam-wd5e-4", "adamw-wd1e-2"):                     # test_gpu_optim.py's three settings
        hp = A.SETTINGS[name]
        assert _old_rule_misses(A.restated32, hp) == 0, name                   # the rule itself is met by the unaltered update
        for mutant in ("neighbouring counter", "eps inside the bias correction"):
            misses.setdefault(mutant, []).append(_old_rule_misses(A.MUTANTS[mutant], hp))
    print(f"ADAMREG elements the old rule refuses, per setting: {misses}")
    assert misses["neighbouring counter"] == [0, 0, 0], misses
    assert sum(n == 0 for n in misses["eps inside the bias correction"]) >= 2, misses


def test_the_cpu_double_is_within_k_units_with_distinct_counters(monkeypatch):
    from acm_gnn_amd import _lib
    fake = fake_lib.install(monkeypatch)
    hp = A.SETTINGS["adam-wd5e-4"]
    sizes = [5, 2049, 33, 700, 1, 4099]
    steps = A.counters(len(sizes), far=(1, 700), farther=4)
    rows = A.table(sizes, steps, 7, hp)
    state = [[torch.from_numpy(t.copy()) for t in row] + [torch.tensor(float(s))] for row, s in zip(rows, steps)]
    entries = (_lib.AdamTensor * len(sizes))()
    for e, (p, g, m, v, st) in zip(entries, state):
        e.param, e.grad, e.exp_avg, e.exp_avg_sq, e.step, e.numel = p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), st.data_ptr(), p.numel()
    counter = torch.zeros(1, dtype=torch.int64)
    cfg = _lib.AdamConfig(hp[0], hp[1], hp[2], hp[3], hp[4], int(hp[5]), counter.data_ptr(), None, None)
    assert fake.acm_adam_step(len(sizes), C.cast(entries, C.c_void_p), C.byref(cfg), None) == 0
    worst = {"p": 0.0, "m": 0.0, "v": 0.0}
    for row, s, (p, g, m, v, st) in zip(rows, steps, state):
        assert float(st) == s + 1 and np.array_equal(g.numpy(), row[1])
        r = A.ratios((p.numpy(), m.numpy(), v.numpy()), A.reference(*row, s, hp))
        worst = {q: max(worst[q], r[q]) for q in worst}
    print("ADAMREG cpu double | " + " | ".join(f"{q}' {worst[q]:.2f}" for q in "mvp"))
    assert int(counter) == 1 and max(worst.values()) <= A.K, worst
