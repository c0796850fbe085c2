"""One Adam / AdamW step per element in every kernel that applies it, from warm state and with a different step counter on every
tensor (tests/adam_regimes.py: the float64 reference, the unit, the element regimes; tests/test_adam_regimes_cpu.py asserts what
that module states).  MI355X box.

Four routes: acm_adam_step's block update (both packs of a 45-tensor table, vector / tail / scalar paths; the separate advance
kernel), its flush-in-launch form (the reducing blocks update the gradient elements they produce and look their tensor's
counter up themselves), the small-graph step (four epilogues reading per-tensor factors from a table) and the batched small step
(hyper-parameters per slot as well).  Each test seeds the state, runs one step, computes the reference from what the kernel was
given -- where the kernel produces the gradient itself, the gradient read back after the step -- and asserts

    |got - ref64| <= K * unit,  K = 8,    for every element of p', m' and v' of every tensor,

that every counter rose by exactly 1, and also_advance with them.  Largest ratios measured: EXPERIMENTS.md, "One Adam step per
element"."""
import ctypes as C
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import adam_regimes as A
from test_gpu_optim import _segments_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                       # (a copy: the host array stays what the reference is computed from)


def _host(t):
    return t.detach().cpu().numpy().reshape(-1).copy()


class _Worst:
    """Largest ratio per quantity over the tensors of a case; ``check`` logs the figures, then asserts."""

    def __init__(self, what):
        self.what, self.r, self.at = what, {"p": 0.0, "m": 0.0, "v": 0.0}, {"p": None, "m": None, "v": None}

    def add(self, tensor, before, g, after, step, hp):
        """before / after: (p, m, v) as flat fp32 arrays; g: the gradient the kernel used; step: the counter before the step."""
        ref = A.reference(before[0], g, before[1], before[2], step, hp)
        r = A.ratios((after[0], after[1], after[2]), ref)
        for q in self.r:
            if r[q] > self.r[q]:
                self.r[q], self.at[q] = r[q], tensor

    def check(self):
        print(f"ADAMREG {self.what} | " + " | ".join(f"{q}' {self.r[q]:.2f} ({self.at[q]})" for q in "mvp"))
        assert max(self.r.values()) <= A.K, (self.what, self.r, self.at)


# ---- a. acm_adam_step, plain ------------------------------------------------------------------------------------------------
def _plain_table(hp):
    steps = A.counters(len(A.PLAIN_SIZES))
    assert steps[39] + 1 == steps[40] and 100000 in steps[40:]           # distinct across the pack boundary too
    return steps, A.table(A.PLAIN_SIZES, steps, 11, hp)


def _device_state(rows, steps):
    """Parameters, gradients (every second one a 4-byte-offset view: the scalar path), moments and counters on the device."""
    out = []
    for i, ((p, g, m, v), s) in enumerate(zip(rows, steps)):
        if i % 2:
            buf = torch.empty(g.size + 1, device=DEV)
            gd = buf[1:]
            gd.copy_(torch.from_numpy(g))
        else:
            gd = _dev(g)
        out.append(dict(p=_dev(p), g=gd, m=_dev(m), v=_dev(v), step=torch.tensor(float(s), device=DEV)))
    return out


def _check_plain(what, rows, steps, state, hp):
    worst = _Worst(what)
    for i, ((p, g, m, v), s, st) in enumerate(zip(rows, steps, state)):
        assert float(st["step"]) == s + 1, (i, s, float(st["step"]))
        assert np.array_equal(_host(st["g"]), g), i
        worst.add(f"#{i}:{p.size}", (p, m, v), g, (_host(st["p"]), _host(st["m"]), _host(st["v"])), s, hp)
    worst.check()


@pytest.mark.parametrize("setting", list(A.SETTINGS))
def test_adam_step_per_element_through_the_optimizer(setting):
    """FusedAdam / FusedAdamW with optimizer.state seeded before the first step(): 45 tensors (the last five in the second pack),
    sizes around the chunk of 2048, every second gradient a 4-byte-offset view, counters 0, 1, 2, ... with one at 700 and one at
    100 000."""
    from acm_gnn_amd import FusedAdam, FusedAdamW
    hp = A.SETTINGS[setting]
    steps, rows = _plain_table(hp)
    state = _device_state(rows, steps)
    params = [torch.nn.Parameter(st["p"]) for st in state]
    opt = (FusedAdamW if hp[5] else FusedAdam)(params, lr=hp[0], betas=(hp[1], hp[2]), eps=hp[3], weight_decay=hp[4])
    for prm, st in zip(params, state):
        opt.state[prm] = {"step": st["step"], "exp_avg": st["m"], "exp_avg_sq": st["v"]}
        prm.grad = st["g"]
    opt.also_advance = torch.full((1,), 41, dtype=torch.int64, device=DEV)
    opt.step()
    torch.cuda.synchronize()
    assert int(opt.also_advance) == 42
    for prm, st in zip(params, state):                  # the optimizer adopted the seeded tensors, it did not replace them
        assert opt.state[prm]["exp_avg"].data_ptr() == st["m"].data_ptr() and opt.state[prm]["step"].data_ptr() == st["step"].data_ptr()
        st["p"] = prm.detach()
    _check_plain(f"plain | {setting}", rows, steps, state, hp)


def test_adam_step_per_element_with_the_separate_advance_kernel():
    """The C ABI with arrive = NULL: the update launches carry no arrival counter and adam_advance_kernel raises the counters of
    each pack afterwards."""
    from acm_gnn_amd import _lib
    lib = _lib.load()
    hp = A.SETTINGS["adam-wd5e-4"]
    steps, rows = _plain_table(hp)
    state = _device_state(rows, steps)
    entries = (_lib.AdamTensor * len(state))()
    for e, st in zip(entries, state):
        e.param, e.grad, e.exp_avg, e.exp_avg_sq = st["p"].data_ptr(), st["g"].data_ptr(), st["m"].data_ptr(), st["v"].data_ptr()
        e.step, e.numel = st["step"].data_ptr(), st["p"].numel()
    counter = torch.full((1,), 7, dtype=torch.int64, device=DEV)
    cfg = _lib.AdamConfig(hp[0], hp[1], hp[2], hp[3], hp[4], int(hp[5]), counter.data_ptr(), None, None)
    _lib.check(lib.acm_adam_step(len(state), C.cast(entries, C.c_void_p), C.byref(cfg), None))
    torch.cuda.synchronize()
    assert int(counter) == 8
    _check_plain("plain, arrive = NULL | adam-wd5e-4", rows, steps, state, hp)


# ---- b. acm_adam_step with pending: the flush inside the launch ---------------------------------------------------------------
FLUSH_NAMES = ["w", "b", "v", "odd", "free", "big"]                      # the segments produce the gradients of w, b, v
FLUSH_STEPS = {"w": 2, "b": 100000, "v": 9, "odd": 14, "free": 700, "big": 23}      # no covered counter next to an uncovered one


def _flush_run(hp, fused):
    """Two steps of tests/test_gpu_optim.py's segments case from warm moments and distinct counters.  Returns per step
    {tensor: (before, gradient read back, after, counter before)} and the non-gradient output."""
    from acm_gnn_amd import _lib
    lib = _lib.load()
    lst, views, loss, want, keep = _segments_case()
    rng = np.random.default_rng(5)
    sizes = {"w": 7 * 192, "b": 64, "v": 96, "odd": 5, "free": 33, "big": 5000}
    grads = dict(views)
    grads["free"], grads["big"] = torch.zeros(33, device=DEV), torch.zeros(5000, device=DEV)
    host = {}
    for k in FLUSH_NAMES:
        p = A.draw_p(rng, sizes[k])
        # the gradient the moments are drawn around: what the segments will sum to / the one written below
        g = want[k].reshape(-1).float().cpu().numpy() if k in want else A.draw_g(rng, sizes[k], p, hp)
        m, v = A.draw_moments(rng, p, g, hp, FLUSH_STEPS[k])
        host[k] = (p, g, m, v)
    params = {k: _dev(host[k][0]).view(grads[k].shape) for k in FLUSH_NAMES}
    m = {k: _dev(host[k][2]).view(grads[k].shape) for k in FLUSH_NAMES}
    v = {k: _dev(host[k][3]).view(grads[k].shape) for k in FLUSH_NAMES}
    steps = {k: torch.tensor(float(FLUSH_STEPS[k]), device=DEV) for k in FLUSH_NAMES}
    counter = torch.zeros(1, dtype=torch.int64, device=DEV)
    arrive = torch.zeros(1, dtype=torch.int32, device=DEV)
    entries = (_lib.AdamTensor * len(FLUSH_NAMES))()
    for e, k in zip(entries, FLUSH_NAMES):
        e.param, e.grad, e.exp_avg, e.exp_avg_sq = params[k].data_ptr(), grads[k].data_ptr(), m[k].data_ptr(), v[k].data_ptr()
        e.step, e.numel = steps[k].data_ptr(), params[k].numel()
    n_seg = lst.n
    record = []
    for it in range(2):
        before = {k: (_host(params[k]), _host(m[k]), _host(v[k]), float(steps[k])) for k in FLUSH_NAMES}
        for k in ("odd", "free", "big"):                                  # the gradients no segment writes: drawn for this step
            grads[k].copy_(torch.from_numpy(host[k][1] if it == 0 else A.draw_g(rng, sizes[k], before[k][0], hp)))
        lst.n = n_seg
        cfg = _lib.AdamConfig(hp[0], hp[1], hp[2], hp[3], hp[4], int(hp[5]), counter.data_ptr(), arrive.data_ptr(),
                              C.addressof(lst) if fused else None)
        if not fused:
            _lib.check(lib.acm_reduce_flush(C.byref(lst), None))
        _lib.check(lib.acm_adam_step(len(FLUSH_NAMES), C.cast(entries, C.c_void_p), C.byref(cfg), None))
        torch.cuda.synchronize()
        assert lst.n == 0 and int(counter) == it + 1 and int(arrive) == 0
        record.append({k: (before[k][:3], _host(grads[k]), (_host(params[k]), _host(m[k]), _host(v[k])), before[k][3], float(steps[k]))
                       for k in FLUSH_NAMES})
    for k in ("w", "b", "v"):                                             # the segments stored the sums they were given
        torch.testing.assert_close(views[k].double(), want[k].view(views[k].shape), rtol=1e-5, atol=1e-4)
    return record, float(loss)


@pytest.mark.parametrize("setting", ["adam-wd5e-4", "adamw-lr0.05"])
def test_adam_step_per_element_with_the_flush_inside_the_launch(setting):
    """Each of two steps on its own, from the state read back before it, with the gradients the segments stored; and the whole
    record bit-identical to acm_reduce_flush followed by acm_adam_step from the same seeded state."""
    hp = A.SETTINGS[setting]
    (apart, loss_a), (fused, loss_f) = _flush_run(hp, False), _flush_run(hp, True)
    for it, rec in enumerate(fused):
        worst = _Worst(f"flush in launch, step {it + 1} | {setting}")
        for k, (before, g, after, s, s_after) in rec.items():
            assert s == FLUSH_STEPS[k] + it and s_after == s + 1, (k, s, s_after)
            worst.add(k, before, g, after, s, hp)
        worst.check()
    assert loss_a == loss_f
    for rec_a, rec_f in zip(apart, fused):
        for k in FLUSH_NAMES:
            for part_a, part_f in zip(rec_a[k][:3], rec_f[k][:3]):
                for x, y in zip(part_a if isinstance(part_a, tuple) else (part_a,), part_f if isinstance(part_f, tuple) else (part_f,)):
                    assert np.array_equal(x.view(np.int32), y.view(np.int32)), k
            assert rec_a[k][3:] == rec_f[k][3:], k


# ---- c. / d. the small-graph step, single and batched ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _small_problem(k4):
    from acm_gnn_amd import SparseFeatures, data as D, train as T
    from acm_gnn_amd.distributed import make_sharded_operators
    sg = A.small_graph()
    low, deg = D.build_filters(sp.csr_matrix(sg.adj, dtype=np.float32))
    ops = make_sharded_operators(low, deg, torch.device(DEV), with_structure=k4)
    xs = SparseFeatures.from_scipy(sp.csr_matrix(sg.x), DEV)
    y = torch.from_numpy(sg.y).to(DEV)
    w = T.row_weights(torch.from_numpy(sg.train).to(DEV), sg.n)
    return ops, xs, y, w


def _small_model(config, seed):
    from acm_gnn_amd import GCN
    mt, s, ln = A.SMALL_CONFIGS[config]
    torch.manual_seed(seed)
    model = GCN(A.SMALL_F_IN, A.SMALL_HIDDEN, A.SMALL_CLASSES, 2, A.small_graph().n, 0.0, mt, s, variant=False, attn_layernorm=ln)
    with torch.no_grad():                              # LayerNorm parameters away from (1, 0): their gradients are live
        for name, p in model.named_parameters():
            if "layer_norm" in name:
                p.add_(0.3 * torch.randn_like(p))
    model = model.to(DEV)
    model.train()
    return model


def _role_tensors(model):
    """[(layer, role name, parameter)] in the order of the step's tensor table."""
    from acm_gnn_amd import small
    cfg = model.gcns[0]._config()
    return [(li, small._ROLE_NAMES[r], small._param(layer, r)) for li, layer in enumerate(model.gcns) for r in small._roles(cfg)]


@functools.lru_cache(maxsize=None)
def _gradient_estimate(config, seed):
    """{(layer, role name): the gradient of the unseeded model} from a gradient-only plan on the same inputs."""
    from acm_gnn_amd.small import SmallPlan
    ops, xs, y, w = _small_problem(A.SMALL_CONFIGS[config][1] == 1)
    model = _small_model(config, seed)
    plan = SmallPlan(model, xs, ops, y, w, optimizer=None, update=False)
    plan.run()
    torch.cuda.synchronize()
    return {key: _host(g) for key, g in plan.grads.items()}


def _small_run(config, setting, slot=0):
    """(plan, optimizer, the role tensors, their counters): a model whose optimizer.state is in place for every role BEFORE the plan
    is built -- moments by adam_regimes.draw_moments around the gradient estimate, a distinct counter per role, layer and slot."""
    from acm_gnn_amd import FusedAdam, FusedAdamW
    from acm_gnn_amd.small import SmallPlan
    hp = A.SETTINGS[setting]
    ops, xs, y, w = _small_problem(A.SMALL_CONFIGS[config][1] == 1)
    estimate = _gradient_estimate(config, 3 + slot)
    model = _small_model(config, 3 + slot)
    opt = (FusedAdamW if hp[5] else FusedAdam)(model.parameters(), lr=hp[0], betas=(hp[1], hp[2]), eps=hp[3], weight_decay=hp[4])
    tensors = _role_tensors(model)
    steps = A.small_counters(len(tensors), slot)
    rng = np.random.default_rng(17 + slot)
    for (li, name, prm), s in zip(tensors, steps):
        m, v = A.draw_moments(rng, _host(prm), estimate[li, name], hp, s)
        opt.state[prm] = {"step": torch.tensor(float(s), device=DEV), "exp_avg": _dev(m).view(prm.shape),
                          "exp_avg_sq": _dev(v).view(prm.shape)}
    opt.also_advance = torch.full((1,), 100 + slot, dtype=torch.int64, device=DEV)
    assert SmallPlan.why_not(model, xs, ops, opt) is None
    plan = SmallPlan(model, xs, ops, y, w, optimizer=opt, keep_grads=True)
    for _, _, prm in tensors:                           # _bind_parameters took the seeded state as it is
        assert float(opt.state[prm]["step"]) in steps
    return plan, opt, tensors, steps


def _snapshot(opt, tensors):
    return [(_host(prm), _host(opt.state[prm]["exp_avg"]), _host(opt.state[prm]["exp_avg_sq"]), float(opt.state[prm]["step"]))
            for _, _, prm in tensors]


def _check_small(what, plan, opt, tensors, steps, before, hp, slot=0):
    after = _snapshot(opt, tensors)
    assert int(opt.also_advance) == 101 + slot
    worst = _Worst(what)
    quiet = warm = total = 0
    for (li, name, _), s, b, a in zip(tensors, steps, before, after):
        assert b[3] == s and a[3] == s + 1, (li, name, s, a[3])
        g = _host(plan.grads[li, name])
        if name == "struc_low":                         # rows the loss does not reach: gradient exactly 0 against warm moments
            quiet += int((g == 0).sum())
            warm += int(((g == 0) & (b[1] != 0)).sum())
            total += g.size
        worst.add(f"{li}.{name}", b[:3], g, a[:3], s, hp)
    if total:
        print(f"ADAMREG {what} | struc_low elements with g = 0: {quiet} of {total}, {warm} of them with m != 0")
        assert quiet > 0.5 * total and warm > 0.1 * total, (quiet, warm, total)
    worst.check()
    return after


def _used(timer):
    return {k.split("/")[0] for k in timer.events}


@pytest.mark.parametrize("setting", ["adam-wd5e-4", "adamw-wd1e-2"])
@pytest.mark.parametrize("config", list(A.SMALL_CONFIGS))
def test_small_graph_step_updates_per_element(config, setting):
    """acm_small_step with keep_grads: every role of both layers (34 tensors with four channels and LayerNorm, 14 with three and
    none), a training set of a tenth of the rows."""
    from acm_gnn_amd import functional as AF
    hp = A.SETTINGS[setting]
    plan, opt, tensors, steps = _small_run(config, setting)
    assert len(tensors) == (34 if config == "acmgcnp-k4-ln" else 14)
    before = _snapshot(opt, tensors)
    timer = AF.KernelTimer()
    AF.set_kernel_timer(timer)
    try:
        plan.run()
        torch.cuda.synchronize()
    finally:
        AF.set_kernel_timer(None)
    assert "small_step" in _used(timer), sorted(_used(timer))
    _check_small(f"small step {config} | {setting}", plan, opt, tensors, steps, before, hp)


def test_batched_small_graph_step_updates_per_element_with_hyper_parameters_per_slot():
    """Two slots through acm_small_batch_step, one Adam and one AdamW with different lr, eps and betas, all 68 counters distinct:
    each slot bit-identical to its own single-plan run from the same seeded state, and within K units of the reference."""
    from acm_gnn_amd import functional as AF
    from acm_gnn_amd.small import SmallBatch
    config, settings = "acmgcnp-k4-ln", ["adam-beta1-0-eps1e-3", "adamw-lr0.05"]
    single = [_small_run(config, s, slot) for slot, s in enumerate(settings)]
    batched = [_small_run(config, s, slot) for slot, s in enumerate(settings)]
    assert len({s for run in batched for s in run[3]}) == 68
    before = [_snapshot(opt, tensors) for _, opt, tensors, _ in batched]
    timer = AF.KernelTimer()
    AF.set_kernel_timer(timer)
    try:
        for plan, _, _, _ in single:
            plan.run()
        SmallBatch([plan for plan, _, _, _ in batched]).run()
        torch.cuda.synchronize()
    finally:
        AF.set_kernel_timer(None)
    assert {"small_step", "small_batch_step"} <= _used(timer), sorted(_used(timer))
    for slot, setting in enumerate(settings):
        plan_b, opt_b, tensors_b, steps = batched[slot]
        plan_s, opt_s, tensors_s, _ = single[slot]
        after = _check_small(f"small batch step, slot {slot} | {setting}", plan_b, opt_b, tensors_b, steps, before[slot], A.SETTINGS[setting], slot)
        assert torch.equal(plan_b.loss, plan_s.loss), slot
        for (li, name, _), got, want in zip(tensors_b, after, _snapshot(opt_s, tensors_s)):
            for x, y in zip(got[:3], want[:3]):
                assert np.array_equal(x.view(np.int32), y.view(np.int32)), (slot, li, name)
            assert got[3] == want[3] and torch.equal(plan_b.grads[li, name], plan_s.grads[li, name]), (slot, li, name)
