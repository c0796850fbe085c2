"""A batch of small-graph runs in the same six launches (acm_small_batch_step, small.SmallBatch, train.fit_batched): grid row k
of every launch is the single step of slot k, so every comparison here is exact (torch.equal) against the single entry points
(acm_small_step, acm_eval_metrics, acm_select_step, train.fit), which the existing tests pin against the float64 oracle."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from test_gpu_small import CONFIGS, DEV, _case, _model, _random_graph
from test_gpu_small_envelope import _direct_case

pytestmark = pytest.mark.gpu


def _run_of(case, f_in, classes, cfg, p_drop=0.0, seed=0, lr=0.01, wd=5e-4, decoupled=False, tr=None, drop_seed=0x1234ABCD5678):
    """(model, optimizer, training plan) of one run; the same arguments give the same initial state."""
    from acm_gnn_amd import FusedAdam, FusedAdamW, functional as AF, train as T
    from acm_gnn_amd.small import SmallPlan
    model = _model(case, f_in, classes, cfg, p_drop, seed=seed)
    if p_drop > 0:
        model.dropout_state = AF.DropoutState(torch.device(DEV), seed=drop_seed)
        model.dropout_state.step.fill_(5)
    opt = (FusedAdamW if decoupled else FusedAdam)(model.parameters(), lr=lr, weight_decay=wd)
    if p_drop > 0:
        opt.also_advance = model.dropout_state.step
    model.train()
    y = torch.from_numpy(case["y"]).to(DEV)
    tr = case["tr"] if tr is None else tr
    w = T.row_weights(torch.from_numpy(np.asarray(tr)).to(DEV), case["n"])
    assert SmallPlan.why_not(model, case["xs"], case["ops"], opt) is None
    return model, opt, SmallPlan(model, case["xs"], case["ops"], y, w, optimizer=opt)


def _state(model, opt, plan):
    out = {f"p.{k}": v.detach().clone() for k, v in model.state_dict().items()}
    for k, p in enumerate(model.parameters()):
        for name, v in opt.state.get(p, {}).items():
            if torch.is_tensor(v):
                out[f"opt.{k}.{name}"] = v.detach().clone()
    out.update(loss=plan.loss.clone(), logits=plan.logits.clone(), att1=plan.att1.clone(), att2=plan.att2.clone())
    ds = getattr(model, "dropout_state", None)
    if ds is not None:
        out["drop_step"] = ds.step.clone()
    return out


def _assert_same(a, b, what):
    assert a.keys() == b.keys(), what
    for k in a:
        assert torch.equal(a[k], b[k]) or (torch.isnan(a[k]).all() and torch.isnan(b[k]).all()), (what, k)


def _hub_case(cfg):
    adj = _random_graph(700, 30, 3, hub=700)
    rng = np.random.default_rng(8)
    x_np = (rng.random((700, 40)) < 0.05).astype(np.float32) * rng.uniform(0.5, 1.5, (700, 40)).astype(np.float32)
    x_np[:, 5] = rng.uniform(0.5, 1.5, 700)
    case = _direct_case(adj, x_np, 3, seed=11, s=cfg["s"])
    for h in (case["ops"].low, case["xs"].csr_t):
        assert h.chunk == 8 and h.max_degree >= 699 and h.max_degree > 64 * h.chunk and h.n_partial_slots % 16 == 0, h
    return case


SLOT_ARGS = [dict(p_drop=0.0, seed=1, lr=0.01, wd=5e-4, decoupled=False, drop_seed=11),
             dict(p_drop=0.5, seed=2, lr=0.03, wd=1e-3, decoupled=True, drop_seed=22),
             dict(p_drop=0.9, seed=3, lr=0.002, wd=0.0, decoupled=False, drop_seed=33)]


def _three(case, f_in, classes, cfg):
    rng = np.random.default_rng(5)
    return [_run_of(case, f_in, classes, cfg, tr=np.sort(rng.permutation(case["n"])[: case["n"] // (2 + k)]), **a)
            for k, a in enumerate(SLOT_ARGS)]


def test_one_slot_equals_the_single_step():
    from acm_gnn_amd.small import SmallBatch
    cfg = CONFIGS[2]
    case = _case(_random_graph(300, 10, 2), 64, 3, seed=11, s=cfg["s"])
    single, batched = _run_of(case, 64, 3, cfg, p_drop=0.5), _run_of(case, 64, 3, cfg, p_drop=0.5)
    b = SmallBatch([batched[2]])
    for step in range(5):
        single[2].run()
        b.run()
        torch.cuda.synchronize()
        _assert_same(_state(*single), _state(*batched), step)
    assert int(batched[0].dropout_state.step) == 10


@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[4], CONFIGS[1], CONFIGS[5]],
                         ids=["three_channels", "four_channels", "variant", "layernorm"])
@pytest.mark.parametrize("empty", [False, True], ids=["full", "empty_slots"])
def test_slots_equal_their_own_single_runs_and_share_nothing(cfg, empty, tune, monkeypatch):
    """Three runs that differ in split, seed, lr, weight decay, dropout (0 / 0.5 / 0.9) and Adam / AdamW on the chunk-8 hub graph
    (rows of several windows in the graph handle and the transposed feature handle: per-slot slots, counters, long3 / long4).
    ``empty``: four slots with 1 and 3 empty; the buffers of slot 1's former occupant do not change."""
    from acm_gnn_amd.small import SmallBatch, SmallPlan
    tune(chunk=8)
    monkeypatch.setattr(SmallPlan, "_operator", staticmethod(lambda ops: ops.low))
    case = _hub_case(cfg)
    singles, batched = _three(case, 40, 3, cfg), _three(case, 40, 3, cfg)
    if empty:
        singles, batched = singles[1:], batched[1:]     # slots 0 and 2: AdamW with dropout 0.5, Adam with dropout 0.9
        former = _run_of(case, 40, 3, cfg, p_drop=0.5, seed=9)
        b = SmallBatch([batched[0][2], former[2], batched[1][2]], n_slots=4)      # slot 3 is empty from the start
        b.run()
        for s in singles:
            s[2].run()
        b.set_slot(1, None)                             # ... and slot 1 from here on
        torch.cuda.synchronize()
        before, ws_before = _state(*former), former[2].workspace.clone()
    else:
        b = SmallBatch([r[2] for r in batched])
    for step in range(4):
        for s in singles:
            s[2].run()
        b.run()
    torch.cuda.synchronize()
    for k, (s, r) in enumerate(zip(singles, batched)):
        _assert_same(_state(*s), _state(*r), f"run {k}")
    if empty:
        _assert_same(before, _state(*former), "the former occupant of the empty slot")
        assert torch.equal(ws_before, former[2].workspace)


@pytest.mark.parametrize("n,classes", [(1, 1), (2, 8), (3, 1), (3, 8)])
def test_full_table_at_the_smallest_sizes(n, classes):
    from acm_gnn_amd import _lib
    from acm_gnn_amd.small import SmallBatch
    adj = sp.csr_matrix(np.ones((n, n), np.float32) - np.eye(n, dtype=np.float32))
    x_np = np.linspace(0.5, 1.5, n, dtype=np.float32).reshape(n, 1)
    cfg = CONFIGS[0]
    case = _direct_case(adj, x_np, classes, seed=3, s=0, tr=np.arange(n))
    singles = [_run_of(case, 1, classes, cfg, seed=k, lr=0.01 * (k + 1)) for k in range(32)]
    batched = [_run_of(case, 1, classes, cfg, seed=k, lr=0.01 * (k + 1)) for k in range(32)]
    b = SmallBatch([r[2] for r in batched])
    for _ in range(2):
        for s in singles:
            s[2].run()
        b.run()
    torch.cuda.synchronize()
    for k, (s, r) in enumerate(zip(singles, batched)):
        _assert_same(_state(*s), _state(*r), f"slot {k}")
    # 33 slots: refused before any launch
    lib = _lib.load()
    slots = (C.POINTER(_lib.SmallStep) * 33)(*[C.pointer(r[2].p) for r in batched], C.pointer(batched[0][2].p))
    plan = batched[0][2]
    st = lib.acm_small_batch_bind(plan.low.handle, plan.x.csr.handle, plan._xt.handle, 33, slots, b.table.data_ptr(), b.table.numel(), None)
    assert st == 4 and b"33" in lib.acm_last_error()
    st = lib.acm_small_batch_step(plan.low.handle, plan.x.csr.handle, plan._xt.handle, 33, C.byref(plan.p), b.table.data_ptr(), None)
    assert st == 4
    torch.cuda.synchronize()
    for k, (s, r) in enumerate(zip(singles, batched)):
        _assert_same(_state(*s), _state(*r), f"slot {k} after the refusals")


def test_capture_and_slot_hand_over():
    from acm_gnn_amd.small import SmallBatch
    cfg = CONFIGS[2]
    case = _case(_random_graph(300, 10, 2), 64, 3, seed=11, s=cfg["s"])
    singles, batched = _three(case, 64, 3, cfg), _three(case, 64, 3, cfg)
    other_s, other_b = _run_of(case, 64, 3, cfg, p_drop=0.5, seed=9, lr=0.02), _run_of(case, 64, 3, cfg, p_drop=0.5, seed=9, lr=0.02)
    b = SmallBatch([r[2] for r in batched])
    b.run()                                             # one eager step first (every kernel has run before the capture)
    for s in singles:
        s[2].run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # (a capture runs nothing)
        b.run()
    torch.cuda.synchronize()
    for k, (s, r) in enumerate(zip(singles, batched)):
        _assert_same(_state(*s), _state(*r), f"slot {k} after the capture")
    same = graph
    for _ in range(3):
        graph.replay()
        for s in singles:
            s[2].run()
    torch.cuda.synchronize()
    for k, (s, r) in enumerate(zip(singles, batched)):
        _assert_same(_state(*s), _state(*r), f"slot {k} after three replays")
    b.set_slot(1, other_b[2])                           # table bytes only
    assert graph is same
    for _ in range(3):
        graph.replay()
        for s in (singles[0], other_s, singles[2]):
            s[2].run()
    torch.cuda.synchronize()
    _assert_same(_state(*other_s), _state(*other_b), "the run that took slot 1")
    _assert_same(_state(*singles[0]), _state(*batched[0]), "slot 0")
    _assert_same(_state(*singles[2]), _state(*batched[2]), "slot 2")
    _assert_same(_state(*singles[1]), _state(*batched[1]), "the run that left slot 1 stands where it left")


def test_evaluation_pass_metrics_and_selection():
    from acm_gnn_amd import functional as AF, train as T
    from acm_gnn_amd.small import SmallBatch, SmallPlan
    cfg = CONFIGS[2]
    case = _case(_random_graph(300, 10, 2), 64, 3, seed=11, s=cfg["s"])
    n = case["n"]
    y = torch.from_numpy(case["y"]).to(DEV)
    y[17] = -1                                          # unlabeled: in no index set
    rng = np.random.default_rng(2)
    perm = np.setdiff1d(rng.permutation(n), [17], assume_unique=True)
    sets = [torch.from_numpy(np.sort(perm[a:b])).to(DEV) for a, b in ((0, 100), (100, 200), (200, 299))]
    w = T._set_weights(sets, y)
    assert float(w[:, 17].abs().sum()) == 0.0
    models = [_model(case, 64, 3, cfg, 0.0, seed=k) for k in range(3)]
    for m in models:
        m.eval()
    single = [SmallPlan(m, case["xs"], case["ops"]) for m in models]
    batched = [SmallPlan(m, case["xs"], case["ops"]) for m in models]
    b = SmallBatch(batched)
    b.run()
    for p in single:
        p.run()
    torch.cuda.synchronize()
    for k in range(3):
        assert torch.equal(single[k].logits, batched[k].logits) and torch.equal(single[k].att2, batched[k].att2), k
    va = int(sets[1][0])
    for plans in (single, batched):
        plans[0].logits[int(sets[2][0])] = torch.tensor([0.25, 0.25, 0.25], device=DEV)      # an arg-max tie
        plans[1].logits[va, 1] = float("nan")                                               # a NaN validation loss in slot 1
    metrics = AF.BatchMetrics(3, n, 3, 3, y)
    select = AF.BatchSelection("min_val_loss", 2, 6, 3, DEV)
    losses = [torch.full((), 0.5 + k, device=DEV) for k in range(3)]
    singles_sel = [AF.SelectionState("min_val_loss", 2, 6, DEV) for _ in range(3)]
    bufs = [AF.eval_metrics_buffers(n, 3, DEV) for _ in range(3)]
    for k in range(3):
        metrics.set_slot(k, batched[k].logits, w)
        select.set_slot(k, losses[k], metrics.out[k])
    metrics.flush(), select.flush()
    for epoch in range(5):
        for k in range(3):
            res = AF.eval_metrics(single[k].logits, y, w, 1, bufs[k])
            singles_sel[k].launch(losses[k], res)
        metrics.launch()
        select.launch()
        torch.cuda.synchronize()
        for k in range(3):
            a, r = bufs[k][0], metrics.out[k]
            assert torch.equal(a.nan_to_num(nan=-7.0), r.nan_to_num(nan=-7.0)), (epoch, k, a, r)
            assert torch.equal(singles_sel[k].ctrl, select.ctrl[k]) and torch.equal(singles_sel[k].best, select.best[k]), (epoch, k)
            assert torch.equal(singles_sel[k].history.nan_to_num(nan=-7.0), select.history[k].nan_to_num(nan=-7.0)), (epoch, k)
        for k in range(3):                              # a validation loss that rises every epoch: the window rule fires
            for plans in (single, batched):
                plans[k].logits[sets[1], y[sets[1]]] -= 1.0
    assert bool(torch.isnan(metrics.out[1][3])) and not bool(torch.isnan(metrics.out[0][3]))
    assert any(s for _, s in select.poll()) and select.poll()[1][1] is False      # a NaN never stops


@pytest.mark.parametrize("rule", ["min_val_loss", "max_val_acc"])
def test_fit_batched_is_fit_run_by_run(rule):
    from acm_gnn_amd import FusedAdam, functional as AF, train as T
    cfg = CONFIGS[2]
    case = _case(_random_graph(300, 10, 2), 64, 3, seed=11, s=cfg["s"])
    n = case["n"]
    y = torch.from_numpy(case["y"]).to(DEV)
    # The labels are random, so any learning run's validation loss soon turns upwards and the window rule stops it within a few
    # epochs (which one depends on the step size and the dropout noise).  Run 2 has lr = 0 and no dropout: its validation loss
    # is the same number every epoch, equal is not greater, and it uses its whole budget.
    lrs = [0.5, 0.001, 0.0, 0.002, 0.05]

    def make():
        runs = []
        r = np.random.default_rng(4)
        for k, lr in enumerate(lrs):
            perm = r.permutation(n)
            sets = [torch.from_numpy(np.sort(perm[a:b])).to(DEV) for a, b in ((0, 120), (120, 210), (210, 300))]
            model = _model(case, 64, 3, cfg, 0.5 if k % 2 else 0.0, seed=k)
            if k % 2:
                model.dropout_state = AF.DropoutState(torch.device(DEV), seed=100 + k)
            runs.append((model, FusedAdam(model.parameters(), lr=lr, weight_decay=5e-4), *sets))
        return runs

    ref = [T.fit(m, o, case["xs"], case["ops"], y, tr, va, te, 24, rule=rule, early_stopping=3, use_graph=True, sync_every=4)
           for m, o, tr, va, te in make()]
    lengths = [len(h) for _, h in ref]
    if rule == "min_val_loss":
        assert min(lengths) < 24 and max(lengths) == 24 and len(set(lengths)) >= 3, lengths     # early stops at different
                                                                                               # epochs, and one whole budget
    got = T.fit_batched(make(), case["xs"], case["ops"], y, 24, rule=rule, early_stopping=3, batch=2, sync_every=4)
    assert T.fit_batched.last_refusal is None
    for k, ((sel_r, hist_r), (sel_g, hist_g)) in enumerate(zip(ref, got)):
        assert sel_r == sel_g and hist_r == hist_g, (k, len(hist_r), len(hist_g))
