"""A batch of small-graph runs on DIFFERENT graphs in the same six launches (acm_small_batch_step_graphs,
small.SmallGraphBatch, train.fit_batched_graphs): grid row k of every launch is the single step of slot k on slot k's own
handles -- the launch is as wide as the widest graph's, the slot loops with its own widths -- so every comparison here is exact
(torch.equal) against the single entry points (acm_small_step, acm_eval_metrics, acm_select_step, train.fit), which the
existing tests pin against the float64 oracle."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

import test_gpu_small_batch as SB
from test_gpu_small import CONFIGS, DEV, _case, _model, _random_graph
from test_gpu_small_batch import SLOT_ARGS, _assert_same, _hub_case, _run_of, _state
from test_gpu_small_envelope import _direct_case
from test_gpu_small_hidden import _model as _model_hidden

pytestmark = pytest.mark.gpu
ESHAPE, EINVAL = 2, 1


def _features(seed, density, n=700, f_in=40):
    rng = np.random.default_rng(seed)
    return (rng.random((n, f_in)) < density).astype(np.float32) * rng.uniform(0.5, 1.5, (n, f_in)).astype(np.float32)


def _plain_case(cfg, graph_seed=3, seed=21, n=700):
    """No hub, sparse features, one node without any."""
    x_np = _features(seed, 0.05, n)
    x_np[11] = 0.0
    return _direct_case(_random_graph(n, 30, graph_seed), x_np, 3, seed=seed, s=cfg["s"])


def _mid_case(cfg):
    """A mid-sized hub (250 neighbours) and features dense enough that every feature row and most node rows are cut."""
    return _direct_case(_random_graph(700, 30, 4, hub=250), _features(31, 0.3), 3, seed=31, s=cfg["s"])


def _info(h):
    from acm_gnn_amd import _lib
    info = _lib.CsrInfo()
    _lib.check(_lib.load().acm_csr_info(h.handle, C.byref(info)), "acm_csr_info")
    return info


def _own_grids(plan):
    from acm_gnn_amd import _lib
    g = _lib.SmallBatchGrids()
    _lib.check(_lib.load().acm_small_batch_grids(plan.low.handle, plan.x.csr.handle, plan._xt.handle if plan._xt is not None else None,
                                                 C.byref(plan.p), C.byref(g)), "acm_small_batch_grids")
    return (g.proj, g.wide, g.graph, g.item_blocks, g.red_blocks)


def _runs_on(cases, cfg, f_in=40, classes=3):
    """Run k on cases[k] with SLOT_ARGS[k % 3] and its own split."""
    rng = np.random.default_rng(5)
    return [_run_of(case, f_in, classes, cfg, tr=np.sort(rng.permutation(case["n"])[: case["n"] // (2 + k % 3)]), **SLOT_ARGS[k % 3])
            for k, case in enumerate(cases)]


def _handles(case, train=True):
    from acm_gnn_amd.small import SmallGraphBatch
    return SmallGraphBatch.handles_of(case["xs"], case["ops"], train)


@pytest.fixture
def chunk8(tune, monkeypatch):
    """Work items of 8 entries and the plans on ops.low itself, as the hub test of test_gpu_small_batch.py runs."""
    from acm_gnn_amd.small import SmallPlan
    tune(chunk=8)
    monkeypatch.setattr(SmallPlan, "_operator", staticmethod(lambda ops: ops.low))


@pytest.mark.parametrize("cfg,hidden", [(CONFIGS[0], 64), (CONFIGS[4], 64), (CONFIGS[1], 64), (CONFIGS[5], 64), (CONFIGS[4], 32)],
                         ids=["three_channels", "four_channels", "variant", "layernorm", "hidden_32"])
def test_slots_on_different_graphs_equal_their_own_single_steps(cfg, hidden, chunk8, monkeypatch):
    """Slots hub / plain / mid: three graphs of 700 rows with their own features, labels and splits -- the widest graph is
    not last and the narrowest not first -- and hyper-parameters, dropout and Adam / AdamW per SLOT_ARGS."""
    from acm_gnn_amd.small import SmallBatch, SmallGraphBatch
    if hidden != 64:
        monkeypatch.setattr(SB, "_model", lambda case, f_in, classes, cfg, p_drop, seed=0:
                            _model_hidden(case, f_in, classes, cfg, p_drop, hidden=hidden, seed=seed))
    cases = [_hub_case(cfg), _plain_case(cfg), _mid_case(cfg)]
    assert int((cases[1]["x_np"] != 0).sum(1).min()) == 0 and int((cases[0]["x_np"] != 0).sum(0).max()) == 700
    # not vacuous: the work-item counts of the operator, the features and the transposed features differ between slots, and
    # with them the width of every launch
    for name, pick in (("operator", lambda c: c["ops"].low), ("x", lambda c: c["xs"].csr), ("x_t", lambda c: c["xs"].csr_t)):
        counts = [int(_info(pick(c)).n_items) for c in cases]
        assert len(set(counts)) >= 2, (name, counts)
    singles, batched = _runs_on(cases, cfg), _runs_on(cases, cfg)
    assert all(r[2].hidden == hidden for r in batched)
    own = [_own_grids(r[2]) for r in batched]
    for launch in range(4):                              # proj, wide, graph, item_blocks (red_blocks: the hidden width's)
        assert len({g[launch] for g in own}) >= 2, (launch, own)
    assert "feature" in SmallBatch.why_not([r[2] for r in batched])
    b = SmallGraphBatch([r[2] for r in batched])
    env = (b.grids.proj, b.grids.wide, b.grids.graph, b.grids.item_blocks, b.grids.red_blocks)
    assert env == tuple(max(g[i] for g in own) for i in range(5)) and env != own[2] and env != own[1]
    for step in range(4):
        for s in singles:
            s[2].run()
        b.run()
    torch.cuda.synchronize()
    for k, (s, r) in enumerate(zip(singles, batched)):
        _assert_same(_state(*s), _state(*r), f"slot {k}")


def test_an_envelope_wider_than_every_occupant_and_empty_slots(chunk8):
    """The launches are the hub graph's, the occupants stand on two plain graphs: every workgroup past a slot's own width
    returns.  Four slots, 1 and 3 empty; the buffers of slot 1's former occupant do not change."""
    from acm_gnn_amd.small import SmallGraphBatch
    cfg = CONFIGS[4]
    hub, plains = _hub_case(cfg), [_plain_case(cfg), _plain_case(cfg, graph_seed=6, seed=22)]
    singles, batched = _runs_on(plains, cfg), _runs_on(plains, cfg)
    former = _run_of(plains[0], 40, 3, cfg, p_drop=0.5, seed=9)
    b = SmallGraphBatch([batched[0][2], former[2], batched[1][2]], n_slots=4, handles=[_handles(hub)])
    env = (b.grids.proj, b.grids.wide, b.grids.graph, b.grids.item_blocks)
    for r in batched:                                   # (launch 1 walks the features' rows, which the hub does not lengthen)
        own = _own_grids(r[2])[:4]
        assert own[0] <= env[0] and all(o < e for o, e in zip(own[1:], env[1:])), (own, env)
    b.run()
    for s in singles:
        s[2].run()
    b.set_slot(1, None)
    torch.cuda.synchronize()
    before, ws_before = _state(*former), former[2].workspace.clone()
    for step in range(4):
        for s in singles:
            s[2].run()
        b.run()
    torch.cuda.synchronize()
    for k, (s, r) in enumerate(zip(singles, batched)):
        _assert_same(_state(*s), _state(*r), f"run {k}")
    _assert_same(before, _state(*former), "the former occupant of the empty slot")
    assert torch.equal(ws_before, former[2].workspace)


def test_a_graph_outside_the_envelope_is_refused_and_the_table_stays(chunk8):
    from acm_gnn_amd import _lib
    from acm_gnn_amd.small import SmallGraphBatch
    cfg = CONFIGS[0]
    lib = _lib.load()
    plain, hub = _plain_case(cfg), _hub_case(cfg)
    singles, batched = _runs_on([plain, plain], cfg), _runs_on([plain, plain], cfg)
    wide = _run_of(hub, 40, 3, cfg, seed=4)
    b = SmallGraphBatch([r[2] for r in batched])         # the envelope is the plain graph's own grids
    b.run()
    for s in singles:
        s[2].run()
    torch.cuda.synchronize()
    table = b.table.clone()
    # the C entry: ACM_ESHAPE, nothing written
    a = (C.c_void_p * 2)(batched[0][2].low.handle.value, wide[2].low.handle.value)
    x = (C.c_void_p * 2)(batched[0][2].x.csr.handle.value, wide[2].x.csr.handle.value)
    xt = (C.c_void_p * 2)(batched[0][2]._xt.handle.value, wide[2]._xt.handle.value)
    slots = (C.POINTER(_lib.SmallStep) * 2)(C.pointer(batched[0][2].p), C.pointer(wide[2].p))
    st = lib.acm_small_batch_bind_graphs(2, a, x, xt, slots, C.byref(b.grids), b.table.data_ptr(), b.table.numel(), None)
    assert st == ESHAPE and b"workgroups" in lib.acm_last_error() and b"slot 1" in lib.acm_last_error(), lib.acm_last_error()
    torch.cuda.synchronize()
    assert torch.equal(table, b.table)
    # the class: the library's message, the slot keeps its run
    with pytest.raises(RuntimeError, match="ACM_ESHAPE|workgroups"):
        b.set_slot(1, wide[2])
    assert b.plans[1] is batched[1][2] and torch.equal(table, b.table)
    # a graph of 699 rows: the row-count message, from the class and from the C entry
    short = _run_of(_plain_case(cfg, n=699), 40, 3, cfg, seed=5)
    with pytest.raises(ValueError, match="699 and 700 rows"):
        b.set_slot(1, short[2])
    a[1], x[1], xt[1] = short[2].low.handle.value, short[2].x.csr.handle.value, short[2]._xt.handle.value
    slots[1] = C.pointer(short[2].p)
    st = lib.acm_small_batch_bind_graphs(2, a, x, xt, slots, C.byref(b.grids), b.table.data_ptr(), b.table.numel(), None)
    assert st == EINVAL and b"n_rows" in lib.acm_last_error() and b"disagree" in lib.acm_last_error(), lib.acm_last_error()
    with pytest.raises(ValueError, match="rows"):
        SmallGraphBatch([batched[0][2]], n_slots=2, handles=[_handles(dict(xs=short[2].x, ops=short[2].ops))])
    torch.cuda.synchronize()
    assert torch.equal(table, b.table)
    # the previous binding still replays correctly
    for step in range(2):
        for s in singles:
            s[2].run()
        b.run()
    torch.cuda.synchronize()
    for k, (s, r) in enumerate(zip(singles, batched)):
        _assert_same(_state(*s), _state(*r), f"slot {k} after the refusals")


def test_capture_and_slot_hand_over_across_graphs(chunk8):
    """A captured step whose envelope includes the hub graph, with plain graphs in both slots; slot 1 then passes to a run on
    the hub graph by table bytes, and the same graph object keeps replaying."""
    from acm_gnn_amd.small import SmallGraphBatch
    cfg = CONFIGS[4]
    plains, hub = [_plain_case(cfg), _plain_case(cfg, graph_seed=6, seed=22)], _hub_case(cfg)
    singles, batched = _runs_on(plains, cfg), _runs_on(plains, cfg)
    other_s, other_b = _run_of(hub, 40, 3, cfg, p_drop=0.5, seed=9, lr=0.02), _run_of(hub, 40, 3, cfg, p_drop=0.5, seed=9, lr=0.02)
    b = SmallGraphBatch([r[2] for r in batched], handles=[_handles(hub)])
    b.run()                                             # one eager step first (every kernel has run before the capture)
    for s in singles:
        s[2].run()
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # (a capture runs nothing)
        b.run()
    torch.cuda.synchronize()
    for _ in range(3):
        graph.replay()
        for s in singles:
            s[2].run()
    torch.cuda.synchronize()
    for k, (s, r) in enumerate(zip(singles, batched)):
        _assert_same(_state(*s), _state(*r), f"slot {k} after three replays")
    b.set_slot(1, other_b[2])                           # table bytes only: a run on ANOTHER graph, wider in every launch
    assert all(o >= p for o, p in zip(_own_grids(other_b[2]), _own_grids(batched[1][2])))
    for _ in range(3):
        graph.replay()
        for s in (singles[0], other_s):
            s[2].run()
    torch.cuda.synchronize()
    _assert_same(_state(*other_s), _state(*other_b), "the run on the hub graph that took slot 1")
    _assert_same(_state(*singles[0]), _state(*batched[0]), "slot 0")
    _assert_same(_state(*singles[1]), _state(*batched[1]), "the run that left slot 1 stands where it left")


def test_evaluation_pass_metrics_and_selection_with_per_slot_labels(chunk8):
    from acm_gnn_amd import functional as AF, train as T
    from acm_gnn_amd.small import SmallGraphBatch, SmallPlan
    cfg = CONFIGS[4]
    cases = [_hub_case(cfg), _plain_case(cfg), _mid_case(cfg)]
    n = 700
    ys = [torch.from_numpy(c["y"]).to(DEV) for c in cases]
    assert not torch.equal(ys[0], ys[1]) and not torch.equal(ys[1], ys[2])
    ys[1][17] = -1                                      # unlabeled in slot 1 alone: in none of its index sets
    ws = []
    for k in range(3):
        perm = np.setdiff1d(np.random.default_rng(40 + k).permutation(n), [17], assume_unique=True)
        sets = [torch.from_numpy(np.sort(perm[a:b])).to(DEV) for a, b in ((0, 250 + 10 * k), (250 + 10 * k, 480), (480, 699))]
        ws.append(T._set_weights(sets, ys[k]))
    models = [_model(c, 40, 3, cfg, 0.0, seed=k) for k, c in enumerate(cases)]
    for m in models:
        m.eval()
    single = [SmallPlan(m, c["xs"], c["ops"]) for m, c in zip(models, cases)]
    batched = [SmallPlan(m, c["xs"], c["ops"]) for m, c in zip(models, cases)]
    b = SmallGraphBatch(batched)
    assert b.grids.item_blocks == 0
    b.run()
    for p in single:
        p.run()
    torch.cuda.synchronize()
    for k in range(3):
        assert torch.equal(single[k].logits, batched[k].logits) and torch.equal(single[k].att2, batched[k].att2), k
        assert torch.equal(single[k].att1, batched[k].att1), k
    metrics = AF.BatchMetrics(3, n, 3, 3, ys[0])
    select = AF.BatchSelection("min_val_loss", 2, 6, 3, DEV)
    losses = [torch.full((), 0.5 + k, device=DEV) for k in range(3)]
    singles_sel = [AF.SelectionState("min_val_loss", 2, 6, DEV) for _ in range(3)]
    bufs = [AF.eval_metrics_buffers(n, 3, DEV) for _ in range(3)]
    metrics.set_slot(0, batched[0].logits, ws[0])        # the default: the shared tensor (slot 0's own here)
    for k in (1, 2):
        metrics.set_slot(k, batched[k].logits, ws[k], ys[k])
    with pytest.raises(ValueError, match="labels"):
        metrics.set_slot(2, batched[2].logits, ws[2], ys[2][:-1])
    for k in range(3):
        select.set_slot(k, losses[k], metrics.out[k])
    metrics.flush(), select.flush()
    for epoch in range(4):
        for k in range(3):
            res = AF.eval_metrics(single[k].logits, ys[k], ws[k], 1, bufs[k])
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
            rows = torch.nonzero(ws[k][1]).flatten()
            for plans in (single, batched):
                plans[k].logits[rows, ys[k][rows]] -= 1.0
    # the slots were judged on different labels: slot 1 on slot 0's labels gives other numbers
    other = AF.eval_metrics_buffers(n, 3, DEV)
    AF.eval_metrics(single[1].logits, ys[0], ws[1], 1, other)
    torch.cuda.synchronize()
    assert not torch.equal(other[0], metrics.out[1])
    assert any(s for _, s in select.poll())


def _tiny(n, kind, classes):
    """Two distinct graphs per size: ``kind`` 0 the complete graph, 1 the path (n = 1: no edge either way, other features)."""
    full = np.ones((n, n), np.float32) - np.eye(n, dtype=np.float32)
    path = np.diag(np.ones(n - 1, np.float32), 1) + np.diag(np.ones(n - 1, np.float32), -1) if n > 1 else full
    x_np = np.linspace(0.5, 1.5, n, dtype=np.float32).reshape(n, 1) * (1.0 + kind)
    return _direct_case(sp.csr_matrix(path if kind else full), x_np, classes, seed=3 + kind, s=0, tr=np.arange(n))


@pytest.mark.parametrize("n,classes", [(1, 1), (1, 8), (3, 1), (3, 8)])
def test_full_table_at_the_smallest_sizes_on_two_graphs(n, classes):
    from acm_gnn_amd.small import SmallGraphBatch
    cfg = CONFIGS[0]
    cases = [_tiny(n, 0, classes), _tiny(n, 1, classes)]
    singles = [_run_of(cases[k % 2], 1, classes, cfg, seed=k, lr=0.01 * (k + 1)) for k in range(32)]
    batched = [_run_of(cases[k % 2], 1, classes, cfg, seed=k, lr=0.01 * (k + 1)) for k in range(32)]
    assert batched[0][2].low is not batched[1][2].low and batched[0][2].x is not batched[1][2].x
    b = SmallGraphBatch([r[2] for r in batched])
    for _ in range(2):
        for s in singles:
            s[2].run()
        b.run()
    torch.cuda.synchronize()
    for k, (s, r) in enumerate(zip(singles, batched)):
        _assert_same(_state(*s), _state(*r), f"slot {k}")


@pytest.mark.parametrize("rule", ["min_val_loss", "max_val_acc"])
def test_fit_batched_graphs_is_fit_run_by_run(rule):
    """5 runs on 3 graphs in 2 slots: a slot passes from graph to graph under one captured epoch."""
    from acm_gnn_amd import FusedAdam, functional as AF, train as T
    cfg = CONFIGS[2]
    cases = [_case(_random_graph(300, 6 + 6 * g, 2 + g), 64, 3, seed=11 + g, density=0.01 * (g + 1), s=cfg["s"]) for g in range(3)]
    ys = [torch.from_numpy(c["y"]).to(DEV) for c in cases]
    lrs = [0.5, 0.001, 0.0, 0.002, 0.05]                # (run 2: lr = 0 and no dropout, it uses its whole budget)

    def make():
        runs = []
        r = np.random.default_rng(4)
        for k, lr in enumerate(lrs):
            case = cases[k % 3]
            perm = r.permutation(300)
            sets = [torch.from_numpy(np.sort(perm[a:b])).to(DEV) for a, b in ((0, 120), (120, 210), (210, 300))]
            model = _model(case, 64, 3, cfg, 0.5 if k % 2 else 0.0, seed=k)
            if k % 2:
                model.dropout_state = AF.DropoutState(torch.device(DEV), seed=100 + k)
            runs.append((model, FusedAdam(model.parameters(), lr=lr, weight_decay=5e-4), case["xs"], case["ops"], ys[k % 3], *sets))
        return runs

    ref = [T.fit(m, o, x, a, y, tr, va, te, 12, rule=rule, early_stopping=3, use_graph=True, sync_every=4)
           for m, o, x, a, y, tr, va, te in make()]
    got = T.fit_batched_graphs(make(), 12, rule=rule, early_stopping=3, batch=2, sync_every=4)
    assert T.fit_batched_graphs.last_refusal is None
    for k, ((sel_r, hist_r), (sel_g, hist_g)) in enumerate(zip(ref, got)):
        assert sel_r == sel_g and hist_r == hist_g, (k, len(hist_r), len(hist_g))
    assert len(ref[2][1]) == 12
