"""The fused small-graph step (acm_small_step: csrc/acm_small.hip, acm_gnn_amd/small.py) at the edges of its envelope, with
the comparisons and tolerances of tests/test_gpu_small.py (loss, logits and every gradient of both layers against the
float64 oracle; whole runs against the general path; bit-identical replays):

  * the ceiling graph of 16 384 nodes, whose work list is longer than the 16 384 waves of the wide launches (2, 5), so
    waves take a second item; with a row of several windows of pieces in the graph handle and in the transposed feature
    handle (launch 6), isolated nodes, a raw self-loop, a feature on every node and feature columns that are zero
    everywhere -- one step, whole training runs eager and captured, the evaluation pass;
  * rows of several windows at small size (chunk 8), up to the 256 pieces of a row of sixteen windows;
  * every class count 1 .. 8 (columns padded to 8, layer 2's LayerNorm over C entries);
  * graphs of one to three nodes, one-feature inputs;
  * the boundaries: 16 384 rows and 8 classes are taken, 16 385 rows and 9 classes are not.

Each test first asserts that its inputs reach the path it is about (handle statistics of the handles the kernels walk)."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import acm_oracle as O
from test_gpu_small import (CONFIGS, DEV, GRAPHS, _case, _check_one_step, _filters64, _model, _random_graph, _runs_agree)

pytestmark = pytest.mark.gpu
N_MAX = 16384
HUB_BIG, HUB_MID = 4099, 11777                        # rows of ~9 000 (three windows at chunk 128) and ~1 500 (one window)
ISOLATED = np.arange(N_MAX - 50, N_MAX)               # no edge at all: A + I holds the self-loop only
F_FULL, F_ZERO = 17, (0, 130, 263)                    # a feature on every node; feature columns that are zero everywhere
F_IN = 264


def _cfg_id(c):
    return f"{c['mt']}_v{c['v']}s{c['s']}ln{int(c['ln'])}"


def _direct_case(adj, x_np, classes, seed, s, tr=None):
    """What tests/test_gpu_small.py's _case builds, for inputs that helper would change (it clears node 3's features and
    trains on n // 2 rows): the features as given, ``tr`` (default: a random half) as the training rows."""
    from acm_gnn_amd import SparseFeatures, data as D
    from acm_gnn_amd.distributed import make_sharded_operators
    n = adj.shape[0]
    rng = np.random.default_rng(seed)
    y = rng.integers(0, classes, n)
    if tr is None:
        tr = np.sort(rng.permutation(n)[: n // 2])
    low, deg = D.build_filters(adj)
    ops = make_sharded_operators(low, deg, torch.device(DEV), with_structure=bool(s))
    xs = SparseFeatures.from_scipy(sp.csr_matrix(x_np), DEV)
    return dict(adj=adj, low=low, deg=deg, ops=ops, x_np=x_np, xs=xs, y=y, tr=tr, n=n)


def _ceiling_graph(n, seed=16384):
    """A power-law background of average degree ~24, the two hubs, the isolated nodes and a raw self-loop (node 7)."""
    rng = np.random.default_rng(seed)
    m = n * 24 // 2
    w = 1.0 / (np.arange(n) + 5.0) ** 0.7
    r, c = rng.choice(n, m, p=w / w.sum()), rng.integers(0, n, m)
    pool = np.setdiff1d(np.arange(n), np.r_[ISOLATED, HUB_BIG, HUB_MID])
    r = np.r_[r, np.full(9000, HUB_BIG), np.full(1500, HUB_MID)]
    c = np.r_[c, rng.choice(pool, 9000, replace=False), rng.choice(pool, 1500, replace=False)]
    a = sp.csr_matrix((np.ones(len(r), np.float32), (r, c)), shape=(n, n))
    a = ((a + a.T) > 0).astype(np.float32).tocsr()
    keep = np.ones(n, np.float32)
    keep[ISOLATED[ISOLATED < n]] = 0.0
    a = (sp.diags(keep) @ a @ sp.diags(keep)).tocsr()
    a.setdiag(0)
    a.eliminate_zeros()
    a = a.tolil()
    a[7, 7] = 1.0
    return a.tocsr()


def _ceiling_features(n, seed=264):
    rng = np.random.default_rng(seed)
    x = (rng.random((n, F_IN)) < 0.02).astype(np.float32) * rng.uniform(0.5, 1.5, (n, F_IN)).astype(np.float32)
    x[:, F_FULL] = rng.uniform(0.5, 1.5, n).astype(np.float32)
    x[:, list(F_ZERO)] = 0.0
    return x


@functools.lru_cache(maxsize=None)
def _ceiling_inputs(n=N_MAX):
    return _ceiling_graph(n), _ceiling_features(n)


@functools.lru_cache(maxsize=None)
def _ceiling_case(s, classes):
    adj, x_np = _ceiling_inputs()
    return _direct_case(adj, x_np, classes, seed=11, s=s)


def _assert_ceiling_handles(case):
    """The handles the six launches walk: more items than the wide launches have waves, a row of several windows in the
    graph handle (launches 2-5) and in the transposed feature handle (launch 6)."""
    from acm_gnn_amd.small import SmallPlan
    low, xt = case["ops"].low, case["xs"].csr_t
    assert SmallPlan._operator(case["ops"]) is low, "the fused step would walk a re-chunked copy"
    assert low.n_rows == N_MAX and low.n_items > N_MAX and low.max_degree > 64 * low.chunk, low
    assert low.n_long_rows >= 2 and low.n_partial_slots % 16 == 0, low
    assert xt.n_rows == F_IN and xt.max_degree == N_MAX and xt.max_degree > 64 * xt.chunk, xt
    x_np = case["x_np"]
    assert (x_np[:, list(F_ZERO)] == 0).all() and (x_np[:, F_FULL] != 0).all()
    assert case["adj"][ISOLATED].nnz == 0 and case["adj"][7, 7] == 1.0


# 8 classes with the structure channel, 6 (citeseer's count) without
CEILING = [(CONFIGS[0], 6), (CONFIGS[3], 8), (CONFIGS[4], 8), (CONFIGS[6], 6)]


@pytest.mark.parametrize("p_drop", [0.0, 0.5], ids=["nodrop", "drop"])
@pytest.mark.parametrize("cfg,classes", CEILING, ids=[f"{_cfg_id(c)}_C{k}" for c, k in CEILING])
def test_ceiling_graph_one_step_matches_the_oracle(cfg, classes, p_drop):
    case = _ceiling_case(cfg["s"], classes)
    _assert_ceiling_handles(case)
    _check_one_step(case, F_IN, classes, cfg, p_drop)


@pytest.mark.parametrize("p_drop", [0.0, 0.5], ids=["nodrop", "drop"])
@pytest.mark.parametrize("cfg", CONFIGS, ids=_cfg_id)
def test_rows_of_several_windows_at_small_size(cfg, p_drop, tune, monkeypatch):
    """chunk 8 on a 700-node graph whose node 0 has 699 neighbours: three windows of pieces for that row in the graph
    handle and in the transposed feature handle (a feature on every node), every other row of more than 8 neighbours an
    ordinary long row.  SmallPlan._operator would re-chunk the graph handle to 128 (one window): here the kernels walk
    the chunk-8 handle itself."""
    from acm_gnn_amd.small import SmallPlan
    tune(chunk=8)
    monkeypatch.setattr(SmallPlan, "_operator", staticmethod(lambda ops: ops.low))
    adj = _random_graph(700, 30, 3, hub=700)
    rng = np.random.default_rng(8)
    x_np = (rng.random((700, 40)) < 0.05).astype(np.float32) * rng.uniform(0.5, 1.5, (700, 40)).astype(np.float32)
    x_np[:, 5] = rng.uniform(0.5, 1.5, 700)
    case = _direct_case(adj, x_np, 3, seed=11, s=cfg["s"])
    for h in (case["ops"].low, case["xs"].csr_t):
        assert h.chunk == 8 and h.max_degree >= 699 and h.max_degree > 64 * h.chunk and h.n_partial_slots % 16 == 0, h
    _check_one_step(case, 40, 3, cfg, p_drop)


def test_rows_of_sixteen_windows_are_exact_and_deterministic(tune, monkeypatch):
    """The most pieces a row can take: 16 windows x 16 = 256 (chunk 8, a row of 4 200 neighbours in the graph handle and
    in the transposed feature handle) -- where the arrival order of the pieces varies most.  One step against the oracle,
    then two captured ten-step runs bit-identical to the eager one."""
    from acm_gnn_amd import FusedAdamW, functional as AF, train as T
    from acm_gnn_amd.small import SmallPlan
    tune(chunk=8)
    monkeypatch.setattr(SmallPlan, "_operator", staticmethod(lambda ops: ops.low))
    n, cfg = 4200, CONFIGS[3]
    adj = _random_graph(n, 8, 5, hub=n)
    rng = np.random.default_rng(9)
    x_np = (rng.random((n, 24)) < 0.1).astype(np.float32)
    x_np[:, 2] = 1.0
    case = _direct_case(adj, x_np, 4, seed=5, s=1)
    for h in (case["ops"].low, case["xs"].csr_t):
        assert h.chunk == 8 and h.max_degree >= n - 1 and h.max_degree > 15 * 2 * 16 * h.chunk, h     # 16 windows
    # the full feature column: 256 pieces; the other 23 (~420 entries each): one window of 16
    assert case["xs"].csr_t.n_partial_slots == 256 + 23 * 16, case["xs"].csr_t
    _check_one_step(case, 24, 4, cfg, 0.5)
    y = torch.from_numpy(case["y"]).to(DEV)
    w = T.row_weights(torch.from_numpy(case["tr"]).to(DEV), n)

    def run(use_graph):
        model = _model(case, 24, 4, cfg, 0.6, seed=3)
        model.dropout_state = AF.DropoutState(torch.device(DEV), seed=77)
        opt = FusedAdamW(model.parameters(), lr=0.02, weight_decay=5e-3)
        step = T.TrainStep(model, opt, case["xs"], case["ops"], y, w, use_graph=use_graph)
        assert step.small is not None and step.small.low.chunk == 8, step.small_refused
        return [float(step()) for _ in range(10)], [p.detach().clone() for p in model.parameters()]

    la, pa = run(False)
    for use_graph in (True, True):
        lb, pb = run(use_graph)
        assert la == lb
        assert all(torch.equal(u, v) for u, v in zip(pa, pb))


@pytest.mark.parametrize("classes", range(1, 9))
@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[3]], ids=_cfg_id)
def test_every_class_count(cfg, classes):
    """C = 1 .. 8 on the graph with long rows: columns past C are padded lanes, layer 2's LayerNorm averages over C.  One
    class: log_softmax is identically 0, so the loss and every gradient are exactly zero in the oracle and must be here."""
    adj, f_in, _ = GRAPHS["pieces"]()
    case = _case(adj, f_in, classes, seed=11, s=cfg["s"])
    assert case["ops"].low.n_long_rows > 0
    plan, loss, ref_loss, ref_grads = _check_one_step(case, f_in, classes, cfg, 0.5)
    if classes == 1:
        assert loss == ref_loss == 0.0
        for (li, name), g in plan.grads.items():
            if li == 1:
                assert float(g.abs().max()) == 0.0 and float(ref_grads[f"gcns.1.{name}"].abs().max()) == 0.0, name


def _tiny_adj(n):
    a = sp.lil_matrix((n, n), dtype=np.float32)
    if n >= 2:
        a[0, 1] = a[1, 0] = 1.0                       # n = 3: node 2 is isolated
    return a.tocsr()


@pytest.mark.parametrize("p_drop", [0.0, 0.5], ids=["nodrop", "drop"])
@pytest.mark.parametrize("f_in", [1, 40])
@pytest.mark.parametrize("cfg", [CONFIGS[0], CONFIGS[3]], ids=_cfg_id)
@pytest.mark.parametrize("n", [1, 2, 3])
def test_smallest_graphs(n, cfg, f_in, p_drop):
    """Graphs of one to three nodes, every node a training row, one-feature and wider inputs."""
    rng = np.random.default_rng(n * 100 + f_in)
    if f_in == 1:
        x_np = rng.uniform(0.5, 1.5, (n, 1)).astype(np.float32)
    else:
        x_np = (rng.random((n, f_in)) < 0.3).astype(np.float32) * rng.uniform(0.5, 1.5, (n, f_in)).astype(np.float32)
        x_np[:, 0] = 1.0
    case = _direct_case(_tiny_adj(n), x_np, 3, seed=n, s=cfg["s"], tr=np.arange(n))
    assert case["ops"].low.n_rows == n and case["ops"].low.n_items == n
    _check_one_step(case, f_in, 3, cfg, p_drop)


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
def test_ceiling_training_run_equals_the_general_path(use_graph):
    """Ten steps of TrainStep on the ceiling graph (ACMII + structure + LayerNorm, dropout, AdamW) against
    TrainStep(small_step=False) -- the general path runs its input pipeline on the same rows of several windows -- with
    the checks of test_gpu_small.py::test_training_run_equals_the_general_path; under capture, a second small-path run
    is bit-identical to the first."""
    from acm_gnn_amd import FusedAdamW, functional as AF, train as T
    cfg, classes, p_drop = CONFIGS[3], 8, 0.5
    case = _ceiling_case(1, classes)
    _assert_ceiling_handles(case)
    y = torch.from_numpy(case["y"]).to(DEV)
    w = T.row_weights(torch.from_numpy(case["tr"]).to(DEV), N_MAX)

    def run(small):
        model = _model(case, F_IN, classes, cfg, p_drop, seed=3)
        model.dropout_state = AF.DropoutState(torch.device(DEV), seed=77)
        opt = FusedAdamW(model.parameters(), lr=0.02, weight_decay=5e-3)
        step = T.TrainStep(model, opt, case["xs"], case["ops"], y, w, use_graph=use_graph, small_step=None if small else False)
        assert (step.small is not None) == small, step.small_refused
        losses = [float(step()) for _ in range(10)]
        return model, opt, losses

    ma, oa, la = run(True)
    mb, ob, lb = run(False)
    np.testing.assert_allclose(la, lb, rtol=3e-5, atol=1e-6)
    _runs_agree(ma, oa, mb, ob, 10, p_drop)
    if use_graph:
        mc, _, lc = run(True)
        assert la == lc
        assert all(torch.equal(u, v) for u, v in zip(ma.parameters(), mc.parameters()))


def test_ceiling_evaluation_pass():
    """EvalStep on the small path (launches 1-3, train = 0) on the ceiling graph: logits against the float64 oracle's
    eval-mode forward, accuracies and loss against EvalStep(small_step=False), a captured pass bit-identical."""
    from acm_gnn_amd import train as T
    cfg, classes = CONFIGS[4], 8
    case = _ceiling_case(1, classes)
    _assert_ceiling_handles(case)
    y = torch.from_numpy(case["y"]).to(DEV)
    idx = torch.randperm(N_MAX, generator=torch.Generator().manual_seed(0)).to(DEV)
    sets = (idx[: N_MAX // 2], idx[N_MAX // 2: 3 * N_MAX // 4], idx[3 * N_MAX // 4:])
    model = _model(case, F_IN, classes, cfg, 0.5)
    ev_s = T.EvalStep(model, case["xs"], case["ops"], y, sets)
    ev_g = T.EvalStep(model, case["xs"], case["ops"], y, sets, small_step=False)
    ev_c = T.EvalStep(model, case["xs"], case["ops"], y, sets, use_graph=True)
    assert ev_s.small is not None and ev_g.small is None and ev_c.small is not None, ev_s.small_refused
    (o1, a1, l1), (o2, a2, l2), (o3, a3, l3) = ev_s(), ev_g(), ev_c()
    params = {k: v.detach().cpu().double() for k, v in model.state_dict().items() if k.startswith("gcns.")}
    low_t, high_t, un_t = _filters64(case["adj"])
    ref = O.gcn_forward(params, torch.from_numpy(case["x_np"]).double(), low_t, high_t, un_t, model_type=cfg["mt"],
                        variant=cfg["v"], structure_info=cfg["s"], attn_layernorm=cfg["ln"], dropout=0.5, training=False)
    scale = float(ref.abs().max()) + 1e-6
    assert float((o1.cpu().double() - ref).abs().max()) <= 2e-5 * scale + 1e-5
    torch.testing.assert_close(o1, o2, rtol=1e-4, atol=1e-5)
    np.testing.assert_allclose(a1, a2, atol=2e-3)
    np.testing.assert_allclose(l1, l2, rtol=1e-4)
    assert torch.equal(o1, o3) and a1 == a3 and l1 == l3


def test_the_envelope_ends_at_16384_rows_and_8_classes():
    """16 384 rows and 8 classes take the fused step; 16 385 rows and 9 classes are declined with their reasons, and
    TrainStep stays on the general path saying why."""
    from acm_gnn_amd import FusedAdam, train as T
    from acm_gnn_amd.small import SmallPlan
    cfg = CONFIGS[0]
    cases = {N_MAX: _ceiling_case(0, 6)}
    adj = sp.csr_matrix(sp.diags([np.ones(N_MAX)], [1], shape=(N_MAX + 1, N_MAX + 1)), dtype=np.float32)
    adj = ((adj + adj.T) > 0).astype(np.float32).tocsr()            # a path of 16 385 nodes
    x_np = np.zeros((N_MAX + 1, F_IN), np.float32)
    x_np[np.arange(N_MAX + 1), np.arange(N_MAX + 1) % F_IN] = 1.0
    cases[N_MAX + 1] = _direct_case(adj, x_np, 6, seed=1, s=0)

    def plan_of(case, classes):
        model = _model(case, F_IN, classes, cfg, 0.0)
        opt = FusedAdam(model.parameters(), lr=0.01)
        why = SmallPlan.why_not(model, case["xs"], case["ops"], opt)
        y = torch.from_numpy(case["y"] % classes).to(DEV)
        w = T.row_weights(torch.from_numpy(case["tr"]).to(DEV), case["n"])
        step = T.TrainStep(model, opt, case["xs"], case["ops"], y, w)
        assert (step.small is None) == (why is not None) and step.small_refused == why
        return why

    assert plan_of(cases[N_MAX], 8) is None
    assert plan_of(cases[N_MAX + 1], 8) == f"{N_MAX + 1} rows (<= {N_MAX})"
    assert plan_of(cases[N_MAX], 9) == "9 classes (<= 8)"
