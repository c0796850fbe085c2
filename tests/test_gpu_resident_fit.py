"""fit / fit_concurrent with the selection state on the device (sync_every > 1, keep_best) against the synchronous loop, end to
end on the GPU: a 200-node generated graph and the real Chameleon structure, counter-based dropout 0.5 with seeded states,
model / optimizer / seeds rebuilt identically for every arm.  Everything is compared exactly."""
import functools
import os

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from conftest import GOLDEN
from select_ref import same_floats, select_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPOCHS, WINDOW = 60, 10
LR = {"synthetic": 0.05, "chameleon": 0.2, "gcn": 0.1}           # high enough for the validation loss to turn inside the budget
SYNCS = (2, 7, 64)


@functools.lru_cache(maxsize=None)
def _problem(name):
    """(operators, CSR features, dense features, labels, (train, val, test), n, f_in, classes)"""
    from acm_gnn_amd import SparseFeatures, data as D, synthetic as S
    from acm_gnn_amd.distributed import make_sharded_operators
    if name == "synthetic":
        g = S.generate_graph("random", 5, 40, degree_intra=2, edge_homo=0.3, seed=3, device=DEV)
        x = S.random_features(g.n, 32, seed=3, device=DEV)
        sets = S.disassortative_splits(g.labels, 5, seed=3)
        xs = SparseFeatures.from_scipy(sp.csr_matrix(x.cpu().numpy()), DEV)
        return g.operators(), xs, x, g.labels, sets, g.n, 32, 5
    g = np.load(os.path.join(GOLDEN, "graph_chameleon.npz"))
    n = int(g["n"])
    adj = sp.csr_matrix((np.ones(len(g["adj_un_indices"]), np.float32), g["adj_un_indices"], g["adj_un_indptr"]), shape=(n, n))
    low, deg = D.build_filters(adj)
    ops = make_sharded_operators(low, deg, torch.device(DEV))
    rng = np.random.default_rng(11)
    x_np = (rng.random((n, 300)) < 0.02).astype(np.float32)
    y = torch.from_numpy(rng.integers(0, 5, n)).to(DEV)
    idx = torch.from_numpy(rng.permutation(n)).to(DEV)
    sets = (idx[: n // 2], idx[n // 2: 3 * n // 4], idx[3 * n // 4:])
    return ops, SparseFeatures.from_scipy(sp.csr_matrix(x_np), DEV), torch.from_numpy(x_np).to(DEV), y, sets, n, 300, 5


def _make(problem, kind, seed=0):
    """A fresh (model, optimizer, features) for one arm: same initial parameters, optimizer state and dropout stream each time."""
    import acm_gnn_amd
    from acm_gnn_amd import FusedAdam, baselines, functional as AF
    ops, xs, x, y, sets, n, f_in, classes = _problem(problem)
    torch.manual_seed(100 + seed)
    if kind == "acmgcn":
        model, feats, lr = acm_gnn_amd.GCN(f_in, 64, classes, 2, n, 0.5, "acmgcn", 0).to(DEV), xs, LR[problem]
    else:
        model, feats, lr = baselines.GCN(f_in, 32, classes, 0.5, "gcn").to(DEV), x, LR["gcn"]
    model.fused_dropout = True
    model.dropout_state = AF.DropoutState(torch.device(DEV), seed=4242 + seed)
    return model, FusedAdam(model.parameters(), lr=lr, weight_decay=5e-4), feats


def _fit(problem, kind, rule, seed=0, epochs=EPOCHS, sets=None, **kw):
    from acm_gnn_amd import train as T
    ops, xs, x, y, sets0, *_ = _problem(problem)
    model, opt, feats = _make(problem, kind, seed)
    es = WINDOW if rule == "min_val_loss" else 0
    res = T.fit(model, opt, feats, ops, y, *(sets or sets0), epochs, rule=rule, early_stopping=es, use_graph=True, **kw)
    return res, model


@functools.lru_cache(maxsize=None)
def _base(problem, kind, rule):
    """The synchronous loop's (selected, history): computed once, shared, never modified."""
    (sel, hist), _ = _fit(problem, kind, rule)
    return sel, tuple(hist)


def _same(got, want):
    return same_floats(got[0], want[0]) and same_floats(list(got[1]), list(want[1]))


@pytest.mark.parametrize("problem,kind", [("synthetic", "acmgcn"), ("chameleon", "acmgcn"), ("synthetic", "gcn")])
def test_preconditions_hold(problem, kind):
    """What makes the comparisons below mean something: the synchronous loop is reproducible bit for bit, the acmgcn arms run the
    fused small-graph plan (the baseline the general path), and the early stop trips strictly inside the budget."""
    from acm_gnn_amd import train as T
    ops, xs, x, y, sets, *_ = _problem(problem)
    model, opt, feats = _make(problem, kind)
    step = T.TrainStep(model, opt, feats, ops, y, T.row_weights(sets[0], y.shape[0], device=y.device))
    assert (step.small is not None) == (kind == "acmgcn"), step.small_refused
    for rule in ("max_val_acc", "min_val_loss"):
        again, _ = _fit(problem, kind, rule)
        assert _same(again, _base(problem, kind, rule)), rule
    hist = _base(problem, kind, "min_val_loss")[1]
    print(f"{problem}/{kind}: min_val_loss stops after {len(hist)} of {EPOCHS} epochs")
    assert 12 < len(hist) - 1 < EPOCHS - 1, len(hist)
    assert len(_base(problem, kind, "max_val_acc")[1]) == EPOCHS
    for rule in ("max_val_acc", "min_val_loss"):
        sel, h = _base(problem, kind, rule)
        want = select_ref(h, rule, WINDOW if rule == "min_val_loss" else 0)
        assert same_floats(sel, want[0]) and len(want[1]) == len(h)


@pytest.mark.parametrize("rule", ["max_val_acc", "min_val_loss"])
@pytest.mark.parametrize("problem,kind", [("synthetic", "acmgcn"), ("chameleon", "acmgcn"), ("synthetic", "gcn")])
def test_sync_every_returns_what_the_synchronous_loop_returns(problem, kind, rule):
    want = _base(problem, kind, rule)
    for k in SYNCS:
        got, _ = _fit(problem, kind, rule, sync_every=k)
        assert _same(got, want), (k, len(got[1]), len(want[1]))


def test_second_protocol_float64_results():
    """criterion="bce", metric="rocauc": the evaluation pass hands its four numbers over in float64."""
    (sel, hist), _ = _fit("synthetic", "acmgcn", "max_val_acc", epochs=6, criterion="bce", metric="rocauc")
    assert len(hist) == 6 and all(0.0 <= v <= 1.0 for row in hist for v in row[1:4])
    for k in SYNCS:
        got, _ = _fit("synthetic", "acmgcn", "max_val_acc", epochs=6, criterion="bce", metric="rocauc", sync_every=k)
        assert _same(got, (sel, hist)), k


@pytest.mark.parametrize("problem", ["synthetic", "chameleon"])
def test_keep_best_returns_the_selected_model(problem):
    from acm_gnn_amd import train as T
    ops, xs, x, y, sets, *_ = _problem(problem)
    want = _base(problem, "acmgcn", "min_val_loss")
    best_epoch = select_ref(want[1], "min_val_loss", WINDOW)[2]
    assert 0 <= best_epoch < len(want[1]) - 1, "the selected epoch must not be the last one for this test to mean anything"
    got, model = _fit(problem, "acmgcn", "min_val_loss", sync_every=7, keep_best=True)
    assert _same(got, want)
    _, accs, val_loss = T.EvalStep(model, xs, ops, y, sets)()
    assert same_floats(tuple(accs) + (val_loss,), want[1][best_epoch][1:]), (accs, val_loss, want[1][best_epoch])
    _, last = _fit(problem, "acmgcn", "min_val_loss", sync_every=7)
    assert any(not torch.equal(p, q) for p, q in zip(model.parameters(), last.parameters()))
    got1, model1 = _fit(problem, "acmgcn", "min_val_loss", keep_best=True)          # sync_every = 1 on the resident loop
    assert _same(got1, want) and all(torch.equal(p, q) for p, q in zip(model.parameters(), model1.parameters()))


def test_fit_concurrent_with_sync_every_equals_the_runs_alone():
    from acm_gnn_amd import train as T
    ops, xs, x, y, sets0, n, *_ = _problem("synthetic")

    def split(k):
        idx = torch.randperm(n, generator=torch.Generator().manual_seed(k)).to(DEV)
        return idx[: n // 2], idx[n // 2: 3 * n // 4], idx[3 * n // 4:]

    runs = []
    for k in range(4):
        model, opt, feats = _make("synthetic", "acmgcn", seed=k)
        runs.append((model, opt) + split(k))
    got = T.fit_concurrent(runs, xs, ops, y, EPOCHS, rule="min_val_loss", early_stopping=WINDOW, streams=2, sync_every=5)
    assert len(got) == 4
    for k in range(4):
        want, _ = _fit("synthetic", "acmgcn", "min_val_loss", seed=k, sets=split(k))
        assert _same(got[k], want), k
    assert len({len(g[1]) for g in got}) > 1 or len(got[0][1]) < EPOCHS          # the stops were real


@pytest.mark.parametrize("rule", ["max_val_acc", "min_val_loss"])
def test_fit_concurrent_keep_best_on_streams_returns_the_selected_models(rule):
    """keep_best through the stream pool, for both rules (max_val_acc is not fit_concurrent's default): the restore is enqueued
    on a pool stream, the models are read HERE on the default stream right after the call -- each must be its run's selected
    epoch, i.e. an evaluation pass on it reproduces that history row."""
    from acm_gnn_amd import train as T
    ops, xs, x, y, sets0, n, *_ = _problem("synthetic")
    es = WINDOW if rule == "min_val_loss" else 0

    def split(k):
        idx = torch.randperm(n, generator=torch.Generator().manual_seed(k)).to(DEV)
        return idx[: n // 2], idx[n // 2: 3 * n // 4], idx[3 * n // 4:]

    runs = []
    for k in range(3):
        model, opt, feats = _make("synthetic", "acmgcn", seed=k)
        runs.append((model, opt) + split(k))
    got = T.fit_concurrent(runs, xs, ops, y, EPOCHS, rule=rule, early_stopping=es, streams=2, sync_every=7, keep_best=True)
    params = [[p.detach().clone() for p in run[0].parameters()] for run in runs]       # first read, default stream
    not_last = 0
    for k in range(3):
        want, _ = _fit("synthetic", "acmgcn", rule, seed=k, sets=split(k))
        assert _same(got[k], want), k
        best_epoch = select_ref(want[1], rule, es)[2]
        not_last += best_epoch < len(want[1]) - 1
        _, accs, val_loss = T.EvalStep(runs[k][0], xs, ops, y, split(k))()
        assert same_floats(tuple(accs) + (val_loss,), want[1][best_epoch][1:]), (k, accs, val_loss, want[1][best_epoch])
        assert all(torch.equal(p, q) for p, q in zip(params[k], runs[k][0].parameters())), k
    assert not_last, "every run selected its last epoch: the restore is not exercised"


@pytest.mark.parametrize("rule,es", [("max_val_acc", 0), ("min_val_loss", 3)])
def test_host_selected_fit_concurrent_with_more_runs_than_streams_equals_fit(rule, es):
    """The host-selected path of fit_concurrent (sync_every=1): a baseline GCN (the general path) and two acmgcn runs (the fused
    small-graph plan) on two streams, so the third run takes over a freed slot -- each equals fit(use_graph=True) of it alone."""
    from acm_gnn_amd import train as T
    ops, xs, x, y, sets0, n, *_ = _problem("synthetic")
    kinds = ("gcn", "acmgcn", "acmgcn")

    def split(k):
        idx = torch.randperm(n, generator=torch.Generator().manual_seed(k)).to(DEV)
        return idx[: n // 2], idx[n // 2: 3 * n // 4], idx[3 * n // 4:]

    def make(k):
        model, opt, _ = _make("synthetic", kinds[k], seed=k)
        return (model, opt) + split(k)

    runs = [make(k) for k in range(3)]
    got = T.fit_concurrent(runs, xs, ops, y, 10, rule=rule, early_stopping=es, streams=2)
    for k in range(3):
        alone = make(k)
        want = T.fit(alone[0], alone[1], xs, ops, y, *alone[2:], 10, rule=rule, early_stopping=es, use_graph=True)
        assert _same(got[k], want) and 1 <= len(want[1]) <= 10, k
        assert all(torch.equal(p, q) for p, q in zip(runs[k][0].parameters(), alone[0].parameters())), k
        step = T.TrainStep(*make(k)[:2], xs, ops, y, T.row_weights(alone[2], n, device=y.device))
        assert (step.small is not None) == (kinds[k] == "acmgcn"), (k, step.small_refused)


def test_resident_loop_needs_the_captured_graphs():
    from acm_gnn_amd import train as T
    ops, xs, x, y, sets, *_ = _problem("synthetic")
    model, opt, feats = _make("synthetic", "acmgcn")
    with pytest.raises(ValueError, match="use_graph"):
        T.fit(model, opt, feats, ops, y, *sets, 5, sync_every=3)
