"""ROC-AUC on the device (acm_rocauc_scores + torch.sort + acm_rocauc, ABI 29) on the MI355X: exact integer triples where fp32
scores tie and order identically on any device, a pair-counting bound elsewhere, EvalStep / fit with the second protocol and
the drop-in binding of data_utils.eval_rocauc."""
import math
import os
import sys
import types

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import launch_forms as LF
import rocauc_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _weights(sets, n):
    w = torch.zeros(len(sets), n)
    for k, idx in enumerate(sets):
        w[k, torch.as_tensor(idx)] = 1.0 / max(len(idx), 1)
    return w


def _device_triples(logits, labels, sets, buffers=None):
    from acm_gnn_amd import functional as AF
    z = torch.as_tensor(logits).to(DEV)
    auc, counts = AF.eval_rocauc(z, torch.as_tensor(labels).to(DEV), _weights(sets, z.shape[0]).to(DEV), buffers, return_counts=True)
    return counts.cpu().numpy(), auc.cpu().numpy()


def _check_exact(logits, labels, sets, buffers=None):
    scores = R.cpu_scores(logits)
    got, auc = _device_triples(logits, labels, sets, buffers)
    want = np.asarray([R.triple(scores, labels, idx) for idx in sets], np.int64)
    assert np.array_equal(got, want), (got.tolist(), want.tolist())
    for k, t in enumerate(want):
        a = R.auc_of(t)
        assert (math.isnan(a) and math.isnan(auc[k])) or auc[k] == a, (k, auc[k], a)      # the same correctly rounded quotient
    return got


@pytest.mark.parametrize("k", [1, 3, 8])
@pytest.mark.parametrize("n", [5, 257, 5000, 70_001])
def test_exact_triples_on_the_grid(n, k):
    rng = np.random.default_rng(n + k)
    logits = R.grid_logits(n, n + k)
    labels = rng.integers(0, 2, n).astype(np.int64)
    if n == 5:
        labels[:] = [0, 1, 1, 0, 1]
    # overlapping random sets of different sizes; the first is everything
    sets = [np.arange(n)] + [np.sort(rng.permutation(n)[: max(2, n // (j + 1))]) for j in range(1, k)]
    out = set(range(n)) - set(np.concatenate(sets[1:]).tolist()) if k > 1 else set()
    if k > 1 and n > 5:
        labels[sorted(out)] = -1                             # unlabeled rows outside every set but the first...
        sets[0] = np.asarray(sorted(set(range(n)) - out))    # ... which is taken out of them
        labels[sets[1][:3]] = 2                              # rows labelled 2 inside a set: skipped
    _check_exact(logits, labels, sets)


def _grid_case(n, k):
    rng = np.random.default_rng(n + k)
    labels = rng.integers(0, 2, n).astype(np.int64)
    labels[rng.random(n) < 0.02] = -1                       # unlabeled rows inside the sets: skipped
    sets = [np.arange(n)] + [np.sort(rng.permutation(n)[: max(2, n // (j + 1))]) for j in range(1, k)]
    return R.grid_logits(n, n + k), labels, sets


@pytest.mark.parametrize("k", [1, 8])
@pytest.mark.parametrize("n", LF.AUC_TILE_EDGE_N)
def test_exact_triples_where_the_positions_end_on_a_tile_edge(n, k):
    """The n + 1 prefix positions end one short of a tile, exactly on it and one past it."""
    _check_exact(*_grid_case(n, k))


@pytest.mark.parametrize("n,k", [(LF.AUC_SCAN_N, 2), (LF.AUC_SCORES_N, 1)])
def test_exact_triples_past_the_scan_step_and_the_scores_grid(n, k):
    """More than 256 tiles: the scan over the tile counts takes a second trip with a carry; more than 4096 x 256 rows: the
    grid-stride loop of the scores kernel does."""
    _check_exact(*_grid_case(n, k))


def test_long_tie_groups_all_equal_one_class_and_reused_buffers():
    from acm_gnn_amd import functional as AF
    n = 20_000
    rng = np.random.default_rng(5)
    labels = rng.integers(0, 2, n).astype(np.int64)
    sets = [np.sort(rng.permutation(n)[:12_000]), np.arange(0, n, 3), np.arange(n)]
    bufs = AF.rocauc_buffers(n, 3, DEV)
    # five distinct scores: tie groups thousands long, across every tile boundary
    five = R.grid_logits(n, 6, extremes=False, levels=5)
    assert np.unique(R.cpu_scores(five)).size == 5
    first = _check_exact(five, labels, sets, bufs)
    for _ in range(3):
        assert np.array_equal(_device_triples(five, labels, sets, bufs)[0], first)
    # all scores equal: exactly one half
    same = np.tile(np.array([[0.5, -1.25]], np.float32), (n, 1))
    got, auc = _device_triples(same, labels, sets, bufs)
    assert (auc == 0.5).all() and (got[:, 0] == got[:, 1] * got[:, 2]).all()
    # a set with one class only: NaN there, the others unaffected
    one = labels.copy()
    only = np.arange(0, n, 3)
    one[only] = 1
    got = _check_exact(R.grid_logits(n, 7), one, [sets[0], only, sets[2]], bufs)
    assert got[1, 2] == 0 and got[1, 0] == 0 and got[0, 2] > 0
    assert math.isnan(_device_triples(R.grid_logits(n, 7), one, [sets[0], only, sets[2]], bufs)[1][1])


def test_golden_cases_reproduce_the_reference():
    with np.load(os.path.join(GOLDEN, "rocauc_cases.npz")) as f:
        g = {k: f[k] for k in f.files}
    tags = sorted({k.split(":")[0] for k in g})
    assert len(tags) >= 4
    for tag in tags:
        sets = [g[f"{tag}:set{k}"] for k in range(3)]
        got, auc = _device_triples(g[f"{tag}:logits"], g[f"{tag}:labels"], sets)
        assert np.array_equal(got, g[f"{tag}:triples"]), tag
        assert np.abs(auc - g[f"{tag}:reference"]).max() <= 1e-12, tag


def _check_bounded(logits, labels, sets, auc, ceiling=1e-4):
    """``ceiling`` keeps the bound from going vacuous: 1e-4 for the 20 000-row random cases; 1e-3 for the 2000-row graph, whose
    sets hold >= 200 rows of each class, so that one misplaced row (1 / npos >= 2e-3 of AUC) still fails."""
    scores = R.cpu_scores(logits)
    for k, idx in enumerate(sets):
        want = R.auc_of(R.triple(scores, labels, idx))
        bound = R.auc_bound(scores, labels, idx)
        print(f"set {k}: device {auc[k]!r} cpu {want!r} bound {bound:.3e}")
        assert bound < ceiling                               # (never vacuous)
        assert abs(auc[k] - want) <= bound


@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("c", [2, 5])
def test_random_logits_within_the_close_pair_bound(c, seed):
    n = 20_000
    rng = np.random.default_rng(seed)
    logits = (rng.standard_normal((n, c)) * 3).astype(np.float32)
    labels = rng.integers(0, 2, n).astype(np.int64)
    order = rng.permutation(n)
    sets = [np.sort(order[:10_000]), np.sort(order[10_000:15_000]), np.sort(order[15_000:])]
    _, auc = _device_triples(logits, labels, sets)
    _check_bounded(logits, labels, sets, auc)


def _tiny(seed=3):
    from acm_gnn_amd import data as D, distributed as DD
    from acm_gnn_amd.graph import clear_cache
    clear_cache()
    adj, x_np, y_np, splits, n = D.synthetic_dataset("tiny", seed=seed)
    low, deg = D.build_filters(adj)
    ops = DD.make_sharded_operators(low, deg, DEV)
    x, y = torch.from_numpy(x_np).to(DEV), torch.from_numpy(y_np).to(DEV)
    return ops, x, y, y_np, splits, n


def test_eval_step_rocauc_and_bce_eager_captured_and_fit():
    import acm_gnn_amd
    from acm_gnn_amd import train as T
    ops, x, y, y_np, splits, n = _tiny()
    sets = tuple(torch.from_numpy(s).to(DEV) for s in splits)
    torch.manual_seed(1)
    model = acm_gnn_amd.GCN(x.shape[1], 64, 2, 2, n, 0.0, "acmgcnp", 0, variant=False).to(DEV)
    T.EvalStep(model, x, ops, y, sets, loss_set=1)()      # (the first eval-mode forward fills the layers' P = A_low X cache;
    before = T.EvalStep(model, x, ops, y, sets, loss_set=1)()     # every later one reads it: those are the same bits)
    ev = T.EvalStep(model, x, ops, y, sets, loss_set=1, metric="rocauc", criterion="bce")
    out, aucs, loss = ev()
    logits = out.cpu()
    _check_bounded(logits.numpy(), y_np, splits, aucs, ceiling=1e-3)
    va = torch.from_numpy(splits[1])
    want = float(F.binary_cross_entropy_with_logits(logits[va].double(), F.one_hot(torch.from_numpy(y_np), 2)[va].double()))
    assert abs(loss - want) <= 5e-6 * abs(want), (loss, want)
    ev_g = T.EvalStep(model, x, ops, y, sets, loss_set=1, metric="rocauc", criterion="bce", use_graph=True)
    for _ in range(2):
        out_g, aucs_g, loss_g = ev_g()
        assert torch.equal(out_g, out) and aucs_g == aucs and loss_g == loss
    # mixed keywords, and the default pass is what it was
    _, accs, bce = T.EvalStep(model, x, ops, y, sets, loss_set=1, criterion="bce")()
    assert bce == loss and np.allclose(accs, before[1], rtol=0, atol=1e-4)        # (fp32 sums of <= 1000 equal terms; one row is 1e-3)
    _, aucs2, nll = T.EvalStep(model, x, ops, y, sets, loss_set=1, metric="rocauc")()
    assert aucs2 == aucs and abs(nll - before[2]) <= 1e-5 * abs(before[2])
    after = T.EvalStep(model, x, ops, y, sets, loss_set=1)()
    assert torch.equal(after[0], before[0]) and after[1:] == before[1:]
    _, plain = T.evaluate(model, x, ops, y, sets, metric="rocauc")
    assert plain == aucs
    for use_graph in (False, True):
        opt = acm_gnn_amd.FusedAdamW(model.parameters(), lr=0.02, weight_decay=1e-3)
        best, hist = T.fit(model, opt, x, ops, y, *sets, epochs=3, criterion="bce", metric="rocauc", use_graph=use_graph)
        assert len(hist) == 3 and 0.0 <= best <= 1.0
        for row in hist:
            assert all(0.0 <= v <= 1.0 for v in row[1:4]) and np.isfinite(row[0]) and np.isfinite(row[4])


def test_sharded_operators_refuse_rocauc():
    from acm_gnn_amd import train as T
    ops, x, y, _, splits, n = _tiny()

    class Sharded(type(ops)):
        sharded = True

    fake = object.__new__(Sharded)
    fake.__dict__.update(ops.__dict__)
    with pytest.raises(NotImplementedError, match="rocauc"):
        T.EvalStep(None, x, fake, y, [torch.from_numpy(s).to(DEV) for s in splits], metric="rocauc", small_step=False)


def _stub_data_utils(monkeypatch):
    """A data_utils module in the reference's calling convention, built on the numpy helper."""
    du = types.ModuleType("data_utils")

    def eval_acc(y_true, y_pred):
        return float((y_true.view(-1) == y_pred.argmax(-1)).double().mean())

    def eval_rocauc(y_true, y_pred):
        yt = y_true.detach().cpu().numpy().reshape(-1)
        if not ((yt == 1).any() and (yt == 0).any()):
            return -1.0                                      # (the reference raises here; whatever the bound function answers
                                                             # is what has to come back)
        return R.midrank_auc(yt, R.cpu_scores(y_pred))

    @torch.no_grad()
    def evaluate_acmgcn(model, x, adj_low, adj_high, adj_low_unnormalized, dataset, split_idx, eval_func, result=None):
        if result is not None:
            out = result
        else:
            model.eval()
            out = model(x, adj_low, adj_high, adj_low_unnormalized)
        vals = [eval_func(dataset.label[split_idx[k]], out[split_idx[k]]) for k in ("train", "valid", "test")]
        return vals[0], vals[1], vals[2], out

    du.eval_acc, du.eval_rocauc, du.evaluate_acmgcn = eval_acc, eval_rocauc, evaluate_acmgcn
    monkeypatch.setitem(sys.modules, "data_utils", du)
    return du


def test_dropin_fast_evaluate_takes_eval_rocauc(monkeypatch):
    import acm_gnn_amd
    from acm_gnn_amd import dropin, functional as AF
    ops, x, y, y_np, splits, n = _tiny()
    du = _stub_data_utils(monkeypatch)
    stub = du.evaluate_acmgcn
    assert dropin.install_fast_evaluate() is stub and du.evaluate_acmgcn is not stub
    calls = []
    real = AF.eval_rocauc
    monkeypatch.setattr(AF, "eval_rocauc", lambda *a, **kw: (calls.append(1), real(*a, **kw))[1])
    torch.manual_seed(2)
    model = acm_gnn_amd.GCN(x.shape[1], 64, 2, 2, n, 0.0, "acmgcnp", 0, variant=False).to(DEV)
    dataset = types.SimpleNamespace(label=y.view(-1, 1))
    split_idx = {k: torch.from_numpy(s).to(DEV) for k, s in zip(("train", "valid", "test"), splits)}
    got = du.evaluate_acmgcn(model, x, ops, None, None, dataset, split_idx, du.eval_rocauc)
    want = stub(model, x, ops, None, None, dataset, split_idx, du.eval_rocauc, got[3])      # the stub alone on the same logits
    assert len(calls) == 1 and want[3] is got[3]
    torch.testing.assert_close(got[3], stub(model, x, ops, None, None, dataset, split_idx, du.eval_rocauc)[3], rtol=1e-5, atol=1e-6)
    scores = R.cpu_scores(got[3])
    for k, idx in enumerate(splits):
        assert isinstance(got[k], float)
        assert abs(got[k] - want[k]) <= R.auc_bound(scores, y_np, idx) < 1e-3            # (ceiling: see _check_bounded)
    # a one-class test split: the bound function's own answer, exactly
    one = y.clone()
    one[split_idx["test"]] = 1
    lone = types.SimpleNamespace(label=one.view(-1, 1))
    got1 = du.evaluate_acmgcn(model, x, ops, None, None, lone, split_idx, du.eval_rocauc)
    want1 = stub(model, x, ops, None, None, lone, split_idx, du.eval_rocauc, got1[3])
    assert got1[:3] == want1[:3] and got1[2] == -1.0
    assert len(calls) == 2                                   # (the library looked first, then handed the call over)
    # eval_acc keeps its own fast path
    acc = du.evaluate_acmgcn(model, x, ops, None, None, dataset, split_idx, du.eval_acc)
    ref = stub(model, x, ops, None, None, dataset, split_idx, du.eval_acc, acc[3])
    assert acc[:3] == pytest.approx(ref[:3], abs=1e-12) and len(calls) == 2
