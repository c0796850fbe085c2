"""Model selection and early stopping on the device, everything that needs no GPU: the two entry points are exported (ABI still
29) and refuse bad arguments before any launch, their structs have the C layout, and -- on the CPU double, with numpy
implementations of acm_select_step / acm_copy_if set on the installed instance -- ``fit`` / ``fit_concurrent`` with
``sync_every`` > 1 return exactly what ``sync_every=1`` returns."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import fake_lib
from conftest import ROOT
from fake_lib import _vec
from select_ref import same_floats, select_ref


# ------------------------------------------------------------------------------------------------ the real library, no GPU
def test_new_symbols_are_exported_and_the_abi_is_still_29():
    from acm_gnn_amd import _lib
    lib = _lib.load()
    assert lib.acm_version() == 29 == _lib.ABI_VERSION
    for name in ("acm_select_step", "acm_copy_if"):
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name)
    from acm_gnn_amd import build
    assert "acm_select.hip" in build.SOURCES


def _select_block(**kw):
    from acm_gnn_amd import _lib
    p = _lib.Select()
    p.rule, p.early_stopping, p.epochs = 1, 3, 10
    p.result, p.train_loss, p.ctrl, p.best, p.history = 0x1000, 0x2000, 0x3000, 0x4000, 0x5000     # never dereferenced: every
    for k, v in kw.items():                                                                       # call below is refused
        setattr(p, k, v)
    return p


@pytest.mark.parametrize("bad,word", [
    (dict(rule=2), b"rule"), (dict(rule=-1), b"rule"), (dict(epochs=0), b"epochs"), (dict(early_stopping=-1), b"early_stopping"),
    (dict(result=None), b"result"), (dict(result_f64=0x6000), b"result"), (dict(train_loss=None), b"NULL"),
    (dict(ctrl=None), b"NULL"), (dict(best=None), b"NULL"), (dict(history=None), b"NULL")])
def test_select_step_refuses_bad_arguments_before_any_launch(bad, word):
    from acm_gnn_amd import _lib
    lib = _lib.load()
    p = _select_block(**bad)
    assert lib.acm_select_step(C.byref(p), None) == 1                   # ACM_EINVAL (a launch here would be ACM_EHIP: no GPU)
    assert word in lib.acm_last_error(), lib.acm_last_error()
    assert lib.acm_select_step(None, None) == 1


def test_copy_if_refuses_bad_arguments_before_any_launch():
    from acm_gnn_amd import _lib
    lib = _lib.load()
    table = (_lib.CopyTensor * 2)()
    table[0].src, table[0].dst, table[0].numel = 0x1000, 0x2000, 4
    table[1].src, table[1].dst, table[1].numel = 0x3000, 0x4000, 4
    tp = C.cast(table, C.c_void_p)
    assert lib.acm_copy_if(-1, tp, 0x5000, None) == 1 and b"n_tensors" in lib.acm_last_error()
    assert lib.acm_copy_if(2, None, 0x5000, None) == 1 and b"table" in lib.acm_last_error()
    assert lib.acm_copy_if(2, tp, None, None) == 1 and b"flag" in lib.acm_last_error()
    table[1].numel = -1                                   # the SECOND entry: the whole table is checked before the first launch
    assert lib.acm_copy_if(2, tp, 0x5000, None) == 1 and b"tensor 1" in lib.acm_last_error()
    table[1].numel, table[1].dst = 4, None
    assert lib.acm_copy_if(2, tp, 0x5000, None) == 1 and b"tensor 1" in lib.acm_last_error()
    table[1].dst = 0x4002
    assert lib.acm_copy_if(2, tp, 0x5000, None) == 1 and b"aligned" in lib.acm_last_error()
    assert lib.acm_copy_if(0, None, 0x5000, None) == 0    # an empty table: nothing to launch


def test_new_structs_have_the_c_layout(tmp_path):
    from acm_gnn_amd import _lib
    structs = {"acm_select_t": _lib.Select, "acm_copy_tensor_t": _lib.CopyTensor}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "acm_hip.h"', "int main(void){"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {}
    for ln in subprocess.check_output([str(exe)], text=True).splitlines():
        s, f, v = ln.split()
        got[(s, f)] = int(v)
    for cname, cls in structs.items():
        assert got[(cname, "size")] == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)


# ------------------------------------------------------------------------------------------------ the CPU double
def _np_select_step(pp, stream):
    """acm_select_step as include/acm_hip.h states it, on host pointers."""
    p = pp._obj
    if p.rule not in (0, 1) or p.epochs < 1 or p.early_stopping < 0 or bool(p.result) == bool(p.result_f64):
        return 1
    ctrl, best = _vec(p.ctrl, 8, np.int32), _vec(p.best, 2, np.float64)
    hist = fake_lib._view(p.history, p.epochs, 5, 5, np.float64)
    epoch = int(ctrl[0])
    if ctrl[1] != 0 or epoch >= p.epochs:
        ctrl[3] = 0
        return 0
    res = _vec(p.result, 4, np.float32).astype(np.float64) if p.result else _vec(p.result_f64, 4, np.float64).copy()
    hist[epoch, 0] = np.float64(_vec(p.train_loss, 1, np.float32)[0])
    hist[epoch, 1:] = res
    m_va, m_te, val_loss = res[1], res[2], res[3]
    key = m_va if p.rule == 0 else -val_loss
    ctrl[3] = 0
    if not np.isnan(key) and (ctrl[2] < 0 or key > best[0]):
        best[0], best[1], ctrl[2], ctrl[3] = key, m_te, epoch, 1
    es = int(p.early_stopping)
    if p.rule == 1 and es > 0 and epoch > es:
        s = np.float64(0.0)
        for v in hist[epoch - es:epoch, 4]:
            s = s + v
        if val_loss > s / np.float64(es):
            ctrl[1] = 1
    ctrl[0] = epoch + 1
    return 0


def _np_copy_if(n, table, flag, stream):
    from acm_gnn_amd import _lib
    if n < 0 or (n and not table) or not flag:
        return 1
    if _vec(flag, 1, np.int32)[0] == 0:
        return 0
    for t in (C.cast(table, C.POINTER(_lib.CopyTensor * n)).contents if n else []):
        if t.numel:
            _vec(t.dst, int(t.numel), np.int32)[...] = _vec(t.src, int(t.numel), np.int32)
    return 0


def _install(monkeypatch):
    """The CPU double with the two new entry points; a "captured" step / pass is its eager twin (nothing to capture here)."""
    fake = fake_lib.install(monkeypatch)
    fake.acm_select_step, fake.acm_copy_if = _np_select_step, _np_copy_if
    from acm_gnn_amd import train as T
    monkeypatch.setattr(T.TrainStep, "_capture", lambda self: None)
    monkeypatch.setattr(T.EvalStep, "_capture", lambda self: None)
    return fake


SEQUENCES = {
    "ties": [(0.5, 0.1, 0.7, 0.31, 1.0), (0.4, 0.2, 0.7, 0.32, 0.9), (0.3, 0.3, 0.8, 0.33, 0.9), (0.2, 0.2, 0.8, 0.34, 0.95)],
    "nan": [(0.5, 0.1, float("nan"), 0.31, float("nan")), (0.4, 0.2, 0.6, 0.32, 0.9), (0.3, 0.3, float("nan"), 0.33, float("nan")),
            (0.2, 0.2, 0.5, 0.34, 0.8)],
    "all_nan": [(0.5, 0.1, float("nan"), 0.31, float("nan"))] * 3,
    "stop": [(1.0, 0.5, 0.5, 0.5, v) for v in (1.0, 0.9, 0.8, 0.7, 0.6, 0.65, 0.7, 0.9, 0.5, 0.4)],
    "inf": [(1.0, 0.5, float("-inf"), 0.25, float("inf")), (1.0, 0.5, float("-inf"), 0.5, float("inf"))],
}


@pytest.mark.parametrize("name", sorted(SEQUENCES))
@pytest.mark.parametrize("rule,es", [("max_val_acc", 0), ("min_val_loss", 0), ("min_val_loss", 3)])
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_selection_state_on_the_double_equals_the_host_loop(monkeypatch, name, rule, es, dtype):
    """SelectionState end to end on host memory, and the double itself against the restated host loop."""
    _install(monkeypatch)
    from acm_gnn_amd import functional as AF
    rows = [tuple(float(np.float32(v)) for v in r) for r in SEQUENCES[name]]       # what an fp32 pass can produce
    want = select_ref(rows, rule, es)
    st = AF.SelectionState(rule, es, len(rows), "cpu")
    for r in rows + rows[:2]:                                                     # two calls beyond the budget
        st.launch(torch.tensor(r[0], dtype=torch.float32), torch.tensor(r[1:], dtype=dtype))
    selected, history, best_epoch = st.result()
    assert same_floats(selected, want[0]) and same_floats(history, want[1]) and best_epoch == want[2]
    assert st.poll() == (len(want[1]), want[3] is not None)
    if name == "stop" and es:
        assert want[3] == 6                   # 0.7 > mean(0.7, 0.6, 0.65); epoch 5's 0.65 < mean(0.8, 0.7, 0.6)
    with pytest.raises(ValueError):
        st.launch(torch.tensor(0.0, dtype=torch.float64), torch.zeros(4))
    with pytest.raises(ValueError):
        st.launch(torch.tensor(0.0), torch.zeros(5))


def test_snapshot_follows_the_selection_and_restores_in_place(monkeypatch):
    _install(monkeypatch)
    from acm_gnn_amd import functional as AF
    params = [torch.nn.Parameter(torch.zeros(3, 2)), torch.nn.Parameter(torch.zeros(0)), torch.nn.Parameter(torch.zeros(5))]
    st = AF.SelectionState("max_val_acc", 0, 6, "cpu", params=params)
    accs = [0.2, 0.5, 0.4, 0.5, 0.9, 0.1]
    for e, a in enumerate(accs):
        with torch.no_grad():
            for p in params:
                p.fill_(float(e + 1))
        st.launch(torch.tensor(0.0), torch.tensor([0.0, a, 0.0, 0.0]))
    ptrs = [p.data_ptr() for p in params]
    assert st.result()[2] == 4
    assert st.restore() and [p.data_ptr() for p in params] == ptrs
    assert all(bool((p == 5.0).all()) for p in params)
    with pytest.raises(ValueError):
        st.restore(torch.nn.Linear(2, 2))
    with pytest.raises(RuntimeError):
        AF.SelectionState("max_val_acc", 0, 6, "cpu").restore()


def _problem(n_runs=1):
    import scipy.sparse as sp
    from acm_gnn_amd import GCN, FusedAdam, SparseFeatures, data as D
    from acm_gnn_amd.distributed import make_sharded_operators
    n = 90
    rng = np.random.default_rng(12)
    m = n * 4
    r, c = rng.integers(0, n, m), rng.integers(0, n, m)
    adj = sp.csr_matrix((np.ones(m, np.float32), (r, c)), shape=(n, n))
    adj = ((adj + adj.T) > 0).astype(np.float32).tocsr()
    adj.setdiag(0)
    adj.eliminate_zeros()
    low, deg = D.build_filters(adj)
    ops = make_sharded_operators(low, deg, torch.device("cpu"))
    xs = SparseFeatures.from_scipy(sp.csr_matrix(((rng.random((n, 50)) < 0.08) * 1.0).astype(np.float32)), "cpu")
    y = torch.from_numpy(rng.integers(0, 3, n))

    def make(k):
        torch.manual_seed(k)
        model = GCN(50, 64, 3, 2, n, 0.0, "acmgcn", 0)
        idx = torch.randperm(n, generator=torch.Generator().manual_seed(k))
        return model, FusedAdam(model.parameters(), lr=0.1), idx[:40], idx[40:65], idx[65:]
    return ops, xs, y, make


EPOCHS = 14


@pytest.mark.parametrize("rule,es", [("max_val_acc", 0), ("max_val_acc", 3), ("min_val_loss", 0), ("min_val_loss", 3)])
def test_fit_with_sync_every_equals_the_synchronous_loop(monkeypatch, rule, es):
    _install(monkeypatch)
    from acm_gnn_amd import train as T
    ops, xs, y, make = _problem()

    def fit(**kw):
        model, opt, tr, va, te = make(0)
        return T.fit(model, opt, xs, ops, y, tr, va, te, EPOCHS, rule=rule, early_stopping=es, use_graph=True, **kw), model

    (sel, hist), base_model = fit()
    want = select_ref(hist, rule, es)
    assert same_floats(sel, want[0]) and len(hist) == len(want[1])
    if rule == "min_val_loss" and es:
        assert 4 < len(hist) < EPOCHS, "the early stop must trip inside the budget for this test to mean anything"
    else:
        assert len(hist) == EPOCHS
    for k in (2, 5, 64):
        (sel_k, hist_k), _ = fit(sync_every=k)
        assert same_floats(sel_k, sel) and same_floats(hist_k, hist), k
    # keep_best: the returned model is the selected epoch's -- an evaluation pass on it reproduces that history row
    (sel_b, hist_b), model = fit(sync_every=5, keep_best=True)
    assert same_floats(sel_b, sel) and same_floats(hist_b, hist)
    _, _, tr, va, te = make(0)
    _, accs, val_loss = T.EvalStep(model, xs, ops, y, (tr, va, te))()
    assert same_floats(tuple(accs) + (val_loss,), hist[want[2]][1:])
    if want[2] != len(hist) - 1:
        assert any(not torch.equal(p, q) for p, q in zip(model.parameters(), base_model.parameters()))


@pytest.mark.parametrize("rule,es", [("max_val_acc", 0), ("max_val_acc", 3), ("min_val_loss", 0), ("min_val_loss", 3)])
def test_fit_concurrent_with_sync_every_equals_fit(monkeypatch, rule, es):
    """Every (rule, early_stopping) through fit_concurrent's resident path -- "max_val_acc" is NOT its default rule -- at a
    sync_every that divides nothing (5), one that leaves a remainder of the budget (2 * 7 = 14, so 5 and 64 do; 2 does not) and
    one larger than the budget (64)."""
    _install(monkeypatch)
    from acm_gnn_amd import train as T
    ops, xs, y, make = _problem()
    want = []
    for k in range(3):
        m, opt, tr, va, te = make(k)
        want.append(T.fit(m, opt, xs, ops, y, tr, va, te, EPOCHS, rule=rule, early_stopping=es, use_graph=True))
    if (rule, es) == ("min_val_loss", 3):
        assert any(len(h) < EPOCHS for _, h in want), "no run stops early: the stop is not exercised"
    else:
        assert all(len(h) == EPOCHS for _, h in want)
    for sync in (2, 5, 64):
        got = T.fit_concurrent([make(k) for k in range(3)], xs, ops, y, epochs=EPOCHS, rule=rule, early_stopping=es, sync_every=sync)
        for k in range(3):
            assert same_floats(got[k][0], want[k][0]) and same_floats(got[k][1], want[k][1]), (sync, k)
    # keep_best through the same entry point: every model comes back as its run's selected epoch
    runs = [make(k) for k in range(3)]
    got = T.fit_concurrent(runs, xs, ops, y, epochs=EPOCHS, rule=rule, early_stopping=es, sync_every=5, keep_best=True)
    for k, (model, _, tr, va, te) in enumerate(runs):
        assert same_floats(got[k][0], want[k][0]) and same_floats(got[k][1], want[k][1]), k
        _, accs, val_loss = T.EvalStep(model, xs, ops, y, (tr, va, te))()
        assert same_floats(tuple(accs) + (val_loss,), want[k][1][select_ref(want[k][1], rule, es)[2]][1:]), k


def test_a_dropped_rule_would_show(monkeypatch):
    """The two rules select DIFFERENT values on this problem, so the comparisons above tell a swapped or dropped ``rule`` apart."""
    _install(monkeypatch)
    from acm_gnn_amd import train as T
    ops, xs, y, make = _problem()
    differ = 0
    for k in range(3):
        m, opt, tr, va, te = make(k)
        _, hist = T.fit(m, opt, xs, ops, y, tr, va, te, EPOCHS, rule="max_val_acc", use_graph=True)
        differ += not same_floats(select_ref(hist, "max_val_acc", 0)[0], select_ref(hist, "min_val_loss", 0)[0])
    assert differ, "both rules select the same test metric in every run: choose another problem"


class _InertStream:
    """Stands in for torch.cuda.Stream and, as ``_InertStream.use``, for torch.cuda.stream: nothing here touches a device."""
    made = []

    def __init__(self):
        self.made.append(self)
        self.entered = 0

    def synchronize(self):
        pass

    def use(self):
        import contextlib
        self.entered += 1
        return contextlib.nullcontext()


class _FakeRun:
    """A run that is finished after ``rounds`` calls of ``finished()``; every call goes to the shared log."""

    def __init__(self, name, rounds, log):
        self.name, self.rounds, self.log = name, rounds, log

    def enqueue(self, sync_every):
        self.log.append((self.name, "enqueue"))

    def finished(self):
        self.log.append((self.name, "finished"))
        self.rounds -= 1
        return self.rounds == 0

    def result(self):
        self.log.append((self.name, "result"))
        return self.name


def test_the_stream_scheduler_on_five_runs_and_two_slots(monkeypatch):
    """train._run_on_streams, the one scheduler of fit_concurrent, with runs that finish after 3, 1, 4, 1 and 2 rounds."""
    from acm_gnn_amd import train as T
    monkeypatch.setattr(_InertStream, "made", [])
    monkeypatch.setattr(torch.cuda, "Stream", _InertStream)
    monkeypatch.setattr(torch.cuda, "stream", _InertStream.use)
    log = []
    runs = [_FakeRun(name, rounds, log) for name, rounds in zip("abcde", (3, 1, 4, 1, 2))]

    def start(k):
        log.append((runs[k].name, "start"))
        return runs[k]

    assert T._run_on_streams(start, 5, 2, 1) == list("abcde")               # the results, in the order of the runs
    assert len(_InertStream.made) == 2 and all(s.entered for s in _InertStream.made)
    # a round = the entries from one "start or enqueue" stretch up to the next: slot filling, every enqueue, then the reads
    rounds, phase = [], None
    for name, what in log:
        if what in ("start", "enqueue") and phase not in ("start", "enqueue"):
            rounds.append([])
        rounds[-1].append((name, what))
        phase = what
    live_want = ["ab", "ac", "ac", "dc", "ec", "e"]       # b leaves after round 0 (-> c), a after 2 (-> d), d after 3 (-> e)
    assert len(rounds) == len(live_want)
    for entries, live in zip(rounds, live_want):
        whats = [w for _, w in entries if w != "result"]
        first_read = whats.index("finished")
        assert "enqueue" not in whats[first_read:] and "start" not in whats[first_read:], entries
        assert [n for n, w in entries if w == "enqueue"] == list(live) == [n for n, w in entries if w == "finished"], entries
    assert [n for n, w in log if w == "start"] == list("abcde")             # freed slots go to the pending runs in order
    assert [[n for n, w in r if w == "start"] for r in rounds] == [["a", "b"], ["c"], [], ["d"], ["e"], []]
    for run in runs:
        calls = [w for n, w in log if n == run.name]
        assert calls.count("result") == 1 and calls[-2:] == ["finished", "result"] and run.rounds == 0, (run.name, calls)


class _RowsStep:
    """TrainStep's and EvalStep's double for the host loop: hands out the rows of a recorded sequence, one per epoch."""
    rows, made = [], []

    def __init__(self, *args, **kw):
        self.made.append(self)
        self.epoch, self.small_refused = -1, None

    def __call__(self):                                 # TrainStep(): the loss -- a tensor, as the loop calls float() on it
        self.epoch += 1
        return torch.tensor(self.rows[self.epoch][0], dtype=torch.float64)

    def launch(self):
        self.epoch += 1

    def read(self):
        row = self.rows[self.epoch]
        return None, list(row[1:4]), row[4]


@pytest.mark.parametrize("name", sorted(SEQUENCES))
@pytest.mark.parametrize("rule,es", [("max_val_acc", 0), ("max_val_acc", 3), ("min_val_loss", 0), ("min_val_loss", 3)])
@pytest.mark.parametrize("use_graph", [True, False])
def test_the_host_loop_states_the_rule_of_select_ref(monkeypatch, name, rule, es, use_graph):
    """The ONE statement of the host rule (train._HostRun, reached through ``fit`` with its step and pass replaced by rows) against
    the restated loop: both rules, windows 0 and 3, NaN validation metrics, an early stop strictly inside the budget."""
    from acm_gnn_amd import train as T
    rows = SEQUENCES[name]
    monkeypatch.setattr(_RowsStep, "rows", rows)
    monkeypatch.setattr(_RowsStep, "made", [])
    monkeypatch.setattr(T, "TrainStep", _RowsStep)
    monkeypatch.setattr(T, "EvalStep", _RowsStep)
    seen = []

    def evaluate(*args, metric="acc"):
        seen.append(len(seen))
        return len(seen) - 1, list(rows[len(seen) - 1][1:4])

    monkeypatch.setattr(T, "evaluate", evaluate)
    monkeypatch.setattr(T, "_eager_val_loss", lambda out, labels, val_idx, criterion: rows[out][4])
    idx = torch.arange(2)
    got = T.fit(None, None, torch.zeros(4, 1), None, torch.zeros(4, dtype=torch.long), idx, idx, idx, len(rows), rule=rule,
                early_stopping=es, use_graph=use_graph)
    want = select_ref(rows, rule, es)
    assert same_floats(got[0], want[0]) and same_floats(got[1], want[1])
    assert len(_RowsStep.made) == (2 if use_graph else 1) and (bool(seen) != use_graph)
    assert all(s.epoch == len(want[1]) - 1 for s in _RowsStep.made)          # nothing was enqueued past the stop
    if name == "stop" and rule == "min_val_loss" and es:
        assert len(got[1]) == 7 < len(rows)
    else:
        assert len(got[1]) == len(rows)


def test_refresh_is_refused_once_the_run_has_begun(monkeypatch):
    _install(monkeypatch)
    from acm_gnn_amd import functional as AF, train as T
    ops, xs, y, make = _problem()
    model, opt, tr, va, te = make(0)
    st = AF.SelectionState("max_val_acc", 0, 4, "cpu")
    ev = T.EvalStep(model, xs, ops, y, (tr, va, te), use_graph=True, selector=st, train_loss=torch.tensor(0.5))
    ev.refresh()                                       # before the first epoch: allowed
    ev()
    assert st.poll() == (1, False)
    with pytest.raises(RuntimeError, match="refresh"):
        ev.refresh()
    assert st.poll() == (1, False)                     # and the state is as it was


def test_the_resident_loop_states_its_requirements(monkeypatch):
    _install(monkeypatch)
    from acm_gnn_amd import train as T
    ops, xs, y, make = _problem()
    model, opt, tr, va, te = make(0)
    with pytest.raises(ValueError, match="use_graph"):
        T.fit(model, opt, xs, ops, y, tr, va, te, 4, sync_every=3)
    with pytest.raises(ValueError, match="use_graph"):
        T.fit(model, opt, xs, ops, y, tr, va, te, 4, keep_best=True)
    with pytest.raises(ValueError, match="sync_every"):
        T.fit(model, opt, xs, ops, y, tr, va, te, 4, sync_every=0, use_graph=True)

    class Sharded(type(ops)):
        sharded = True

    sharded = object.__new__(Sharded)
    sharded.__dict__.update(ops.__dict__)
    with pytest.raises(NotImplementedError, match="sharded"):
        T.fit(model, opt, xs, sharded, y, tr, va, te, 4, sync_every=3, use_graph=True)
    with pytest.raises(ValueError, match="index sets"):
        T.EvalStep(model, xs, ops, y, (tr, va), selector=object())
