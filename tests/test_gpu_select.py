"""acm_select_step and acm_copy_if on the device, kernel level: hand-made per-epoch sequences are fed one call at a time and the
state is compared with the restated host loop (tests/select_ref.py) exactly -- ``==`` on doubles and ints, NaN matching NaN --
with guard bands around everything the kernels may write."""
import ctypes as C

import numpy as np
import pytest
import torch

import launch_forms as LF
from select_ref import same_floats, select_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NAN, INF = float("nan"), float("inf")
SENTINEL = -12345.6789          # history rows never written
GUARD_I, GUARD_D = -7777, 4321.25
RULES = ("max_val_acc", "min_val_loss")


def _f32(v):
    return float(np.float32(v))


class _Bench:
    """ctrl / best / history inside guarded allocations, the sequence's inputs on the device, one raw call per epoch."""

    def __init__(self, rows, rule, es, epochs, dtype):
        from acm_gnn_amd import _lib
        self.lib = _lib.load()
        self.rows = [tuple(_f32(v) for v in r) for r in rows]           # what an fp32 pass can produce (fp64 arm: the same numbers)
        self.rule, self.es, self.epochs = rule, es, epochs
        self.ints = torch.full((24,), GUARD_I, dtype=torch.int32, device=DEV)
        self.ints[8:16] = torch.tensor([0, 0, -1, 0, 0, 0, 0, 0], dtype=torch.int32)
        self.dbl = torch.full((6,), GUARD_D, dtype=torch.float64, device=DEV)
        self.dbl[2:4] = 0.0
        self.hist = torch.full((epochs * 5 + 10,), SENTINEL, dtype=torch.float64, device=DEV)
        self.hist[epochs * 5:] = GUARD_D
        self.loss = torch.tensor([r[0] for r in self.rows], dtype=torch.float32, device=DEV)
        self.res = torch.tensor([r[1:] for r in self.rows], dtype=dtype, device=DEV).contiguous()
        p = self.p = _lib.Select()
        p.rule, p.early_stopping, p.epochs = RULES.index(rule), es, epochs
        p.ctrl, p.best, p.history = self.ints[8:].data_ptr(), self.dbl[2:].data_ptr(), self.hist.data_ptr()
        self.calls = 0

    def call(self, k):
        """One launch on row ``k`` of the sequence."""
        from acm_gnn_amd import _lib
        ptr = self.res[k].data_ptr()
        self.p.result, self.p.result_f64 = (ptr, None) if self.res.dtype == torch.float32 else (None, ptr)
        self.p.train_loss = self.loss[k:].data_ptr()
        _lib.check(self.lib.acm_select_step(C.byref(self.p), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "acm_select_step")
        self.calls += 1

    def state(self):
        ints, dbl, hist = self.ints.tolist(), self.dbl.tolist(), self.hist.tolist()
        assert ints[:8] == [GUARD_I] * 8 and ints[16:] == [GUARD_I] * 8 and ints[12:16] == [0] * 4, ints
        assert dbl[:2] == [GUARD_D] * 2 and dbl[4:] == [GUARD_D] * 2, dbl
        assert hist[self.epochs * 5:] == [GUARD_D] * 10
        epoch, stopped, best_epoch, improved = ints[8:12]
        written = [tuple(hist[5 * e:5 * e + 5]) for e in range(epoch)]
        assert all(v == SENTINEL for v in hist[5 * epoch:5 * self.epochs]), "a row beyond the epoch counter was written"
        return dict(epoch=epoch, stopped=stopped, best_epoch=best_epoch, improved=improved, best_key=dbl[2], selected=dbl[3],
                    history=written)

    def check_against_host_loop(self, n_fed):
        """The state after feeding rows 0 .. n_fed - 1 (one call each) equals the host loop over them."""
        selected, history, best_epoch, stop_epoch = select_ref(self.rows[:n_fed], self.rule, self.es, self.epochs)
        st = self.state()
        assert same_floats(st["history"], history), (n_fed, st["history"][-1:], history[-1:])
        assert st["epoch"] == len(history) and st["stopped"] == int(stop_epoch is not None)
        assert st["best_epoch"] == best_epoch and same_floats(st["selected"], selected)
        if best_epoch >= 0:
            r = history[best_epoch]
            assert same_floats(st["best_key"], r[2] if self.rule == "max_val_acc" else -r[4])
        frozen = stop_epoch is not None and n_fed - 1 > stop_epoch or n_fed > self.epochs
        assert st["improved"] == int(not frozen and best_epoch == n_fed - 1)
        return st, stop_epoch


def _feed(rows, rule, es, dtype, epochs=None, every=True):
    b = _Bench(rows, rule, es, len(rows) if epochs is None else epochs, dtype)
    stop = None
    for k in range(len(rows)):
        b.call(k)
        if every or k == len(rows) - 1:
            _, stop = b.check_against_host_loop(k + 1)
    return b, stop


BOTH = pytest.mark.parametrize("dtype", [torch.float32, torch.float64], ids=["fp32", "fp64"])


@BOTH
@pytest.mark.parametrize("name,rows,best_epoch,selected", [
    ("ties", [(.5, .1, .7, .31, 1.), (.4, .2, .7, .32, .9), (.3, .3, .8, .33, .9), (.2, .2, .8, .34, .95), (.2, .2, .75, .35, .9)], 2, .33),
    ("nan_first", [(.5, .1, NAN, .31, 1.), (.4, .2, .1, .32, .9), (.3, .3, .2, .33, .9)], 2, .33),
    ("nan_middle", [(.5, .1, .4, .31, 1.), (.4, .2, NAN, .32, .9), (.3, .3, .2, .33, .9), (.3, .3, .5, .34, .9)], 3, .34),
    ("all_nan", [(.5, .1, NAN, .31, NAN)] * 4, -1, 0.0),
    ("minus_inf_first", [(.5, .1, -INF, .31, 1.), (.4, .2, -INF, .32, .9), (.3, .3, -1e30, .33, .9)], 2, .33),
    ("minus_inf_only", [(.5, .1, -INF, .31, 1.), (.4, .2, -INF, .32, .9)], 0, .31),
])
def test_rule_max_metric(name, rows, best_epoch, selected, dtype):
    b, _ = _feed(rows, "max_val_acc", 0, dtype)
    st = b.state()
    assert st["best_epoch"] == best_epoch and st["selected"] == _f32(selected) and st["stopped"] == 0


@BOTH
def test_rule_min_loss_selects_like_the_host_loop(dtype):
    rows = [(.5, .1, .7, .31, 1.), (.4, .2, .7, .32, NAN), (.3, .3, .8, .33, .9), (.2, .2, .8, .34, .9), (.2, .2, .8, .35, INF),
            (.2, .2, .8, .36, .5), (.2, .2, .8, .37, -0.0)]
    b, stop = _feed(rows, "min_val_loss", 0, dtype)
    assert stop is None and b.state()["best_epoch"] == 6
    b, _ = _feed([(.5, .1, .7, .31, INF), (.5, .1, .7, .32, INF)], "min_val_loss", 0, dtype)          # key -inf: a valid first selection
    assert b.state()["best_epoch"] == 0 and b.state()["best_key"] == -INF


WINDOWS = [1, 3, 63, 64, 65, 200]          # around the 64-wide chunks the window is fetched in


@BOTH
@pytest.mark.parametrize("es", WINDOWS)
def test_early_stop_first_possible_epoch(es, dtype):
    """The condition holds from epoch ``es`` on but may be looked at from ``es + 1`` on: the run stops exactly there."""
    rows = [(.5, .1, .5, .3, 1.0)] * es + [(.5, .1, .5, .3, 5.0), (.5, .1, .5, .3, 10.0)] + [(.5, .1, .5, .3, 20.0)] * 3
    b, stop = _feed(rows, "min_val_loss", es, dtype, every=es <= 65)
    assert stop == es + 1 and b.state()["epoch"] == es + 2


@BOTH
@pytest.mark.parametrize("es", WINDOWS)
def test_equal_to_the_mean_is_not_greater(es, dtype):
    """A constant fp32 loss: every window sum is exact in float64, the mean IS the loss, the run goes on."""
    rows = [(.5, .1, .5, .3, 0.7)] * (es + 6)
    b, stop = _feed(rows, "min_val_loss", es, dtype, every=False)
    assert stop is None and b.state()["epoch"] == es + 6


@BOTH
@pytest.mark.parametrize("es", WINDOWS)
def test_window_sums_in_epoch_order(es, dtype):
    """A window whose float64 sum depends on the order of its additions: the loss ``es`` first, then ``es - 1`` losses of
    -3/8 ulp(es).  Added in epoch order every one of them is rounded away, the sum stays ``es`` and the mean is exactly 1.0: a
    current loss of 1.0 is not greater.  Any order that lets the small terms meet first (backwards, pairwise, per lane) ends
    below ``es`` and would stop the run here."""
    ulp = float(es) - float(np.nextafter(float(es), 0.0))            # the spacing of float64 just below es
    tiny = -0.375 * ulp
    assert _f32(tiny) == tiny and float(es) + tiny == float(es) and (es < 3 or (es - 1) * tiny + float(es) < float(es))
    vals = [1.0, float(es)] + [tiny] * (es - 1) + [1.0, 0.25, 7.0]
    rows = [(.5, .1, .5, .3, v) for v in vals]
    b, stop = _feed(rows, "min_val_loss", es, dtype, every=es <= 65)
    assert stop is None or stop > es + 1


@BOTH
@pytest.mark.parametrize("es", WINDOWS)
def test_nan_in_the_window_and_as_the_current_loss_never_stops(es, dtype):
    big = (.5, .1, .5, .3, 50.0)
    rows = [(.5, .1, .5, .3, 1.0)] * (es + 1) + [(.5, .1, .5, .3, NAN)] + [big] * es + [(.5, .1, .5, .3, 1.0), (.5, .1, .5, .3, 99.0)]
    # epoch es + 1: the current loss is NaN; the next es epochs hold 50 > 1 but the NaN is in their window; then it has left
    b, stop = _feed(rows, "min_val_loss", es, dtype, every=es <= 65)
    assert stop == 2 * es + 3, stop


@BOTH
def test_after_a_stop_nothing_changes(dtype):
    rows = [(.5, .1, .5, .3, 1.0)] * 4 + [(.5, .1, .5, .3, 5.0), (.4, .9, .9, .9, 0.01)]
    b = _Bench(rows, "min_val_loss", 3, 80, dtype)
    for k in range(5):
        b.call(k)
    st, stop = b.check_against_host_loop(5)
    assert stop == 4 and st["stopped"] == 1 and st["epoch"] == 5
    ints, dbl, hist = b.ints.clone(), b.dbl.clone(), b.hist.clone()
    for _ in range(70):
        b.call(5)                           # would be the best epoch by far
    after = b.state()
    assert after["improved"] == 0 and after["best_epoch"] == st["best_epoch"] and after["epoch"] == 5
    ints[11] = 0
    assert torch.equal(b.ints, ints) and torch.equal(b.dbl, dbl) and torch.equal(b.hist.view(torch.int64), hist.view(torch.int64))


@BOTH
@pytest.mark.parametrize("rule", RULES)
def test_at_the_budget_nothing_changes(rule, dtype):
    rows = [(.5, .1, .1 * k, .3, 1.0 / (k + 1)) for k in range(8)]        # ever better: every call within the budget improves
    b = _Bench(rows, rule, 0, 5, dtype)
    for k in range(5):
        b.call(k)
    st, _ = b.check_against_host_loop(5)
    assert st["epoch"] == 5 and st["improved"] == 1 and st["best_epoch"] == 4
    dbl, hist = b.dbl.clone(), b.hist.clone()
    for k in range(5, 8):
        b.call(k)
    after = b.state()
    assert after["epoch"] == 5 and after["improved"] == 0 and after["best_epoch"] == 4 and after["stopped"] == 0
    assert torch.equal(b.dbl, dbl) and torch.equal(b.hist, hist)


# ---------------------------------------------------------------------------------------------------- acm_copy_if
SIZES = [0, 1, 3, 4, 5, 1023, 1024, 1025, 65537]
SPECIALS = [0x7FC00001, 0xFFC12345, 0x7F800001, 0x80000000, 0x00000000, 0xFF800000, 0x00000001]       # NaN payloads, -0.0, ...
PAD = 8                                                                  # guard words on both sides of every tensor


def _tables(n_tensors):
    if n_tensors == len(SIZES):
        return list(SIZES)
    small = [s for s in SIZES if s < 65537]
    return [small[(3 * k + 1) % len(small)] for k in range(n_tensors - 1)] + [65537]


def _layout(sizes, offset):
    """Word offsets of the tensors in one buffer: every tensor starts ``offset`` words behind a 16-byte boundary."""
    at, starts = PAD, []
    for s in sizes:
        at = (at + 3) // 4 * 4 + offset
        starts.append(at)
        at += s + PAD
    return starts, at + PAD


@pytest.mark.parametrize("n_tensors", [len(SIZES), 1, 40, 41, 81])
def test_copy_if_is_bitwise_predicated_and_in_bounds(n_tensors):
    _check_copy_if(_tables(n_tensors), n_tensors)


@pytest.mark.parametrize("sizes", LF.COPY_TABLES, ids=lambda t: "+".join(str(s) for s in t))
def test_copy_if_is_bitwise_where_a_block_takes_several_rounds(sizes):
    """Tensors of more than CHUNK * MAX_BLOCKS words: every block copies several rounds of CHUNK words; 2 097 152 is the last
    size with one round, 2 097 153 the first with two (and a one-word tail), 4 194 309 takes three."""
    _check_copy_if(sizes, len(sizes))


def _check_copy_if(sizes, seed):
    from acm_gnn_amd import _lib, functional as AF
    rng = np.random.default_rng(seed)
    for src_off in (0, 1):
        for dst_off in (0, 1):
            s_at, s_len = _layout(sizes, src_off)
            d_at, d_len = _layout(sizes, dst_off)
            src_np = rng.integers(-2 ** 31, 2 ** 31, s_len, dtype=np.int64).astype(np.int32)
            for k, (a, n) in enumerate(zip(s_at, sizes)):
                for j in range(min(n, len(SPECIALS))):
                    src_np[a + (j * 37 + k) % n] = np.array(SPECIALS[j], np.uint32).view(np.int32)
            dst_np = np.full(d_len, 0x5A5A5A5A, np.int32)
            src, dst = torch.from_numpy(src_np).to(DEV), torch.from_numpy(dst_np).to(DEV)
            assert src.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0
            pairs = [(src[a:a + n].view(torch.float32), dst[b:b + n].view(torch.float32)) for a, b, n in zip(s_at, d_at, sizes)]
            assert all(p[0].numel() == 0 or p[0].data_ptr() % 16 == 4 * src_off for p in pairs)
            assert all(p[1].numel() == 0 or p[1].data_ptr() % 16 == 4 * dst_off for p in pairs)
            flag = torch.zeros(3, dtype=torch.int32, device=DEV)
            AF.copy_if(pairs, flag[1:])
            assert torch.equal(dst.cpu(), torch.from_numpy(dst_np)), "flag 0 must leave dst untouched"
            flag[1] = -3                                                 # any non-zero value
            AF.copy_if(pairs, flag[1:])
            want = dst_np.copy()
            for a, b, n in zip(s_at, d_at, sizes):
                want[b:b + n] = src_np[a:a + n]
            got = dst.cpu().numpy()
            assert np.array_equal(got, want), (src_off, dst_off, int(np.flatnonzero(got != want)[0]))
            assert torch.equal(src.cpu(), torch.from_numpy(src_np))


# ---------------------------------------------------------------------------------------------------- capture
@pytest.mark.parametrize("rule,es", [("max_val_acc", 0), ("min_val_loss", 3)])
def test_captured_selection_and_snapshot_equal_the_eager_ones(rule, es):
    """acm_select_step + acm_copy_if captured once and replayed over a 12-epoch sequence: the same state as eager calls."""
    from acm_gnn_amd import functional as AF
    rng = np.random.default_rng(3)
    rows = [(float(rng.random()), float(rng.random()), float(rng.integers(0, 6)) / 5, float(rng.random()),
             float(1.0 + 0.2 * np.sin(k) + 0.05 * k)) for k in range(12)]
    rows = [tuple(_f32(v) for v in r) for r in rows]
    want = select_ref(rows, rule, es)

    def run(captured):
        params = [torch.zeros(1025, device=DEV), torch.zeros(3, 5, device=DEV)]
        st = AF.SelectionState(rule, es, 12, DEV, params=params)
        loss, res = torch.zeros((), device=DEV), torch.zeros(4, device=DEV)
        graph = None
        if captured:
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                st.launch(loss, res)
            torch.cuda.current_stream().wait_stream(side)
            torch.cuda.synchronize()
            st.reset()
            st.history.zero_()
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                st.launch(loss, res)
        for k, r in enumerate(rows):
            loss.fill_(r[0])
            res.copy_(torch.tensor(r[1:]))
            for p in params:
                p.fill_(float(k + 1))
            graph.replay() if captured else st.launch(loss, res)
        selected, history, best_epoch = st.result()
        assert st.restore()
        return selected, history, best_epoch, st.poll(), [p.clone() for p in params], st.ctrl.clone(), st.best.clone(), st.history.clone()

    eager, cap = run(False), run(True)
    assert same_floats(eager[0], want[0]) and same_floats(eager[1], want[1]) and eager[2] == want[2]
    assert eager[3] == (len(want[1]), want[3] is not None)
    assert same_floats(cap[0], eager[0]) and same_floats(cap[1], eager[1]) and cap[2:4] == eager[2:4]
    for a, b in zip(eager[4:], cap[4:]):
        assert all(torch.equal(u, v) for u, v in zip(a, b)) if isinstance(a, list) else torch.equal(a, b)
    assert all(bool((p == float(want[2] + 1)).all()) for p in eager[4])          # the parameters of the selected epoch
