"""A batch of small-graph runs in the same launches, everything that needs no GPU: the five entry points are exported (ABI still
29), the new struct has the C layout, the real library refuses bad slot tables before any launch, the host-side validation
survives the host sanitizers on crafted slot arrays, and -- on the CPU double with the batched entries looped over its own
single-run functions -- ``fit_batched`` returns exactly what ``fit_concurrent(sync_every=...)`` returns."""
import ctypes as C
import os
import shutil
import subprocess

import pytest
import torch

from conftest import ROOT
from select_ref import same_floats
from small_batch_double import install_batch
from test_resident_fit_cpu import EPOCHS, _install, _problem

NEW = ("acm_small_batch_table_bytes", "acm_small_batch_bind", "acm_small_batch_step", "acm_eval_metrics_batch", "acm_select_step_batch")


# ------------------------------------------------------------------------------------------------ the real library, no GPU
def test_new_symbols_are_exported_and_the_abi_is_still_29():
    from acm_gnn_amd import _lib
    lib = _lib.load()
    assert lib.acm_version() == 29 == _lib.ABI_VERSION
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert _lib.SMALL_BATCH_MAX == 32
    text = open(os.path.join(ROOT, "include", "acm_hip.h")).read()
    assert "#define ACM_SMALL_BATCH_MAX 32" in text


def test_new_struct_has_the_c_layout(tmp_path):
    from acm_gnn_amd import _lib
    structs = {"acm_eval_metrics_slot_t": _lib.EvalMetricsSlot, "acm_select_t": _lib.Select, "acm_small_step_t": _lib.SmallStep}
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


def _block(base, **kw):
    """A slot block whose pointers are never dereferenced: every call below is refused."""
    from acm_gnn_amd import _lib
    p = _lib.SmallStep()
    p.n_classes, p.n_channels, p.train, p.update, p.f_in, p.scale = 3, 3, 1, 1, 7, 3.0
    p.x_vals, p.row_scale = 0x100, 0x200
    p.workspace, p.workspace_bytes = base, 4096
    p.logits, p.loss, p.att1, p.att2 = base + 0x2000, base + 0x4000, base + 0x5000, base + 0x6000
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _slots(blocks):
    from acm_gnn_amd import _lib
    arr = (C.POINTER(_lib.SmallStep) * len(blocks))()
    for i, b in enumerate(blocks):
        arr[i] = C.pointer(b) if b is not None else None
    return arr


def test_the_library_refuses_bad_slot_tables_before_any_launch():
    from acm_gnn_amd import _lib
    lib = _lib.load()
    EINVAL, ESHAPE, EUNSUPPORTED = 1, 2, 4
    nbytes = C.c_size_t()
    assert lib.acm_small_batch_table_bytes(0, C.byref(nbytes)) == EINVAL and b"n_slots" in lib.acm_last_error()
    assert lib.acm_small_batch_table_bytes(33, C.byref(nbytes)) == EUNSUPPORTED and b"33" in lib.acm_last_error()
    assert lib.acm_small_batch_table_bytes(4, None) == EINVAL
    assert lib.acm_small_batch_table_bytes(32, C.byref(nbytes)) == 0 and nbytes.value % 32 == 0 and nbytes.value // 32 >= 2 * 1800
    per_slot = nbytes.value // 32
    a, b = _block(0x10000000), _block(0x20000000)
    two = _slots([a, b])

    def bind(n, slots, table=0x7000000, table_bytes=1 << 20):
        return lib.acm_small_batch_bind(None, None, None, n, slots, table, table_bytes, None)

    assert bind(0, two) == EINVAL and b"n_slots" in lib.acm_last_error()
    many = _slots([a] * 33)
    assert bind(33, many) == EUNSUPPORTED and b"33" in lib.acm_last_error()
    assert bind(2, None) == EINVAL and b"NULL" in lib.acm_last_error()
    assert bind(2, two, table=None) == EINVAL and b"table" in lib.acm_last_error()
    assert bind(2, two, table_bytes=2 * per_slot - 1) == ESHAPE and b"table" in lib.acm_last_error()
    assert bind(3, _slots([None, None, None])) == EINVAL and b"empty" in lib.acm_last_error()
    for field, word in (("n_classes", b"n_classes"), ("n_channels", b"n_channels"), ("train", b"train")):
        odd = _block(0x20000000, **{field: getattr(a, field) + 1 if field != "train" else 0})
        assert bind(3, _slots([a, None, odd])) == EINVAL, field
        assert word in lib.acm_last_error() and b"disagree" in lib.acm_last_error(), lib.acm_last_error()
    close = _block(0x10000000 + 4095)                     # its workspace begins on the last byte of a's
    assert bind(2, _slots([a, close])) == EINVAL and b"overlap" in lib.acm_last_error() and b"workspace" in lib.acm_last_error()
    same_loss = _block(0x20000000, loss=a.loss)
    assert bind(2, _slots([a, same_loss])) == EINVAL and b"loss" in lib.acm_last_error()
    # a table nothing is wrong with still needs its handles: refused (no launch, no copy) for the missing operator
    assert bind(2, two) == EINVAL and b"operator" in lib.acm_last_error()
    # the step and the two table-driven launches
    assert lib.acm_small_batch_step(None, None, None, 0, C.byref(a), 0x7000000, None) == EINVAL and b"n_slots" in lib.acm_last_error()
    assert lib.acm_small_batch_step(None, None, None, 33, C.byref(a), 0x7000000, None) == EUNSUPPORTED
    assert lib.acm_small_batch_step(None, None, None, 2, C.byref(a), 0x7000000, None) == EINVAL and b"NULL" in lib.acm_last_error()
    assert lib.acm_eval_metrics_batch(10, 3, 3, 10, 3, 1, 2, None, 1 << 10, None) == EINVAL and b"table" in lib.acm_last_error()
    assert lib.acm_eval_metrics_batch(10, 3, 3, 10, 3, 1, 33, 0x7000000, 1 << 10, None) == EUNSUPPORTED
    assert lib.acm_eval_metrics_batch(10, 3, 3, 10, 3, 1, 0, 0x7000000, 1 << 10, None) == EINVAL
    assert lib.acm_eval_metrics_batch(10, 3, 2, 10, 3, 1, 2, 0x7000000, 1 << 10, None) == ESHAPE
    assert lib.acm_eval_metrics_batch(10, 3, 3, 10, 3, 1, 2, 0x7000000, 4, None) == 5 and b"workspace" in lib.acm_last_error()
    assert lib.acm_select_step_batch(0, 0x7000000, None) == EINVAL and b"n_slots" in lib.acm_last_error()
    assert lib.acm_select_step_batch(33, 0x7000000, None) == EUNSUPPORTED
    assert lib.acm_select_step_batch(2, None, None) == EINVAL and b"table" in lib.acm_last_error()


def test_host_side_validation_under_the_host_sanitizers(tmp_path):
    """tests/c_abi/small_batch_host.cpp: the slot-array checks of acm_small_batch_bind (a header of plain host C++) on crafted
    arrays -- empty slots, the maximum count, ranges that touch and overlap at both ends of the address space -- built with
    AddressSanitizer and UBSan for the host and run here, on the CPU."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = tmp_path / "small_batch_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "acm_gnn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_abi", "small_batch_host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "small_batch_host: ok" in out.stdout, (out.stdout, out.stderr)


# ------------------------------------------------------------------------------------------------ the CPU double
@pytest.mark.parametrize("rule,es", [("min_val_loss", 3), ("max_val_acc", 0)])
def test_fit_batched_equals_fit_concurrent_on_the_double(monkeypatch, rule, es):
    fake = install_batch(_install(monkeypatch))
    from acm_gnn_amd import train as T
    ops, xs, y, make = _problem()
    for sync in (4, 64):
        want = T.fit_concurrent([make(k) for k in range(4)], xs, ops, y, epochs=EPOCHS, rule=rule, early_stopping=es, sync_every=sync)
        fake.small_batch_calls = 0
        got = T.fit_batched([make(k) for k in range(4)], xs, ops, y, EPOCHS, rule=rule, early_stopping=es, batch=2, sync_every=sync)
        assert T.fit_batched.last_refusal is None and fake.small_batch_calls > 0
        for k in range(4):
            assert same_floats(got[k][0], want[k][0]) and same_floats(got[k][1], want[k][1]), (sync, k)
    if es:
        assert any(len(h) < EPOCHS for _, h in want), "no run stops early: the hand-over at different epochs is not exercised"


def _looks(lengths, slots, sync, epochs):
    """The batched loop's schedule restated on the runs' history lengths: per look, (the runs that leave, the slots that were
    empty during it).  A run leaves at the first look by which its last epoch (the stop, or the budget) has been enqueued."""
    pending, out = list(range(len(lengths))), []
    live = [pending.pop(0) for _ in range(min(slots, len(lengths)))]
    done = {k: 0 for k in range(len(lengths))}
    while any(k is not None for k in live):
        todo = min(sync, max(epochs - done[k] for k in live if k is not None))
        empty = sum(k is None for k in live)
        leaving = []
        for i, k in enumerate(live):
            if k is not None:
                done[k] += todo
                if done[k] >= lengths[k]:
                    leaving.append(k)
                    live[i] = pending.pop(0) if pending else None
        out.append((leaving, empty))
    return out


def test_fit_batched_hands_two_slots_over_in_one_look_and_ends_with_an_empty_slot(monkeypatch):
    """More runs than slots (5 on 2): two runs leave in the same look, both slots are handed over by table writes before the next
    replay, and the last run trains beside an empty slot."""
    fake = install_batch(_install(monkeypatch))
    from acm_gnn_amd import train as T
    ops, xs, y, make = _problem()
    want = T.fit_concurrent([make(k) for k in range(5)], xs, ops, y, epochs=EPOCHS, rule="min_val_loss", early_stopping=3, sync_every=4)
    fake.small_batch_calls = 0
    got = T.fit_batched([make(k) for k in range(5)], xs, ops, y, EPOCHS, rule="min_val_loss", early_stopping=3, batch=2, sync_every=4)
    assert T.fit_batched.last_refusal is None and fake.small_batch_calls > 0
    for k in range(5):
        assert same_floats(got[k][0], want[k][0]) and same_floats(got[k][1], want[k][1]), k
    assert any(len(h) < EPOCHS for _, h in want), "no run stops early"
    looks = _looks([len(h) for _, h in want], 2, 4, EPOCHS)
    assert any(len(leaving) == 2 for leaving, _ in looks), "no look in which two runs leave"
    assert looks[-1][1] == 1 and looks[-1][0] == [4], "the last look has no empty slot"


def test_fit_batched_falls_back_outside_the_envelope_and_says_why(monkeypatch):
    fake = install_batch(_install(monkeypatch))
    from acm_gnn_amd import GCN, FusedAdam, train as T
    ops, xs, y, make = _problem()

    def runs():
        out = [make(k) for k in range(4)]
        torch.manual_seed(7)
        narrow = GCN(50, 32, 3, 2, 90, 0.0, "acmgcn", 0)             # hidden 32: outside the fused step's envelope
        out[2] = (narrow, FusedAdam(narrow.parameters(), lr=0.1)) + out[2][2:]
        return out

    want = T.fit_concurrent(runs(), xs, ops, y, epochs=EPOCHS, rule="min_val_loss", early_stopping=3, sync_every=4)
    fake.small_batch_calls = 0
    got = T.fit_batched(runs(), xs, ops, y, EPOCHS, rule="min_val_loss", early_stopping=3, batch=2, sync_every=4)
    assert "hidden width 32" in T.fit_batched.last_refusal and "run 2" in T.fit_batched.last_refusal and fake.small_batch_calls == 0
    for k in range(4):
        assert same_floats(got[k][0], want[k][0]) and same_floats(got[k][1], want[k][1]), k
    T.fit_batched([make(0)], xs, ops, y, 2, batch=2, sync_every=4)
    assert T.fit_batched.last_refusal is None                          # the reason does not outlive the call it was about


def test_fit_batched_states_what_it_does_not_do(monkeypatch):
    install_batch(_install(monkeypatch))
    from acm_gnn_amd import train as T
    ops, xs, y, make = _problem()
    for kw in (dict(keep_best=True), dict(criterion="bce"), dict(metric="rocauc")):
        with pytest.raises(NotImplementedError, match="fit_concurrent"):
            T.fit_batched([make(0)], xs, ops, y, 4, **kw)
    with pytest.raises(ValueError, match="batch"):
        T.fit_batched([make(0)], xs, ops, y, 4, batch=33)
    with pytest.raises(ValueError, match="sync_every"):
        T.fit_batched([make(0)], xs, ops, y, 4, sync_every=0)
    assert T.fit_batched([], xs, ops, y, 4) == []


def test_small_batch_says_why_plans_cannot_share_launches(monkeypatch):
    install_batch(_install(monkeypatch))
    from acm_gnn_amd import GCN, FusedAdam, train as T
    from acm_gnn_amd.small import SmallBatch, SmallPlan
    ops, xs, y, make = _problem()
    w = T.row_weights(torch.arange(40), 90)

    def plan(model, train=True, x=xs):
        return SmallPlan(model, x, ops, y, w, FusedAdam(model.parameters(), lr=0.1)) if train else SmallPlan(model, x, ops)

    base = plan(make(0)[0])
    assert SmallBatch.why_not([base, plan(make(1)[0])]) is None
    torch.manual_seed(3)
    assert "configured" in SmallBatch.why_not([base, plan(GCN(50, 64, 3, 2, 90, 0.0, "acmgcn", 0, variant=True))])
    assert "classes" in SmallBatch.why_not([base, plan(GCN(50, 64, 4, 2, 90, 0.0, "acmgcn", 0))])
    assert "training and evaluation" in SmallBatch.why_not([base, plan(make(1)[0], train=False)])
    import copy
    assert "feature" in SmallBatch.why_not([base, plan(make(1)[0], x=copy.copy(xs))])
    assert "slots" in SmallBatch.why_not([base] * 33)
    with pytest.raises(ValueError, match="classes"):
        SmallBatch([base, plan(GCN(50, 64, 4, 2, 90, 0.0, "acmgcn", 0))])
