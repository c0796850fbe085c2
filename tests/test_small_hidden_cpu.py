"""The small-graph step's hidden width, everything that needs no GPU: ``SmallPlan.why_not`` takes widths 32 and 64 and names
the width it refuses, the plan writes the width into ``acm_small_step_t::hidden`` (the former reserved0, same offset), the
real library refuses other widths before it looks at anything else, and -- on the CPU double with a small step that reads
the field (tests/fake_lib_hidden.py) -- the study's ``baselines.GCN(nfeat, 32, ...)`` trains on the small path under
``train.fit`` and ``fit_batched``; runs of two widths in one ``fit_batched`` call fall back and say why."""
import ctypes as C

import numpy as np
import pytest
import torch

import fake_lib_hidden
from select_ref import same_floats
from small_batch_double import install_batch
from test_resident_fit_cpu import _np_copy_if, _np_select_step, _problem


def _install(monkeypatch):
    """test_resident_fit_cpu._install with the width-reading small step and the capability probe of the real library."""
    fake = fake_lib_hidden.install(monkeypatch)
    fake.acm_select_step, fake.acm_copy_if = _np_select_step, _np_copy_if
    fake.acm_small_step_has_hidden = lambda w: int(w in (0,) + fake_lib_hidden.WIDTHS)
    from acm_gnn_amd import train as T
    monkeypatch.setattr(T.TrainStep, "_capture", lambda self: None)
    monkeypatch.setattr(T.EvalStep, "_capture", lambda self: None)
    return install_batch(fake)


def _make(hidden, n=90):
    from acm_gnn_amd import GCN, FusedAdam

    def make(k):
        torch.manual_seed(k)
        model = GCN(50, hidden, 3, 2, n, 0.0, "acmgcn", 0)
        idx = torch.randperm(n, generator=torch.Generator().manual_seed(k))
        return model, FusedAdam(model.parameters(), lr=0.1), idx[:40], idx[40:65], idx[65:]
    return make


def test_the_real_library_says_which_widths_it_has_and_refuses_the_others():
    from acm_gnn_amd import _lib, small
    lib = _lib.load()
    assert lib.acm_version() == 29 == _lib.ABI_VERSION
    assert [int(lib.acm_small_step_has_hidden(w)) for w in (0, 32, 64, 16, 48, 128, -32)] == [1, 1, 1, 0, 0, 0, 0]
    assert small.hidden_widths() == (32, 64)
    assert _lib.SmallStep.hidden.offset == 28 and _lib.SmallStep.hidden.size == 4           # where reserved0 was
    p = _lib.SmallStep()
    p.n_classes, p.n_channels, p.f_in, p.scale = 3, 3, 7, 3.0
    # Stand-ins for the handles and the table: zero-filled host memory far larger than the library's handle struct and than one
    # table entry.  acm_small_step and acm_small_batch_step refuse the width before they look at a handle;
    # acm_small_batch_bind reads the operator's row count (for the slots' overlap check) first, then refuses the width before
    # anything else of the handle or a byte of the table is touched.
    handle, handle_x, table = (C.create_string_buffer(1 << 16) for _ in range(3))
    for width in (16, 48, 128):
        p.hidden = width
        assert lib.acm_small_step(handle, None, None, C.byref(p), None) == 4
        assert b"hidden width %d" % width in lib.acm_last_error()
        slots = (C.POINTER(_lib.SmallStep) * 1)(C.pointer(p))
        assert lib.acm_small_batch_bind(handle, None, None, 1, slots, table, len(table), None) == 4
        assert b"hidden width %d" % width in lib.acm_last_error()
        assert lib.acm_small_batch_step(handle, handle_x, None, 1, C.byref(p), table, None) == 4
        assert b"hidden width %d" % width in lib.acm_last_error()
    assert handle.raw == handle_x.raw == table.raw == bytes(1 << 16)


def test_a_library_without_the_probe_is_offered_64_only(monkeypatch):
    import fake_lib
    fake_lib.install(monkeypatch)                       # the double as it stands: 64 written in, no probe
    from acm_gnn_amd import small
    from acm_gnn_amd.small import SmallPlan
    assert small.hidden_widths() == (64,)
    ops, xs, y, _ = _problem()
    model, opt = _make(32)(0)[:2]
    assert SmallPlan.why_not(model, xs, ops, opt) == "hidden width 32 (64)"


def test_why_not_takes_32_and_64_and_names_the_width_it_refuses(monkeypatch):
    _install(monkeypatch)
    from acm_gnn_amd.small import SmallPlan
    ops, xs, y, _ = _problem()
    for hidden in (32, 64):
        model, opt = _make(hidden)(0)[:2]
        assert SmallPlan.why_not(model, xs, ops, opt) is None, hidden
    for hidden in (16, 48, 128):
        model, opt = _make(hidden)(0)[:2]
        assert SmallPlan.why_not(model, xs, ops, opt) == f"hidden width {hidden} (32 | 64)"


def test_the_plan_writes_the_width_into_the_struct(monkeypatch):
    _install(monkeypatch)
    from acm_gnn_amd import train as T
    from acm_gnn_amd.small import SmallPlan
    ops, xs, y, _ = _problem()
    w = T.row_weights(torch.arange(40), 90)
    for hidden in (32, 64):
        model, opt = _make(hidden)(0)[:2]
        plan = SmallPlan(model, xs, ops, y, w, opt, keep_grads=True)
        assert plan.p.hidden == hidden and plan.hidden == hidden
        assert plan.grads[(0, "weight_low")].shape == (50, hidden) and plan.grads[(1, "weight_low")].shape == (hidden, 3)
        assert plan.grads[(0, "att_vec_low")].numel() == hidden


def test_the_study_model_at_32_trains_on_the_small_path(monkeypatch):
    fake = _install(monkeypatch)
    from acm_gnn_amd import FusedAdam, baselines, train as T
    ops, xs, y, _ = _problem()
    n = 90
    torch.manual_seed(0)
    model = baselines.GCN(50, 32, 3, 0.0, "acmgcn", nnodes=n)
    opt = FusedAdam(model.parameters(), lr=0.05)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(1))
    before = [p.detach().clone() for p in model.parameters()]
    fake.small_calls, fake.small_widths = 0, []
    sel, hist = T.fit(model, opt, xs, ops, y, idx[:40], idx[40:65], idx[65:], 4, use_graph=True)
    assert fake.small_calls >= 8 and set(fake.small_widths) == {32}            # a step and an evaluation pass per epoch
    assert len(hist) == 4 and all(np.isfinite(h[0]) for h in hist) and hist[-1][0] < hist[0][0]
    assert any(not torch.equal(u, v) for u, v in zip(before, model.parameters()))


def test_fit_batched_at_32_does_not_fall_back_and_mixed_widths_do(monkeypatch):
    fake = _install(monkeypatch)
    from acm_gnn_amd import train as T
    ops, xs, y, _ = _problem()
    make = _make(32)
    want = T.fit_concurrent([make(k) for k in range(4)], xs, ops, y, epochs=6, rule="min_val_loss", sync_every=4)
    fake.small_batch_calls, fake.small_widths = 0, []
    got = T.fit_batched([make(k) for k in range(4)], xs, ops, y, 6, rule="min_val_loss", batch=2, sync_every=4)
    assert T.fit_batched.last_refusal is None and fake.small_batch_calls > 0 and set(fake.small_widths) == {32}
    for k in range(4):
        assert same_floats(got[k][0], want[k][0]) and same_floats(got[k][1], want[k][1]), k
    mixed = [make(0), _make(64)(1), make(2)]
    fake.small_batch_calls = 0
    out = T.fit_batched(mixed, xs, ops, y, 3, batch=2, sync_every=4)
    why = T.fit_batched.last_refusal
    assert why is not None and "run 1" in why and "hidden width 64" in why and "configured differently" in why, why
    assert fake.small_batch_calls == 0 and len(out) == 3 and all(len(h) == 3 for _, h in out)
