"""The loss-row attachment (acm_csr_build_loss_rows, acm_conv_fwd_tail_rows) without a GPU: the host-side
list as a stand-alone program (plain and under the address + undefined-behaviour sanitizers), and the host
wiring on the numpy double of the C ABI, which has none of the new symbols: train.TrainStep then keeps today's path."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import fake_lib
from conftest import ROOT


@pytest.mark.parametrize("sanitize", [False, True])
def test_filtered_work_list_on_the_host(tmp_path, sanitize):
    """tests/c_abi/loss_rows_check.cpp over csrc/acm_items.h: every kept row's edges once and no dropped row, the full
    list's pieces for the kept long rows, no row across a window, consecutive slots."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = tmp_path / "loss_rows_check"
    flags = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"] if sanitize else []
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-Wall", "-Werror", *flags, "-I", os.path.join(ROOT, "acm_gnn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_abi", "loss_rows_check.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "loss_rows_check: ok" in out.stdout, (out.stdout, out.stderr)


def test_new_symbols_are_declared_exported_and_listed():
    from acm_gnn_amd import _lib, tuning
    lib = _lib.load()
    assert lib.acm_version() == 29                                     # new entry points, same ABI number
    assert set(_lib.LOSS_ROWS_SYMBOLS) == {"acm_csr_build_loss_rows", "acm_csr_loss_rows_info", "acm_conv_fwd_tail_rows"}
    for name in _lib.LOSS_ROWS_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    # without a device: argument errors, never success
    out = (C.c_int64 * 4)(*([7] * 4))
    assert lib.acm_csr_build_loss_rows(None, None) == 1 and b"acm_csr_build_loss_rows" in lib.acm_last_error()
    assert lib.acm_csr_loss_rows_info(None, out) == 1
    assert lib.acm_conv_fwd_tail_rows(None, None, None, None, None, 0, None, 0, None) == 1
    assert not hasattr(lib, "acm_conv_bwd_spmm_rows")                  # (the backward form: measured, no gain, not kept -- EXPERIMENTS.md)
    # the switch is a host key of its own: default on, 0 / 1, not a bit of `rewrites`
    assert tuning.HOST_DEFAULTS["loss_rows"] == 1 and tuning.HOST_RANGES["loss_rows"] == (0, 1)
    assert tuning.parse("loss_rows=0") == ({}, {"loss_rows": 0})
    with pytest.raises(ValueError):
        tuning.parse("loss_rows=2")
    with tuning.override(loss_rows=0):
        assert tuning.HOST.loss_rows == 0 and tuning.HOST.rewrites == 15
    assert tuning.HOST.loss_rows == 1


def _setup(dropped=0.5, seed=3):
    from acm_gnn_amd import GCN, data as D
    from acm_gnn_amd.graph import CsrGraph, FilterOperators
    adj, x_np, y_np, _, _ = D.synthetic_dataset("tiny", seed=seed)
    low, _ = D.build_filters(adj)
    ops = FilterOperators(CsrGraph.from_scipy(low, "cpu"))
    x, y = torch.from_numpy(D.row_normalize_features(x_np)), torch.from_numpy(y_np)
    n = x.shape[0]
    w = torch.zeros(n)
    kept = torch.randperm(n, generator=torch.Generator().manual_seed(seed))[: n - int(round(dropped * n))]
    w[kept] = 1.0 / max(kept.numel(), 1)
    torch.manual_seed(0)
    model = GCN(x.shape[1], 16, int(y.max()) + 1, 2, n, 0.0, "acmgcnp", 0)
    return model, ops, x, y, w


def _record_calls(monkeypatch, fake):
    calls = []
    for name in dir(fake):
        fn = getattr(fake, name)
        if name.startswith("acm_") and callable(fn) and name not in ("acm_last_error", "acm_version"):
            monkeypatch.setattr(fake, name, (lambda o, nm: lambda *a: (calls.append(nm), o(*a))[1])(fn, name))
    return calls


def test_the_double_has_no_loss_row_symbols_and_the_step_runs_as_before(monkeypatch):
    fake = fake_lib.install(monkeypatch)
    from acm_gnn_amd import FusedAdam, _lib, train as T, tuning
    assert all(getattr(fake, name, None) is None for name in _lib.LOSS_ROWS_SYMBOLS)
    calls = _record_calls(monkeypatch, fake)
    runs = {}
    for switch in (1, 1, 0):                    # (the first pass is a warm-up: one-off queries such as acm_tuning_get happen there)
        with tuning.override(loss_rows=switch):
            model, ops, x, y, w = _setup()
            step = T.TrainStep(model, FusedAdam(model.parameters(), lr=0.01, weight_decay=5e-4), x, ops, y, w)
            assert step.loss_rows is None
            assert ("lacks" in step.loss_rows_refused) if switch else ("loss_rows=0" in step.loss_rows_refused)
            calls.clear()
            losses = [float(step()) for _ in range(4)]
            runs[switch] = (list(calls), losses, [p.detach().clone() for p in model.parameters()])
    assert runs[1][0] == runs[0][0] and "acm_conv_fwd_tail" in runs[1][0] and "acm_conv_bwd_spmm" in runs[1][0]
    assert not any(name.endswith("_rows") for name in runs[1][0])
    assert runs[1][1] == runs[0][1] and np.isfinite(runs[1][1]).all() and runs[1][1][-1] < runs[1][1][0]       # it trains
    assert all(torch.equal(a, b) for a, b in zip(runs[1][2], runs[0][2]))


def _stub_loss_rows(monkeypatch, fake, launch_status=4):
    """Stand-ins for the three symbols on the double: the builds succeed and are counted, the launch answers
    ACM_EUNSUPPORTED (the caller then makes today's call)."""
    log = {"build": [], "fwd": 0}

    def build(h, keep):
        log["build"].append(1)
        return 0

    def info(h, out):
        for i, v in enumerate((10, 20, 0, 30)):
            out[i] = v
        return 0

    monkeypatch.setattr(fake, "acm_csr_build_loss_rows", build, raising=False)
    monkeypatch.setattr(fake, "acm_csr_loss_rows_info", info, raising=False)
    monkeypatch.setattr(fake, "acm_conv_fwd_tail_rows", lambda *a: (log.__setitem__("fwd", log["fwd"] + 1), launch_status)[1], raising=False)
    return log


def test_one_row_in_eight_is_the_condition_and_the_criterion_counts(monkeypatch):
    fake = fake_lib.install(monkeypatch)
    from acm_gnn_amd import FusedAdam, train as T
    log = _stub_loss_rows(monkeypatch, fake)
    for dropped, built in ((0.0, False), (0.10, False), (0.13, True), (0.5, True), (1.0, True)):
        model, ops, x, y, w = _setup(dropped)
        n_zero = int((w == 0).sum())
        assert (n_zero >= w.numel() / 8) == built, (dropped, n_zero)           # (the shapes straddle the bar as meant)
        step = T.TrainStep(model, FusedAdam(model.parameters(), lr=0.01), x, ops, y, w)
        assert (step.loss_rows is not None) == built, (dropped, step.loss_rows_refused)
        if not built:
            assert "one row in eight" in step.loss_rows_refused
        else:
            assert step.loss_rows_refused is None and step.loss_rows.keep.dtype == torch.uint8
            assert torch.equal(step.loss_rows.keep.bool(), w != 0)
    model, ops, x, y, w = _setup(0.5)
    n_builds = len(log["build"])
    step = T.TrainStep(model, FusedAdam(model.parameters(), lr=0.01), x, ops, y, w, criterion="bce")
    assert step.loss_rows is None and "bce" in step.loss_rows_refused and len(log["build"]) == n_builds


def test_attachment_is_cached_per_weights_rebuilt_on_an_edit_and_falls_back_on_eunsupported(monkeypatch):
    fake = fake_lib.install(monkeypatch)
    from acm_gnn_amd import FusedAdam, train as T
    log = _stub_loss_rows(monkeypatch, fake)
    model, ops, x, y, w = _setup(0.5)
    step = T.TrainStep(model, FusedAdam(model.parameters(), lr=0.01), x, ops, y, w)
    first = step.loss_rows
    assert first is not None and log["build"] == [1]              # the row list, on A_low
    assert ops.loss_rows(w) is first and log["build"] == [1]      # cached: same tensor, same version
    calls = _record_calls(monkeypatch, fake)
    assert np.isfinite(float(step())) and log["fwd"] == 1
    # ACM_EUNSUPPORTED from the _rows tail: today's calls
    assert calls.count("acm_conv_fwd_tail") == 1 and calls.count("acm_conv_bwd_spmm") == 1
    # another live step with other weights on the same operators: refused, the first keeps its attachment
    model2, _, _, _, _ = _setup(0.5)
    w2 = w.clone()
    other = T.TrainStep(model2, FusedAdam(model2.parameters(), lr=0.01), x, ops, y, w2)
    assert other.loss_rows is None and "refused" in other.loss_rows_refused and log["build"] == [1]
    # an in-place edit of the weights bumps _version: the next eager step re-attaches before it launches
    w[int(torch.nonzero(w == 0)[0])] = 0.25
    assert not first.current_for(w)
    assert np.isfinite(float(step()))
    assert log["build"] == [1, 1] and step.loss_rows is not first and step.loss_rows.current_for(w)
    assert torch.equal(step.loss_rows.keep.bool(), w != 0)
    assert np.isfinite(float(step())) and log["build"] == [1, 1]


def test_operators_that_cannot_carry_the_attachment_answer_none(monkeypatch):
    fake = fake_lib.install(monkeypatch)
    from acm_gnn_amd.graph import FilterOperators
    log = _stub_loss_rows(monkeypatch, fake)
    _, ops, _, _, w = _setup(0.5)
    implicit = FilterOperators(ops.low, row_scale=torch.ones(ops.low.n_rows))
    lr = implicit.loss_rows(w)
    assert lr is not None and log["build"] == [1] and implicit.loss_rows(w) is lr
    # sharded or general operator sets, or weights of another length: no attachment
    assert implicit.loss_rows(w[:-1]) is None
    implicit.general = True
    assert implicit.loss_rows(w.clone()) is None and log["build"] == [1]
