"""A batch of small-graph runs on DIFFERENT graphs in the same launches, everything that needs no GPU: the three entry points
are exported (ABI still 29), the new struct has the C layout, the real library refuses bad arguments before any launch, slots
that differ only in their features and row scale pass the new handle-free check where the old one refuses them, the host-side
validation survives the host sanitizers on crafted slot arrays, and -- on the CPU double with the new entries looped over its
own single-run function -- ``fit_batched_graphs`` returns exactly what ``fit`` returns run by run."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT
from select_ref import same_floats
from small_batch_double import install_batch
from small_graphs_double import install_graphs
from test_resident_fit_cpu import EPOCHS, _install
from test_small_batch_cpu import _block, _looks, _slots

NEW = ("acm_small_batch_grids", "acm_small_batch_bind_graphs", "acm_small_batch_step_graphs")
EINVAL, ESHAPE, EUNSUPPORTED = 1, 2, 4


# ------------------------------------------------------------------------------------------------ the real library, no GPU
def test_new_symbols_are_exported_and_the_abi_is_still_29():
    from acm_gnn_amd import _lib
    lib = _lib.load()
    assert lib.acm_version() == 29 == _lib.ABI_VERSION
    for name in NEW:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    text = open(os.path.join(ROOT, "include", "acm_hip.h")).read()
    for name in NEW:
        assert f"int {name}(" in text, name
    assert text.count("synthetic-experiments/train.py:64-164") >= 1 and "acm_small_batch_grids_t" in text


def test_new_struct_has_the_c_layout(tmp_path):
    from acm_gnn_amd import _lib
    cname, cls = "acm_small_batch_grids_t", _lib.SmallBatchGrids
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "acm_hip.h"', "int main(void){",
             f'printf("size %zu\\n", sizeof({cname}));']
    for fname, _ in cls._fields_:
        lines.append(f'printf("{fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = dict((ln.split()[0], int(ln.split()[1])) for ln in subprocess.check_output([str(exe)], text=True).splitlines())
    assert got["size"] == C.sizeof(cls) == 20
    assert [f for f, _ in cls._fields_] == ["proj", "wide", "graph", "item_blocks", "red_blocks"]
    for fname, _ in cls._fields_:
        assert got[fname] == getattr(cls, fname).offset, fname


def _nulls(n):
    return (C.c_void_p * n)()


def test_the_library_refuses_bad_arguments_before_any_launch():
    from acm_gnn_amd import _lib
    lib = _lib.load()
    grids = _lib.SmallBatchGrids(4, 4, 4, 4, 4)
    a, b = _block(0x10000000), _block(0x20000000)
    two = _slots([a, b])

    def bind(n, slots, handles="all", grids=grids, table=0x7000000, table_bytes=1 << 20):
        h = [_nulls(max(n, 1)) for _ in range(3)] if handles == "all" else handles
        return lib.acm_small_batch_bind_graphs(n, h[0], h[1], h[2], slots, C.byref(grids) if grids is not None else None, table,
                                               table_bytes, None)

    # NULL handle arrays, each of the three
    for missing in range(3):
        h = [_nulls(2) for _ in range(3)]
        h[missing] = None
        assert bind(2, two, handles=h) == EINVAL and b"NULL handle array" in lib.acm_last_error(), missing
    assert bind(2, two, grids=None) == EINVAL and b"grids" in lib.acm_last_error()
    assert bind(0, two) == EINVAL and b"n_slots" in lib.acm_last_error()
    assert bind(33, _slots([a] * 33)) == EUNSUPPORTED and b"33" in lib.acm_last_error()
    assert bind(2, None) == EINVAL and b"NULL" in lib.acm_last_error()
    assert bind(3, _slots([None, None, None])) == EINVAL and b"empty" in lib.acm_last_error()
    # slots disagreeing in each shared field
    for field, other in (("n_classes", 4), ("n_channels", 4), ("relu_before", 1), ("layernorm", 1), ("train", 0), ("update", 0),
                         ("f_in", 8), ("hidden", 32)):
        odd = _block(0x20000000, **{field: other})
        assert bind(3, _slots([a, None, odd])) == EINVAL, field
        assert field.encode() in lib.acm_last_error() and b"disagree" in lib.acm_last_error(), lib.acm_last_error()
    # overlapping ranges
    close = _block(0x10000000 + 4095)                     # its workspace begins on the last byte of a's
    assert bind(2, _slots([a, close])) == EINVAL and b"overlap" in lib.acm_last_error() and b"workspace" in lib.acm_last_error()
    assert bind(2, _slots([a, _block(0x20000000, loss=a.loss)])) == EINVAL and b"loss" in lib.acm_last_error()
    assert bind(2, _slots([a, _block(0x20000000, logits=a.workspace + 64)])) == EINVAL and b"logits" in lib.acm_last_error()
    # slots that differ ONLY in their features and row scale: the one-graph check refuses them, the new one lets them through
    # to the first thing that needs a handle
    for field in ("x_vals", "row_scale", "xt_vals", "xt_src_pos"):
        other = _slots([a, _block(0x20000000, **{field: 0x900})])
        assert lib.acm_small_batch_bind(None, None, None, 2, other, 0x7000000, 1 << 20, None) == EINVAL
        assert field.encode() in lib.acm_last_error() and b"disagree" in lib.acm_last_error(), field
        assert bind(2, other, table=None) == EINVAL and b"table" in lib.acm_last_error(), field
        assert bind(2, other) == EINVAL and b"operator" in lib.acm_last_error() and b"slot 0" in lib.acm_last_error(), field
    nbytes = C.c_size_t()
    assert lib.acm_small_batch_table_bytes(2, C.byref(nbytes)) == 0
    assert bind(2, two, table_bytes=nbytes.value - 1) == ESHAPE and b"table" in lib.acm_last_error()
    # the grids and the step
    g = _lib.SmallBatchGrids()
    assert lib.acm_small_batch_grids(None, None, None, C.byref(a), C.byref(g)) == EINVAL and b"NULL" in lib.acm_last_error()
    assert lib.acm_small_batch_grids(None, None, None, C.byref(a), None) == EINVAL
    assert bytes(g) == bytes(20)

    def step(n, shape=a, grids=grids, table=0x7000000):
        return lib.acm_small_batch_step_graphs(n, C.byref(shape) if shape is not None else None,
                                               C.byref(grids) if grids is not None else None, table, None)

    assert step(0) == EINVAL and b"n_slots" in lib.acm_last_error()
    assert step(33) == EUNSUPPORTED
    for kw in (dict(shape=None), dict(grids=None), dict(table=None)):
        assert step(2, **kw) == EINVAL and b"NULL" in lib.acm_last_error(), kw
    assert step(2, shape=_block(0x10000000, hidden=48)) == EUNSUPPORTED
    # grids nobody folded (zeros), grids wider than any handle can ask for, a reducing width that is not the hidden width's
    assert step(2, grids=_lib.SmallBatchGrids()) == ESHAPE and b"grids" in lib.acm_last_error()
    assert step(2, grids=_lib.SmallBatchGrids(1, 1 << 20, 1, 1, 4)) == ESHAPE
    assert step(2, grids=_lib.SmallBatchGrids(4, 4, 4, 4, 4)) == ESHAPE


def test_host_side_validation_under_the_host_sanitizers(tmp_path):
    """tests/c_abi/small_graphs_host.cpp: the graph-per-slot flavour of the slot-array checks (a header of plain host C++) on
    crafted arrays, built with AddressSanitizer and UBSan for the host and run here, on the CPU."""
    cxx = shutil.which("g++") or shutil.which("clang++")
    assert cxx, "a host C++ compiler"
    exe = tmp_path / "small_graphs_host"
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "include"), "-I", os.path.join(ROOT, "acm_gnn_amd", "csrc"),
                           os.path.join(ROOT, "tests", "c_abi", "small_graphs_host.cpp"), "-o", str(exe)])
    out = subprocess.run([str(exe)], capture_output=True, text=True)
    assert out.returncode == 0 and "small_graphs_host: ok" in out.stdout, (out.stdout, out.stderr)


# ------------------------------------------------------------------------------------------------ the CPU double
def _graph(seed, n=90, f_in=50):
    """One graph of the study: its own adjacency, its own features, its own labels."""
    import scipy.sparse as sp
    from acm_gnn_amd import SparseFeatures, data as D
    from acm_gnn_amd.distributed import make_sharded_operators
    rng = np.random.default_rng(100 + seed)
    m = n * (3 + seed)                                    # (denser from graph to graph: the handles differ in size)
    r, c = rng.integers(0, n, m), rng.integers(0, n, m)
    adj = sp.csr_matrix((np.ones(m, np.float32), (r, c)), shape=(n, n))
    adj = ((adj + adj.T) > 0).astype(np.float32).tocsr()
    adj.setdiag(0)
    adj.eliminate_zeros()
    low, deg = D.build_filters(adj)
    ops = make_sharded_operators(low, deg, torch.device("cpu"))
    xs = SparseFeatures.from_scipy(sp.csr_matrix(((rng.random((n, f_in)) < 0.08) * 1.0).astype(np.float32)), "cpu")
    y = torch.from_numpy(rng.integers(0, 3, n))
    return xs, ops, y


def _runs(graphs, n_runs):
    """Run k trains on graph k % len(graphs) with its own model, optimizer and split."""
    from acm_gnn_amd import GCN, FusedAdam
    out = []
    for k in range(n_runs):
        xs, ops, y = graphs[k % len(graphs)]
        n = xs.shape[0]
        torch.manual_seed(k)
        model = GCN(xs.shape[1], 64, 3, 2, n, 0.0, "acmgcn", 0)
        idx = torch.randperm(n, generator=torch.Generator().manual_seed(k))
        out.append((model, FusedAdam(model.parameters(), lr=0.1), xs, ops, y, idx[:40], idx[40:65], idx[65:]))
    return out


def _fit_each(T, runs, **kw):
    return [T.fit(m, o, x, a, y, tr, va, te, EPOCHS, use_graph=True, **kw) for m, o, x, a, y, tr, va, te in runs]


@pytest.mark.parametrize("rule,es", [("min_val_loss", 3), ("max_val_acc", 0)])
def test_fit_batched_graphs_equals_fit_run_by_run_on_the_double(monkeypatch, rule, es):
    """5 runs on 3 graphs of 90 rows in 2 slots: every slot passes from one graph to another at least once."""
    fake = install_graphs(install_batch(_install(monkeypatch)))
    from acm_gnn_amd import train as T
    graphs = [_graph(g) for g in range(3)]
    want = _fit_each(T, _runs(graphs, 5), rule=rule, early_stopping=es, sync_every=4)
    fake.small_batch_calls = 0
    got = T.fit_batched_graphs(_runs(graphs, 5), EPOCHS, rule=rule, early_stopping=es, batch=2, sync_every=4)
    assert T.fit_batched_graphs.last_refusal is None and fake.small_graphs_calls > 0 and fake.small_batch_calls == 0
    for k in range(5):
        assert same_floats(got[k][0], want[k][0]) and same_floats(got[k][1], want[k][1]), k
    assert len(fake.small_graphs_handles) >= 3, "the slots never stood on three different operators"
    # the schedule restated: slots are handed over (5 runs on 2 slots), and consecutive runs are on different graphs
    looks = _looks([len(h) for _, h in want], 2, 4, EPOCHS)
    assert sum(len(leaving) for leaving, _ in looks) == 5 and len(looks) >= 3
    if es:
        assert any(len(h) < EPOCHS for _, h in want), "no run stops early: the hand-over at different epochs is not exercised"


def test_a_run_on_a_graph_of_another_row_count_falls_back_and_says_why(monkeypatch):
    fake = install_graphs(install_batch(_install(monkeypatch)))
    from acm_gnn_amd import train as T
    graphs = [_graph(0), _graph(1), _graph(2), _graph(3, n=80)]

    def runs():
        return _runs(graphs, 4)

    want = _fit_each(T, runs(), rule="min_val_loss", early_stopping=3, sync_every=4)
    got = T.fit_batched_graphs(runs(), EPOCHS, rule="min_val_loss", early_stopping=3, batch=2, sync_every=4)
    why = T.fit_batched_graphs.last_refusal
    assert "run 3" in why and "80 rows" in why and "90" in why and getattr(fake, "small_graphs_calls", 0) == 0
    for k in range(4):
        assert same_floats(got[k][0], want[k][0]) and same_floats(got[k][1], want[k][1]), k
    # another input width, another class count
    wide = [_graph(0), _graph(1, f_in=60)]
    T.fit_batched_graphs(_runs(wide, 2), 2, batch=2, sync_every=4)
    assert "run 1" in T.fit_batched_graphs.last_refusal and "input features" in T.fit_batched_graphs.last_refusal
    T.fit_batched_graphs(_runs(graphs[:2], 2), 2, batch=2, sync_every=4)
    assert T.fit_batched_graphs.last_refusal is None                   # the reason does not outlive the call it was about
    with pytest.raises(ValueError, match="batch"):
        T.fit_batched_graphs(_runs(graphs[:1], 1), 4, batch=33)
    with pytest.raises(ValueError, match="sync_every"):
        T.fit_batched_graphs(_runs(graphs[:1], 1), 4, sync_every=0)
    assert T.fit_batched_graphs([], 4) == []


def test_graph_batch_says_why_plans_cannot_share_launches_and_keeps_its_envelope(monkeypatch):
    install_graphs(install_batch(_install(monkeypatch)))
    from acm_gnn_amd import GCN, FusedAdam, train as T
    from acm_gnn_amd.small import SmallBatch, SmallGraphBatch, SmallPlan
    graphs = [_graph(0), _graph(2), _graph(3, n=80), _graph(1, f_in=60)]

    def plan(g, model=None, train=True):
        xs, ops, y = graphs[g]
        n = xs.shape[0]
        torch.manual_seed(g)
        model = model or GCN(xs.shape[1], 64, 3, 2, n, 0.0, "acmgcn", 0)
        if not train:
            return SmallPlan(model, xs, ops)
        return SmallPlan(model, xs, ops, y, T.row_weights(torch.arange(40), n), FusedAdam(model.parameters(), lr=0.1))

    base, other = plan(0), plan(1)
    assert SmallGraphBatch.why_not([base, other]) is None
    assert "feature" in SmallBatch.why_not([base, other])              # the one-graph class still refuses them
    assert "80 and 90 rows" in SmallGraphBatch.why_not([base, plan(2)])
    assert "input features" in SmallGraphBatch.why_not([base, plan(3)])
    assert "classes" in SmallGraphBatch.why_not([base, plan(1, GCN(50, 64, 4, 2, 90, 0.0, "acmgcn", 0))])
    assert "configured" in SmallGraphBatch.why_not([base, plan(1, GCN(50, 64, 3, 2, 90, 0.0, "acmgcn", 0, variant=True))])
    assert "training and evaluation" in SmallGraphBatch.why_not([base, plan(1, train=False)])
    assert "slots" in SmallGraphBatch.why_not([base] * 33)
    with pytest.raises(ValueError, match="rows"):
        SmallGraphBatch([base, plan(2)])
    # an envelope formed from the sparser graph alone: the denser one's plan is refused with the library's message and the
    # slot keeps the run it had
    narrow = SmallGraphBatch([base], n_slots=2)
    narrow.run()
    with pytest.raises(RuntimeError, match="workgroups"):
        narrow.set_slot(1, other)
    assert narrow.plans == [base, None]
    narrow.run()
    both = SmallGraphBatch([base], n_slots=2, handles=[SmallGraphBatch.handles_of(*graphs[1][:2], True)])
    both.set_slot(1, other)
    both.run()
    assert both.plans == [base, other]
