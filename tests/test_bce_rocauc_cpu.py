"""The second protocol (BCE-with-logits + ROC-AUC, ABI 29) without a GPU: the new entry points fail loudly, the workspace
queries answer, and the numpy expectation the GPU tests use is sklearn's ``roc_auc_score`` and the reference's recorded values."""
import ctypes as C
import math
import os

import numpy as np
import pytest
import torch

import rocauc_ref as R
from conftest import GOLDEN

EINVAL, ESHAPE, EUNSUPPORTED = 1, 2, 4
CASES = ("grid", "fivelevels", "c3", "unlabeled")


def _golden():
    with np.load(os.path.join(GOLDEN, "rocauc_cases.npz")) as f:
        return {k: f[k] for k in f.files}


def test_new_entry_points_fail_loudly_without_a_gpu():
    from acm_gnn_amd import _lib
    lib = _lib.load()
    assert lib.acm_version() == 29 == _lib.ABI_VERSION
    buf = (C.c_double * 64)()                              # a real host address: argument checks come before any launch
    p = C.cast(buf, C.c_void_p)
    assert lib.acm_bce_loss(4, 2, None, 2, None, None, None, None, 2, None, 0, None, None) == EINVAL
    assert b"acm_bce_loss" in lib.acm_last_error()
    assert lib.acm_bce_loss(4, 65, p, 65, p, p, p, p, 65, p, 512, None, None) == EUNSUPPORTED
    assert lib.acm_bce_loss(4, 2, p, 1, p, p, p, None, 0, p, 512, None, None) == ESHAPE          # ld_logits < C
    assert lib.acm_rocauc_scores(4, 2, None, 2, None, None) == EINVAL
    assert lib.acm_rocauc_scores(4, 65, p, 65, p, None) == EUNSUPPORTED
    assert lib.acm_rocauc_scores(4, 1, p, 1, p, None) == ESHAPE                                   # no column 1
    assert lib.acm_rocauc(4, None, None, None, None, 4, 3, None, None, None, 0, None) == EINVAL
    assert lib.acm_rocauc(4, p, p, p, p, 4, 9, p, p, p, 512, None) == ESHAPE
    assert b"9 index sets" in lib.acm_last_error()
    assert lib.acm_rocauc(4, p, p, p, p, 3, 3, p, p, p, 512, None) == ESHAPE                      # ld_weights < n
    assert lib.acm_rocauc(4, p, p, p, p, 4, 3, p, p, p, 8, None) == 5                             # ACM_ENOMEM
    nbytes = C.c_size_t()
    assert lib.acm_rocauc_workspace_bytes(10, 9, C.byref(nbytes)) == ESHAPE
    assert lib.acm_rocauc_workspace_bytes(10, 3, None) == EINVAL
    assert lib.acm_bce_loss_workspace_bytes(10, None) == EINVAL
    assert lib.acm_bce_loss_workspace_bytes(-1, C.byref(nbytes)) == ESHAPE


def test_workspace_queries_grow_with_the_row_count():
    from acm_gnn_amd import _lib
    lib = _lib.load()
    for query, extra in (("acm_bce_loss_workspace_bytes", ()), ("acm_rocauc_workspace_bytes", (1,)),
                         ("acm_rocauc_workspace_bytes", (8,))):
        sizes = []
        for n in (0, 1, 262_145):
            nbytes = C.c_size_t()
            assert getattr(lib, query)(n, *extra, C.byref(nbytes)) == 0
            sizes.append(nbytes.value)
        assert 0 < sizes[0] <= sizes[1] <= sizes[2] and sizes[2] > sizes[0], (query, sizes)
    a, b = C.c_size_t(), C.c_size_t()
    lib.acm_rocauc_workspace_bytes(262_145, 1, C.byref(a))
    lib.acm_rocauc_workspace_bytes(262_145, 8, C.byref(b))
    assert b.value > a.value >= 262_146 * 6                 # flags (2 B) + one set's prefix counts (4 B) per position


def test_numpy_auc_is_the_reference_and_sklearn_on_the_golden_inputs():
    g = _golden()
    for tag in CASES:
        scores = R.cpu_scores(g[f"{tag}:logits"])
        y = g[f"{tag}:labels"]
        for k in range(3):
            idx = g[f"{tag}:set{k}"]
            t = R.triple(scores, y, idx)
            assert tuple(g[f"{tag}:triples"][k]) == t
            assert abs(R.auc_of(t) - g[f"{tag}:reference"][k]) <= 1e-12
            assert abs(R.midrank_auc(y[idx], scores[idx]) - g[f"{tag}:reference"][k]) <= 1e-12
    sk = pytest.importorskip("sklearn.metrics")
    for tag in CASES:
        scores, y = R.cpu_scores(g[f"{tag}:logits"]), g[f"{tag}:labels"]
        for k in range(3):
            idx = g[f"{tag}:set{k}"]
            assert abs(R.midrank_auc(y[idx], scores[idx]) - sk.roc_auc_score(y[idx], scores[idx])) <= 1e-12


def test_grid_scores_tie_where_the_differences_tie():
    """What makes the exact GPU cases exact: on the grid the fp32 softmax score depends on z_1 - z_0 alone, neighbours are far
    apart, and a difference of +20 or more scores exactly 1."""
    z = R.grid_logits(5000, 0)
    s = R.cpu_scores(z)
    d = (z[:, 1] - z[:, 0]).astype(np.float64)
    for v in np.unique(d):
        assert np.unique(s[d == v]).size == 1
    levels = np.sort(np.unique(s[np.abs(d) <= 8]))
    assert np.diff(levels).min() >= 7e-5
    assert (s[d >= 20] == 1.0).all() and np.unique(s[d <= -20]).size == 4


def test_selection_passes_over_an_undefined_metric():
    from acm_gnn_amd import train as T
    assert T._selection_key("max_val_acc", float("nan"), 0.3) is None
    assert T._selection_key("max_val_acc", 0.25, float("nan")) == 0.25
    assert T._selection_key("min_val_loss", 0.25, 0.5) == -0.5
    with pytest.raises(ValueError, match="criterion"):
        T._checked("mse", T.CRITERIA, "criterion")
    assert math.isnan(R.auc_of((0, 0, 5)))


def test_public_entry_points_validate_their_operands(monkeypatch):
    import fake_lib
    fake_lib.install(monkeypatch)                            # (the device seams accept CPU tensors; nothing below launches)
    from acm_gnn_amd import functional as AF
    z, y, w = torch.zeros(6, 2), torch.zeros(6, dtype=torch.int64), torch.ones(3, 6)
    for bad in (dict(logits=z.double()), dict(logits=torch.zeros(2, 6).t()), dict(labels=y.int()), dict(labels=y[:5]),
                dict(labels=torch.zeros(12, dtype=torch.int64)[::2]), dict(weights=w.double()), dict(weights=w[:, :5]),
                dict(weights=torch.ones(6, 3).t()), dict(weights=torch.ones(9, 6)), dict(logits=torch.zeros(6, 1)),
                dict(logits=torch.zeros(6, 65))):
        args = dict(logits=z, labels=y, weights=w)
        args.update(bad)
        with pytest.raises(ValueError, match="eval_rocauc"):
            AF.eval_rocauc(args["logits"], args["labels"], args["weights"])
    for fn in (AF.bce_loss, AF.bce_loss_and_grad, AF.masked_bce):
        with pytest.raises(ValueError):
            fn(z, y.int(), w[0])
        with pytest.raises(ValueError):
            fn(z.double(), y, w[0])
        with pytest.raises(ValueError):
            fn(z, y, w[0].double())
        with pytest.raises(ValueError):
            fn(z, y, torch.ones(5))
