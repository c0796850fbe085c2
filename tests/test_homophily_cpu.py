"""The homophily measures without a GPU: the numpy restatement and ``HomophilyCensus.from_counts`` reproduce the values recorded
from the reference's ``synthetic-experiments/homophily.py`` (tests/golden/make_homophily_golden.py), the new entry points fail
loudly with their status codes, the workspace queries answer, and the wrappers reject what they cannot take."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import homophily_ref as R
from conftest import GOLDEN

EINVAL, ESHAPE, EUNSUPPORTED, ENOMEM = 1, 2, 4, 5
TOL = 5e-7                                   # the reference returns fp32 (its worst difference on these graphs: 2.2e-8)
LABELED = ("hub", "c3f7", "c10")
CASES = LABELED + ("unlabeled", "hand")


def _golden():
    with np.load(os.path.join(GOLDEN, "homophily_cases.npz")) as f:
        return {k: f[k] for k in f.files}


def _census(g, tag):
    n, c = len(g[f"{tag}:labels"]), int(g[f"{tag}:n_classes"])
    ip, ix = R.csr_of_edges(g[f"{tag}:edges"], n)
    return R.census(ip, ix, g[f"{tag}:labels"], c)


def _from_counts(cs):
    from acm_gnn_amd.homophily import HomophilyCensus
    return HomophilyCensus.from_counts(cs["M"], cs["cls"], cs["iso"], cs["n_labeled"], cs["n_deg"], cs["node_sum"])


def test_restatement_and_from_counts_reproduce_the_reference():
    g = _golden()
    for tag in CASES:
        cs = _census(g, tag)
        hc = _from_counts(cs)
        assert abs(R.klass(cs) - g[f"{tag}:ref_class"]) <= TOL and abs(hc.klass - g[f"{tag}:ref_class"]) <= TOL, tag
        if tag not in LABELED:
            continue
        assert abs(R.edge(cs) - g[f"{tag}:ref_edge"]) <= TOL and abs(hc.edge - g[f"{tag}:ref_edge"]) <= TOL, tag
        assert abs(R.node(cs) - g[f"{tag}:ref_node"]) <= TOL and abs(hc.node - g[f"{tag}:ref_node"]) <= TOL, tag
        assert np.abs(R.compat(cs) - g[f"{tag}:ref_compat"]).max() <= TOL, tag
        assert np.abs(hc.compat - g[f"{tag}:ref_compat"]).max() <= TOL, tag
        n = len(g[f"{tag}:labels"])
        op = (g[f"{tag}:norm_indptr"], g[f"{tag}:norm_indices"], g[f"{tag}:norm_vals"])
        for key, x in (("ref_agg", g[f"{tag}:features"]), ("ref_agg_onehot", R.one_hot(g[f"{tag}:labels"], int(g[f"{tag}:n_classes"])))):
            hits, margins = R.agg_rows(R.dense_times(*op, x), g[f"{tag}:labels"], int(g[f"{tag}:n_classes"]))
            close = int((margins < 1e-4).sum())
            mean32 = float(np.float32(hits.sum()) / np.float32(n))          # the reference returns k / n rounded once to fp32
            assert close <= 7 and abs(mean32 - g[f"{tag}:{key}"]) <= close / n, (tag, key, close)


def test_hand_made_graph_counts_by_hand():
    """Triangle 0-1-2 with a raw self-loop on 1, node 3 isolated, node 4 unlabeled and tied to 0; labels 0 0 1 2 -1."""
    g = _golden()
    cs = _census(g, "hand")
    assert cs["M"].tolist() == [[2, 2, 0], [2, 0, 0], [0, 0, 0]]            # (1, 1) and both (0, 4) entries do not count
    assert cs["cls"].tolist() == [2, 1, 1] and cs["iso"].tolist() == [0, 0, 1]
    assert (cs["n_labeled"], cs["n_deg"]) == (4, 3)
    assert cs["row_same"].tolist() == [1, 1, 0, 0, 0] and cs["row_deg"].tolist() == [2, 2, 2, 0, 0]
    hc = _from_counts(cs)
    assert hc.edge == 2 / 6 and hc.node == (0.5 + 0.5 + 0.0) / 3 and hc.klass == 0.375
    assert np.isnan(hc.compat[2]).all() and hc.compat[0].tolist() == [0.5, 0.5, 0.0]
    # a row slice counts on its own and the slices add up
    n, c, y = 5, 3, g["hand:labels"]
    ip, ix = R.csr_of_edges(g["hand:edges"], n)
    a = R.census(ip[:3], ix[:ip[2]], y, c)
    b = R.census(ip[2:] - ip[2], ix[ip[2]:], y, c, row_offset=2)
    assert (R.counts_vector(a) + R.counts_vector(b)).tolist() == R.counts_vector(cs).tolist()
    assert np.concatenate([a["row_deg"], b["row_deg"]]).tolist() == cs["row_deg"].tolist()
    with pytest.raises(ValueError):
        from acm_gnn_amd.homophily import HomophilyCensus
        HomophilyCensus.from_counts(np.zeros((2, 3)), [0, 0], [0, 0], 0, 0, 0.0)


def test_new_entry_points_fail_loudly_without_a_gpu():
    from acm_gnn_amd import _lib
    lib = _lib.load()
    assert lib.acm_version() == 29 == _lib.ABI_VERSION                    # added symbols: the ABI number stays
    buf = (C.c_double * 64)()                                             # a real host address: argument checks come before any launch
    p = C.cast(buf, C.c_void_p)
    assert lib.acm_homophily_census(None, None, 0, 5, None, None, None, None, None, 0, None) == EINVAL
    assert b"acm_homophily_census" in lib.acm_last_error()
    assert lib.acm_homophily_census(None, p, 0, 1, p, p, None, None, p, 512, None) == ESHAPE
    assert lib.acm_homophily_census(None, p, 0, 65, p, p, None, None, p, 512, None) == EUNSUPPORTED
    assert b"65 classes" in lib.acm_last_error()
    assert lib.acm_class_means(4, 3, 2, None, 3, None, None, 3, None, None, 0, None) == EINVAL
    assert b"acm_class_means" in lib.acm_last_error()
    assert lib.acm_class_means(4, 3, 1, p, 3, p, p, 3, p, p, 512, None) == ESHAPE
    assert lib.acm_class_means(4, 3, 65, p, 3, p, p, 3, p, p, 512, None) == EUNSUPPORTED
    assert lib.acm_class_means(4, 3, 2, p, 2, p, p, 3, p, p, 512, None) == ESHAPE           # ld_z < F
    assert lib.acm_class_means(4, 3, 2, p, 3, p, p, 2, p, p, 512, None) == ESHAPE           # ld_mu < F
    assert lib.acm_class_means(4, 3, 2, p, 3, p, p, 3, p, p, 8, None) == ENOMEM
    assert b"workspace 8 B" in lib.acm_last_error()
    assert lib.acm_class_means(4, 3, 2, p, 3, p, p, 3, p, None, 0, None) == ENOMEM
    assert lib.acm_class_score(4, 3, 2, None, 3, None, 3, None, None, None, None, None) == EINVAL
    assert b"acm_class_score" in lib.acm_last_error()
    assert lib.acm_class_score(4, 3, 1, p, 3, p, 3, p, p, None, p, None) == ESHAPE
    assert lib.acm_class_score(4, 3, 65, p, 3, p, 3, p, p, None, p, None) == EUNSUPPORTED
    assert lib.acm_class_score(4, 257, 2, p, 257, p, 257, p, p, None, p, None) == EUNSUPPORTED
    assert b"257 features" in lib.acm_last_error()
    assert lib.acm_class_score(4, 3, 2, p, 2, p, 3, p, p, None, p, None) == ESHAPE          # ld_z < F
    nbytes = C.c_size_t()
    assert lib.acm_homophily_workspace_bytes(10, 10, 5, None) == EINVAL
    assert lib.acm_homophily_workspace_bytes(10, 10, 1, C.byref(nbytes)) == ESHAPE
    assert lib.acm_homophily_workspace_bytes(10, 10, 65, C.byref(nbytes)) == EUNSUPPORTED
    assert lib.acm_class_means_workspace_bytes(10, 4, 5, None) == EINVAL
    assert lib.acm_class_means_workspace_bytes(10, 0, 5, C.byref(nbytes)) == ESHAPE
    assert lib.acm_class_means_workspace_bytes(10, 4, 65, C.byref(nbytes)) == EUNSUPPORTED


def test_workspace_queries_grow_with_the_node_count():
    from acm_gnn_amd import _lib
    lib = _lib.load()
    for query, args in (("acm_homophily_workspace_bytes", lambda n: (n, n, 5)), ("acm_homophily_workspace_bytes", lambda n: (n, n, 64)),
                        ("acm_class_means_workspace_bytes", lambda n: (n, 7, 3)), ("acm_class_means_workspace_bytes", lambda n: (n, 300, 64))):
        sizes = []
        for n in (0, 1, 1500, 1_632_803):
            nbytes = C.c_size_t()
            assert getattr(lib, query)(*args(n), C.byref(nbytes)) == 0
            sizes.append(nbytes.value)
        assert 0 < sizes[0] <= sizes[1] < sizes[2] < sizes[3], (query, sizes)
    a, b = C.c_size_t(), C.c_size_t()
    lib.acm_homophily_workspace_bytes(168_114, 168_114, 2, C.byref(a))
    assert 13 * 168_114 <= a.value < 14 * 168_114              # one label byte per column and three int32 counters per row
    lib.acm_class_means_workspace_bytes(1_632_803, 64, 64, C.byref(b))
    assert b.value <= 2048 * 64 * 65 * 4 + 64                  # at most 2048 tiles of partial sums, whatever the row count


class _Pattern:
    n_rows = n_cols = 6
    device = torch.device("cpu")


def test_wrappers_reject_bad_operands():
    from acm_gnn_amd import FilterOperators
    from acm_gnn_amd import homophily as H
    y = torch.zeros(6, dtype=torch.int64)
    y[3:] = 1
    sharded = FilterOperators(_Pattern(), group=object())
    for fn in (H.census, H.edge_homophily, H.node_homophily, H.compat_matrix, H.class_homophily):
        with pytest.raises(NotImplementedError, match="row-sharded"):
            fn(sharded, y)
    with pytest.raises(NotImplementedError, match="row-sharded"):
        H.aggregation_homophily(None, sharded, y)
    plain = FilterOperators(_Pattern())
    with pytest.raises(TypeError):
        H.census([[0, 1], [1, 0]], y)
    with pytest.raises(ValueError, match="matrix"):
        H.census(torch.zeros(6), y)
    with pytest.raises(ValueError, match="int64"):
        H.census(plain, y.int())
    with pytest.raises(ValueError, match="int64"):
        H.census(plain, y.float())
    with pytest.raises(ValueError, match="classes"):
        H.census(plain, torch.zeros(6, dtype=torch.int64))                 # one class
    with pytest.raises(ValueError, match="classes"):
        H.census(plain, y, n_classes=65)
    with pytest.raises(ValueError, match="labels for an operator"):
        H.census(plain, y[:5])
    with pytest.raises(ValueError, match="labels must be"):
        H.census(plain, torch.zeros(6, 2, 2))
    with pytest.raises(ValueError, match="no columns"):
        H.census(plain, y, row_offset=1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.census(plain, y)                                                 # everything else is in order: CPU labels are refused
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        H.census(torch.eye(6), y)
    z = torch.zeros(6, 4)
    for bad in (dict(z=z.double()), dict(z=torch.zeros(4, 6).t()), dict(z=torch.zeros(6)), dict(labels=y.int()), dict(labels=y[:5]),
                dict(labels=torch.zeros(12, dtype=torch.int64)[::2]), dict(n_classes=1), dict(n_classes=65)):
        args = dict(z=z, labels=y, n_classes=2)
        args.update(bad)
        with pytest.raises(ValueError, match="class_means"):
            H.class_means(**args)
    mu, count = torch.zeros(2, 4), torch.ones(2, dtype=torch.int64)
    for bad in (dict(mu=torch.zeros(2, 3)), dict(mu=mu.double()), dict(class_count=count.int()), dict(class_count=torch.ones(3, dtype=torch.int64)),
                dict(z=torch.zeros(6, 300), mu=torch.zeros(2, 300)), dict(z=z.double())):
        args = dict(z=z, mu=mu, class_count=count, labels=y)
        args.update(bad)
        with pytest.raises(ValueError, match="class_score"):
            H.class_score(**args)
    with pytest.raises(ValueError, match="one label per node"):
        H.aggregation_homophily(z, plain, y[:5].clone())
    with pytest.raises(ValueError, match="features must be"):
        H.aggregation_homophily(torch.zeros(5, 4), plain, y)
    with pytest.raises(ValueError, match="floating point"):
        H.aggregation_homophily(torch.zeros(6, 4, dtype=torch.int64), plain, y)
    onehot = torch.nn.functional.one_hot(y, 2)
    assert H._labels_of(onehot, None, "t")[1] == 2 and H._labels_of(onehot, None, "t")[0].tolist() == y.tolist()
    assert H._labels_of(torch.zeros(3, 4), None, "t")[0].tolist() == [-1, -1, -1]          # all-zero rows are unlabeled
