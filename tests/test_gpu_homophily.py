"""The homophily measures on the GPU (acm_homophily.hip): the census equals the numpy census bit for bit, is deterministic,
capturable and additive over row slices; the four measures match the values recorded from the reference; aggregation homophily
agrees row by row with float64 wherever float64 itself is decided; the class means are accurate and run-to-run identical."""
import os

import numpy as np
import pytest
import torch

import homophily_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

TOL = 5e-7                                   # the reference returns fp32
LABELED = ("hub", "c3f7", "c10")
DEV = "cuda"


@pytest.fixture(scope="module")
def G():
    with np.load(os.path.join(GOLDEN, "homophily_cases.npz")) as f:
        return {k: f[k] for k in f.files}


def _t(a, dtype=None):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dtype is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dtype)


def _pattern(ip, ix, n_cols, chunk=0):
    from acm_gnn_amd import CsrGraph
    return CsrGraph.from_csr(_t(ip), _t(ix), None, n_cols, chunk)


def _valued(ip, ix, vals, n_cols):
    from acm_gnn_amd import CsrGraph
    return CsrGraph.from_csr(_t(ip), _t(ix), _t(vals), n_cols)


def _case(G, tag):
    y = G[f"{tag}:labels"]
    n, c = len(y), int(G[f"{tag}:n_classes"])
    ip, ix = R.csr_of_edges(G[f"{tag}:edges"], n)
    return n, c, ip, ix, y


def _random_graph(n, c, seed, deg=10, unlabeled=0):
    rng = np.random.default_rng(seed)
    src = np.repeat(np.arange(n), deg)
    dst = rng.integers(0, n, n * deg)
    e = np.unique(np.concatenate([np.stack([src, dst], 1), np.stack([dst, src], 1)]), axis=0).astype(np.int32)
    y = rng.integers(0, c, n).astype(np.int64)
    y[:c] = np.arange(c)
    if unlabeled:
        idx = rng.choice(np.arange(c, n), unlabeled, replace=False)
        y[idx[: unlabeled // 2]] = -1
        y[idx[unlabeled // 2:]] = c + 3                       # beyond the class count: unlabeled too, never an index
    return e, y


def _assert_census(res, want):
    torch.cuda.synchronize()
    assert res.counts.cpu().numpy().tolist() == R.counts_vector(want).tolist()
    assert np.array_equal(res.row_same.cpu().numpy(), want["row_same"])
    assert np.array_equal(res.row_deg.cpu().numpy(), want["row_deg"])
    got = float(res.node_sum.cpu()[0])
    assert abs(got - want["node_sum"]) <= 1e-12 * max(1.0, want["node_sum"])        # (float64, another order)


# ---- census ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", LABELED + ("unlabeled", "hand"))
def test_census_is_exact_on_the_golden_graphs(G, tag):
    from acm_gnn_amd import FilterOperators
    from acm_gnn_amd import homophily as H
    n, c, ip, ix, y = _case(G, tag)
    want = R.census(ip, ix, y, c)
    _assert_census(H.census(_pattern(ip, ix, n), _t(y), c), want)
    # the normalised operator D^-1 (A + I) has the same off-diagonal pattern: the same census through FilterOperators
    low = _valued(G[f"{tag}:norm_indptr"], G[f"{tag}:norm_indices"], G[f"{tag}:norm_vals"], n)
    _assert_census(H.census(FilterOperators(low), _t(y), c), want)


def test_census_is_exact_on_one_node_many_classes_and_a_split_hub(G):
    from acm_gnn_amd import homophily as H
    one = H.census(_pattern(np.zeros(2, np.int32), np.zeros(0, np.int32), 1), _t(np.zeros(1, np.int64)), 2)
    _assert_census(one, R.census(np.zeros(2, np.int32), np.zeros(0, np.int32), np.zeros(1, np.int64), 2))
    assert one.counts.cpu().tolist() == [0, 0, 0, 0, 1, 0, 1, 0, 1, 0]                  # cls[0] = iso[0] = n_labeled = 1
    e, y = _random_graph(4099, 64, 5, unlabeled=200)
    ip, ix = R.csr_of_edges(e, 4099)
    _assert_census(H.census(_pattern(ip, ix, 4099), _t(y), 64), R.census(ip, ix, y, 64))
    n, c, ip, ix, y = _case(G, "hub")
    hub = _pattern(ip, ix, n, chunk=128)
    assert hub.n_long_rows > 0                                                         # the 500-neighbour row is split into pieces
    _assert_census(H.census(hub, _t(y), c), R.census(ip, ix, y, c))


def test_census_is_deterministic_and_capturable(G):
    from acm_gnn_amd import homophily as H
    n, c, ip, ix, y = _case(G, "hub")
    graph, yt = _pattern(ip, ix, n, chunk=128), _t(y)
    buf = H.census_buffers(graph, c)
    H.census(graph, yt, c, out=buf)
    torch.cuda.synchronize()
    first = (buf._buf.clone(), buf.row_same.clone(), buf.row_deg.clone())
    H.census(graph, yt, c, out=buf)
    torch.cuda.synchronize()
    assert torch.equal(buf._buf, first[0]) and torch.equal(buf.row_same, first[1]) and torch.equal(buf.row_deg, first[2])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        H.census(graph, yt, c, out=buf)
    torch.cuda.current_stream().wait_stream(side)
    cg = torch.cuda.CUDAGraph()
    with torch.cuda.graph(cg):
        H.census(graph, yt, c, out=buf)
    for _ in range(2):
        buf._buf.fill_(-7), buf.row_same.fill_(-7), buf.row_deg.fill_(-7)
        cg.replay()
        torch.cuda.synchronize()
        assert torch.equal(buf._buf, first[0]) and torch.equal(buf.row_same, first[1]) and torch.equal(buf.row_deg, first[2])


def test_census_of_row_slices_adds_up(G):
    from acm_gnn_amd import homophily as H
    n, c, ip, ix, y = _case(G, "c10")
    graph, yt = _pattern(ip, ix, n), _t(y)
    whole = H.census(graph, yt, c)
    h = 517
    a = H.census(graph.slice_rows(0, h), yt, c, row_offset=0)
    b = H.census(graph.slice_rows(h, n), yt, c, row_offset=h)
    torch.cuda.synchronize()
    assert torch.equal(a.counts + b.counts, whole.counts)
    assert torch.equal(torch.cat([a.row_same, b.row_same]), whole.row_same)
    assert torch.equal(torch.cat([a.row_deg, b.row_deg]), whole.row_deg)


@pytest.mark.parametrize("tag", LABELED + ("unlabeled", "hand"))
def test_measures_match_the_reference(G, tag):
    from acm_gnn_amd import homophily as H
    n, c, ip, ix, y = _case(G, tag)
    res = H.census(_pattern(ip, ix, n), _t(y), c)
    assert abs(res.klass - G[f"{tag}:ref_class"]) <= TOL
    if tag not in LABELED:
        return
    assert abs(res.edge - G[f"{tag}:ref_edge"]) <= TOL
    assert abs(res.node - G[f"{tag}:ref_node"]) <= TOL
    assert np.abs(res.compat - G[f"{tag}:ref_compat"]).max() <= TOL
    # the reference's names and argument order, on the tensors its callers hold: a sparse adjacency and one-hot labels
    e = G[f"{tag}:edges"].astype(np.int64)
    adj = torch.sparse_coo_tensor(_t(e.T.copy()), torch.ones(len(e), device=DEV), (n, n))
    onehot = _t(R.one_hot(y, c))
    assert abs(H.edge_homophily(adj, onehot) - G[f"{tag}:ref_edge"]) <= TOL
    assert abs(H.node_homophily(adj, _t(y)) - G[f"{tag}:ref_node"]) <= TOL
    assert np.abs(H.compat_matrix(adj, _t(y)) - G[f"{tag}:ref_compat"]).max() <= TOL
    assert abs(H.class_homophily(adj, _t(y)) - G[f"{tag}:ref_class"]) <= TOL


# ---- aggregation homophily ----------------------------------------------------------------------------------------------------
def _signal_features(y, c, f, seed):
    rng = np.random.default_rng(seed)
    centers = rng.normal(size=(c, f))
    return (centers[np.maximum(y, 0)] * (y >= 0)[:, None] + 1.5 * rng.normal(size=(len(y), f))).astype(np.float32)


def _agg_operands(G, case):
    """(n, C, labels, features or None, (indptr, indices, vals) of D^-1 (A + I), recorded reference value or None)"""
    if case == "c64f64":
        e, y = _random_graph(4099, 64, 9)
        return 4099, 64, y, _signal_features(y, 64, 64, 19), R.normalised_operator(e, 4099), None
    tag, feats, ref = {"hub_onehot": ("hub", None, "ref_agg_onehot"), "hub_f12": ("hub", "golden", "ref_agg"),
                       "hub_f12_implicit": ("hub", "golden", "ref_agg"), "c10_onehot": ("c10", None, "ref_agg_onehot"),
                       "c3f7": ("c3f7", "golden", "ref_agg"), "f200": ("c3f7", 200, None), "f300_gemm": ("c3f7", 300, None),
                       "unlabeled": ("unlabeled", "golden", None)}[case]
    y = G[f"{tag}:labels"]
    n, c = len(y), int(G[f"{tag}:n_classes"])
    x = None if feats is None else (G[f"{tag}:features"] if feats == "golden" else _signal_features(y, c, feats, feats))
    op = (G[f"{tag}:norm_indptr"], G[f"{tag}:norm_indices"], G[f"{tag}:norm_vals"])
    return n, c, y, x, op, (float(G[f"{tag}:{ref}"]) if ref else None)


@pytest.mark.parametrize("case", ["hub_onehot", "hub_f12", "hub_f12_implicit", "c10_onehot", "c3f7", "c64f64", "f200", "f300_gemm",
                                  "unlabeled"])
def test_aggregation_homophily_agrees_with_float64_row_by_row(G, case):
    """A row may be left out only where float64 itself is undecided: (top1 - top2) / max|W| < tau = 4 (d_max + F + 2) 2^-24, four
    times the worst-case fp32 sequential-sum bound of the gather, the dot product and the mean; at most 2 % of the rows."""
    from acm_gnn_amd import FilterOperators
    from acm_gnn_amd import homophily as H
    n, c, y, x, (ip, ix, vals), ref = _agg_operands(G, case)
    if case == "hub_f12_implicit":                             # pattern + row scale: every stored entry of a row is 1 / d_i
        assert np.array_equal(vals, np.repeat(vals[ip[:-1]], np.diff(ip)))
        adj = FilterOperators(_pattern(ip, ix, n), row_scale=_t(vals[ip[:-1]]))
    else:
        adj = _valued(ip, ix, vals, n)
    x_np = R.one_hot(y, c) if x is None else x
    f = x_np.shape[1]
    value, rows = H.aggregation_homophily(None if x is None else _t(x), adj, _t(y), return_rows=True)
    rows = rows.cpu().numpy().astype(bool)
    hits, margins = R.agg_rows(R.dense_times(ip, ix, vals, x_np), y, c)
    labeled = (y >= 0) & (y < c)
    tau = 4.0 * (int(np.diff(ip).max()) + f + 2) * 2.0 ** -24
    left = labeled & (margins < tau)
    print(f"{case}: n={n} C={c} F={f} tau={tau:.3e} left_out={int(left.sum())} disagree={int((rows != hits)[labeled].sum())} "
          f"value={value:.7f} float64={hits.sum() / labeled.sum():.7f} reference={ref}")
    assert left.sum() <= 0.02 * n
    keep = labeled & ~left
    assert np.array_equal(rows[keep], hits[keep])
    assert not rows[~labeled].any()                            # unlabeled rows are not scored
    assert value == int(rows.sum()) / int(labeled.sum())
    if ref is not None:
        # the reference returns matches.float().mean(): k / n rounded once to fp32; ours is rounded the same way before comparing
        assert abs(float(np.float32(rows.sum()) / np.float32(labeled.sum())) - ref) <= left.sum() / n


@pytest.mark.parametrize("n,c,f,ld", [(1500, 5, 12, 12), (4099, 64, 70, 96), (130, 2, 1, 1)])
def test_class_means_are_accurate_and_bit_identical(n, c, f, ld):
    from acm_gnn_amd import homophily as H
    rng = np.random.default_rng(n + f)
    y = rng.integers(-1, c, n).astype(np.int64)                # some rows unlabeled
    y[:c] = np.arange(c)
    z = (rng.normal(size=(n, f)) + 0.5).astype(np.float32)
    wide = torch.zeros(n, ld, device=DEV)
    wide[:, :f] = _t(z)
    zt, yt = wide[:, :f], _t(y)
    mu, count = H.class_means(zt, yt, c)
    mu2, count2 = H.class_means(zt, yt, c)
    torch.cuda.synchronize()
    want, want_count = R.class_means(z.astype(np.float64), y, c)
    assert count.cpu().numpy().tolist() == want_count.tolist()
    err = np.abs(mu.cpu().numpy().astype(np.float64) - want).max()
    print(f"class means n={n} C={c} F={f}: max error {err:.3e}, bound {1e-6 * np.abs(z).max():.3e}")
    assert err <= 1e-6 * np.abs(z).max()
    assert torch.equal(mu, mu2) and torch.equal(count, count2)


def test_a_class_without_a_member_is_never_chosen():
    from acm_gnn_amd import homophily as H
    z = torch.tensor([[1.0, 0.0], [0.9, 0.1], [0.0, 1.0], [0.1, 0.9]], device=DEV)
    y = torch.tensor([0, 0, 2, 2], device=DEV)                 # class 1 is empty: mu_1 = 0, its score would tie or win at 0
    mu, count = H.class_means(z, y, 3)
    assert count.cpu().tolist() == [2, 0, 2] and mu[1].abs().sum().item() == 0.0
    counts, rows = H.class_score(z, mu, count, y, return_rows=True)
    assert counts.cpu().tolist() == [4, 4] and rows.cpu().tolist() == [1, 1, 1, 1]
    # every real score negative, the empty class's 0: unmasked, class 1 would win every row
    neg = torch.tensor([[-0.1, -1.0], [0.0, 0.0], [-1.0, -0.1]], device=DEV)
    counts, rows = H.class_score(z, neg, count, y, return_rows=True)
    assert counts.cpu().tolist() == [4, 4] and rows.cpu().tolist() == [1, 1, 1, 1]
    counts = H.class_score(z, neg, torch.tensor([2, 1, 2], device=DEV), y)
    assert counts.cpu().tolist() == [0, 4]
