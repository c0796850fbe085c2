"""The homophily measures on the GPU (acm_homophily.hip): the census equals the numpy census bit for bit, is deterministic,
capturable and additive over row slices; the four measures match the values recorded from the reference; aggregation homophily
agrees row by row with float64 wherever float64 itself is decided; the class means are accurate and run-to-run identical."""
import os

import numpy as np
import pytest
import torch

import homophily_ref as R
import launch_forms as LF
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


# ---- launch forms no small case reaches: exact integers against int64 references ---------------------------------------------
# Inputs are small integers held in fp32, so every product and partial sum is an integer below 2^24: any summation order, any
# slab assignment and the MFMA give the same bits, and the comparisons below are ``==`` with no tolerance.
EXACT = 2 ** 24


def _score_case(n, c, f, seed):
    """(z, mu, class_count, labels, want_hit, want_counts, ties) of one exact acm_class_score case.  About a quarter of the
    classes is empty, class 0 among them, and class 0's mu row is the copy of a paired (often winning) row: unmasked it would be
    the first maximum.  Rows of mu are copied at the distances 1 (within a lane), 4 (across the four lanes of a row), 16 and 32
    (across MFMA tiles).  ``ties`` counts the labeled rows whose maximum is tied, in all and per kind."""
    rng = np.random.default_rng(seed)
    z = rng.integers(-2, 3, (n, f)).astype(np.float32)
    mu = rng.integers(-2, 3, (c, f)).astype(np.float32)
    count = rng.integers(1, 9, c).astype(np.int64)
    count[rng.random(c) < 0.25] = 0
    count[0] = 0
    if not count[1:].any():
        count[c - 1] = 3
    free = count > 0
    paired = 0
    fits = {1: lambda k: k % 4 != 3, 4: lambda k: k % 16 < 12, 16: lambda k: True, 32: lambda k: True}
    for turn in range(c):
        d = (32, 16, 4, 1)[turn % 4]
        for k in range(c - d):
            if c >= 8 and free[k] and free[k + d] and fits[d](k) and paired < 0.6 * c:
                mu[k + d] = mu[k]
                free[k] = free[k + d] = False
                if paired == 0:
                    mu[0] = mu[k]                              # the empty class 0 doubles a paired row
                paired += 2
                break
    w = z.astype(np.int64) @ mu.astype(np.int64).T
    assert np.abs(z.astype(np.int64)).max(initial=0) * np.abs(mu.astype(np.int64)).max() * f < EXACT   # every partial sum
    assert np.abs(w).max(initial=0) < EXACT
    w[:, count == 0] = -EXACT
    arg = w.argmax(1)                                          # the first maximum
    y = arg.copy()
    other = rng.random(n) < 0.4
    y[other] = rng.integers(0, c, int(other.sum()))
    top = w == w.max(1, keepdims=True)
    later = np.array([np.flatnonzero(t)[-1] for t in top], np.int64) if n else arg
    swap = rng.random(n) < 0.2
    y[swap] = later[swap]                                      # a later tied class is a miss
    idx = np.arange(n)
    y[idx % 7 == 3] = -1
    y[idx % 11 == 5] = c
    y[idx % 13 == 6] = c + 3
    labeled = (y >= 0) & (y < c)
    hit = labeled & (arg == y)
    a = arg
    def also(d, ok):
        j = np.minimum(a + d, c - 1)
        return labeled & ok & (a + d < c) & top[idx, j]
    ties = dict(any=int((labeled & (top.sum(1) > 1)).sum()), lane=int(also(1, a % 4 != 3).sum()),
                row=int(also(4, a % 16 < 12).sum()), tile=int((also(16, True) | also(32, True)).sum()),
                labeled=int(labeled.sum()))
    return z, mu, count, y.astype(np.int64), hit, [int(hit.sum()), int(labeled.sum())], ties


def _z_layout(z, kind):
    """``z`` on the device as a view of a NaN-filled buffer: contiguous, row pitch F + 1, row pitch F + 4, or a base one float
    behind a 16-byte boundary with a pitch that is a multiple of 4."""
    n, f = z.shape
    if kind == "contiguous":
        return _t(z)
    ld, off = {"pitch_f1": (f + 1, 0), "pitch_f4_nan": (f + 4, 0), "base_off_4B": ((f + 3) // 4 * 4 + 4, 1)}[kind]
    buf = torch.full((off + n * ld + 3,), float("nan"), device=DEV)
    view = buf[off:off + n * ld].view(n, ld)[:, :f]
    view.copy_(_t(z))
    assert view.data_ptr() % 16 == 4 * off and view.stride(0) == ld
    return view


def _run_score(n, c, f, layout="contiguous", ties_required=None):
    from acm_gnn_amd import homophily as H
    z, mu, count, y, want_hit, want_counts, ties = _score_case(n, c, f, 1000 * c + f + n)
    if f >= 16 if ties_required is None else ties_required:
        assert ties["any"] >= 0.10 * ties["labeled"], ties     # conditions on the reference, not on the kernel
        assert ties["lane"] > 0 and ties["row"] > 0 and ties["tile"] > 0, ties
    zt = _z_layout(z, layout)
    counts, rows = H.class_score(zt, _t(mu), _t(count), _t(y), return_rows=True)
    torch.cuda.synchronize()
    assert counts.cpu().tolist() == want_counts
    assert np.array_equal(rows.cpu().numpy().astype(bool), want_hit)


@pytest.mark.parametrize("c,f", LF.SCORE_SHAPES)
def test_class_score_is_exact_on_integers(c, f):
    _run_score(1000, c, f)


@pytest.mark.parametrize("n", LF.SCORE_SMALL_N)
@pytest.mark.parametrize("c,f", [(17, 15), (49, 64)])
def test_class_score_is_exact_at_partial_row_groups(c, f, n):
    _run_score(n, c, f, ties_required=False)                   # (too few rows to demand every kind of tie)


@pytest.mark.parametrize("layout", ["contiguous", "pitch_f1", "pitch_f4_nan", "base_off_4B"])
@pytest.mark.parametrize("c,f", [(16, 4), (33, 16), (49, 64)])
def test_class_score_is_exact_on_padded_and_misaligned_rows(c, f, layout):
    _run_score(1000, c, f, layout)


@pytest.mark.parametrize("c,f,n", LF.SCORE_SECOND_TRIPS)
def test_class_score_is_exact_past_its_grid_cap(c, f, n):
    _run_score(n, c, f)


@pytest.mark.parametrize("n,f,c,pad", LF.MEANS_CASES)
def test_class_means_are_exact_on_integers(n, f, c, pad):
    from acm_gnn_amd import homophily as H
    rng = np.random.default_rng(n + f)
    y = rng.integers(-1, c, n).astype(np.int64)                # some rows unlabeled
    y[:c] = np.arange(c)
    y[-3:] = [c - 1, 0, 1]                                     # the last tile holds members
    z = rng.integers(-3, 4, (n, f)).astype(np.float32)
    want = np.zeros((c, f), np.float32)
    want_count = np.bincount(y[y >= 0], minlength=c)
    for k in range(c):
        s = z[y == k].astype(np.int64).sum(0)
        assert np.abs(z[y == k].astype(np.int64)).sum(0).max() < EXACT
        want[k] = (s.astype(np.float64) / want_count[k]).astype(np.float32)
    wide = torch.full((n, f + pad), float("nan"), device=DEV)
    wide[:, :f] = _t(z)
    mu, count = H.class_means(wide[:, :f], _t(y), c)
    torch.cuda.synchronize()
    assert count.cpu().numpy().tolist() == want_count.tolist()
    assert np.array_equal(mu.cpu().numpy().view(np.int32), want.view(np.int32))


def _symmetric_random_graph(n, c, seed, pairs, unlabeled=0, hub=0):
    """(directed edge list of a symmetric graph with ``pairs`` random pairs and ``hub`` extra neighbours of node 0, labels)"""
    rng = np.random.default_rng(seed)
    src, dst = rng.integers(0, n, pairs), rng.integers(0, n, pairs)
    if hub:
        src = np.concatenate([src, np.zeros(hub, np.int64)])
        dst = np.concatenate([dst, rng.choice(np.arange(1, n), hub, replace=False)])
    key = np.unique(np.concatenate([src * n + dst, dst * n + src]))
    e = np.stack([key // n, key % n], 1).astype(np.int32)
    y = rng.integers(0, c, n).astype(np.int64)
    y[:c] = np.arange(c)
    if unlabeled:
        idx = rng.choice(np.arange(c, n), unlabeled, replace=False)
        y[idx[: unlabeled // 2]] = -1
        y[idx[unlabeled // 2:]] = c + 3
    return e, y


def _census_twice(ip, ix, y, c, n, chunk=0):
    from acm_gnn_amd import homophily as H
    graph, yt = _pattern(ip, ix, n, chunk), _t(y)
    buf = H.census_buffers(graph, c)
    H.census(graph, yt, c, out=buf)
    _assert_census(buf, R.census(ip, ix, y, c))
    first = (buf._buf.clone(), buf.row_same.clone(), buf.row_deg.clone())
    buf._buf.fill_(-7), buf.row_same.fill_(-7), buf.row_deg.fill_(-7)
    H.census(graph, yt, c, out=buf)
    torch.cuda.synchronize()
    assert torch.equal(buf._buf, first[0]) and torch.equal(buf.row_same, first[1]) and torch.equal(buf.row_deg, first[2])
    return graph


@pytest.mark.parametrize("c", LF.CENSUS_BALLOT_CLASSES)
def test_census_is_exact_on_both_sides_of_the_per_lane_counter_limit(c):
    n = LF.CENSUS_SMALL_N
    e, y = _symmetric_random_graph(n, c, 40 + c, pairs=5 * n, unlabeled=200, hub=600)
    ip, ix = R.csr_of_edges(e, n)
    graph = _census_twice(ip, ix, y, c, n, chunk=128)
    assert graph.n_long_rows > 0                               # the hub row is split into pieces


@pytest.mark.parametrize("c", LF.CENSUS_BALLOT_CLASSES)
def test_census_is_exact_past_the_edges_and_finish_grid_caps(c):
    n = LF.CENSUS_EDGES_N
    e, y = _symmetric_random_graph(n, c, 50 + c, pairs=3 * n // 2, unlabeled=2000)
    ip, ix = R.csr_of_edges(e, n)
    _census_twice(ip, ix, y, c, n)


def test_census_is_exact_past_the_prep_grid_cap():
    n = LF.CENSUS_PREP_N
    i = np.arange(n, dtype=np.int64)
    e = np.concatenate([np.stack([i, (i + 1) % n], 1), np.stack([i, (i - 1) % n], 1)]).astype(np.int32)
    y = np.random.default_rng(61).integers(0, 2, n).astype(np.int64)
    ip, ix = R.csr_of_edges(e, n)
    _census_twice(ip, ix, y, 2, n)
