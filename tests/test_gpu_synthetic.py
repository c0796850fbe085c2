"""The synthetic graph generator on the GPU (acm_synth.hip): device output equals the numpy restatement of the sampling contract
(tests/synthetic_ref.py) bit for bit, slices concatenate to the whole, the stream length does not change a result, the select
primitive keeps inside its output, and the generated graphs carry the facts recorded from the reference, feed the census, the
filter construction and a training run."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import launch_forms as LF
import synthetic_ref as R
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

DEV = "cuda"
HOMOS = (0.1, 0.3, 0.5, 0.9)
# (C, npc, degree_intra, h): the golden shapes; wave tails; row ids above 2^16; the whole block chosen; every outside node
# chosen; d at the cap of 256
REGULAR_CASES = [(5, 400, 2, h) for h in HOMOS] + [(3, 37, 5, 0.25), (2, 35_000, 3, 0.5), (3, 5, 4, 0.5), (2, 6, 3, 1 / 3), (2, 300, 128, 0.5)]
RANDOM_CASES = [(5, 400, 2, h) for h in HOMOS] + [(3, 37, 4, 0.4), (2, 35_000, 2, 0.5)]


def _np(t):
    return t.cpu().numpy()


def _gen(kind, c, npc, k, h, seed=0, graph_index=0, **kw):
    from acm_gnn_amd import synthetic as S
    return S.generate_graph(kind, n_classes=c, nodes_per_class=npc, degree_intra=k, edge_homo=h, seed=seed, graph_index=graph_index,
                            device=DEV, **kw)


def _assert_random_equals(g, want):
    assert np.array_equal(_np(g.indptr), want["indptr"]) and g.indptr.dtype == torch.int32
    assert np.array_equal(_np(g.indices), want["indices"]) and g.indices.dtype == torch.int32
    assert _np(g.block_counts).tolist() == want["block_counts"].tolist()
    assert g.info["m"] == want["m"].tolist()


# ---- regular ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,npc,k,h", REGULAR_CASES)
def test_regular_equals_the_restatement_bit_for_bit(c, npc, k, h):
    d_inter = R.degree_inter_of(k, h)
    n, d = c * npc, k + d_inter
    if (c, npc) == (2, 6):
        assert d_inter == n - npc                                         # every outside node
    if (c, npc) == (2, 300):
        assert d == R.MAX_DEGREE
    g = _gen("regular", c, npc, k, h, seed=11, graph_index=3)
    want = R.regular(c, npc, k, d_inter, 11, 3)
    assert g.indices.dtype == torch.int32 and np.array_equal(_np(g.indices).reshape(n, d), want)
    assert np.array_equal(_np(g.indptr), np.arange(n + 1) * d) and g.info["degree_inter"] == d_inter
    assert _np(g.block_counts).tolist() == R.block_counts(np.arange(n + 1) * d, want.reshape(-1), c, npc).tolist()
    assert _np(g.degree).tolist() == [d] * n and _np(g.labels).tolist() == (np.arange(n) // npc).tolist()
    if npc == k + 1:                                                      # the whole block but the row itself
        for j in range(n):
            base = j // npc * npc
            assert [v for v in want[j].tolist() if base <= v < base + npc] == [v for v in range(base, base + npc) if v != j]


def test_regular_slices_concatenate_is_deterministic_and_moves_with_the_graph_index():
    whole = _gen("regular", 5, 400, 2, 0.1, seed=5, graph_index=2)
    parts = [_gen("regular", 5, 400, 2, 0.1, seed=5, graph_index=2, rows=r) for r in ((0, 777), (777, 2000))]
    assert torch.equal(torch.cat([p.indices for p in parts]), whole.indices)
    assert parts[1].rows == (777, 2000) and parts[1].indptr.shape[0] == 2000 - 777 + 1
    assert torch.equal(parts[0].block_counts + parts[1].block_counts, whole.block_counts)
    assert _gen("regular", 5, 400, 2, 0.1, seed=5, graph_index=2, rows=(9, 9)).indices.numel() == 0
    again = _gen("regular", 5, 400, 2, 0.1, seed=5, graph_index=2)
    assert torch.equal(again.indices, whole.indices)
    other = _gen("regular", 5, 400, 2, 0.1, seed=5, graph_index=3)
    assert not torch.equal(other.indices, whole.indices)
    assert not torch.equal(_gen("regular", 5, 400, 2, 0.1, seed=6, graph_index=2).indices, whole.indices)
    with pytest.raises(ValueError, match="row slice"):
        parts[0].operators()
    with pytest.raises(ValueError, match="row slice"):
        parts[0].adj


# ---- random ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,npc,k,h", RANDOM_CASES)
def test_random_equals_the_restatement_bit_for_bit(c, npc, k, h):
    g = _gen("random", c, npc, k, h, seed=11, graph_index=3)
    _assert_random_equals(g, R.random_graph(c, npc, k, h, 11, 3))
    assert g.info["attempts"] == 1                                        # the default stream lengths hold what is asked


def test_random_dense_corner_with_a_short_first_stream_is_extended():
    """C = 3, npc = 8, degree_intra = 6: 24 of the 28 pairs of every block, duplicates dominate; a first stream of 8 draws
    cannot hold 24 keys, so the wrapper extends it -- and the result is what a long stream gives."""
    want = R.random_graph(3, 8, 6, 0.5, 4, 1)
    short = _gen("random", 3, 8, 6, 0.5, seed=4, graph_index=1, stream_length=8)
    assert short.info["attempts"] >= 3
    _assert_random_equals(short, want)
    _assert_random_equals(_gen("random", 3, 8, 6, 0.5, seed=4, graph_index=1), want)
    _assert_random_equals(_gen("random", 3, 8, 6, 0.5, seed=4, graph_index=1, stream_length=5000), want)
    assert np.diag(want["block_counts"]).tolist() == [48] * 3
    other = _gen("random", 3, 8, 6, 0.5, seed=4, graph_index=2)
    assert not (torch.equal(other.indices, short.indices) and torch.equal(other.indptr, short.indptr))


def test_random_chain_clamps_a_class_that_already_has_too_many():
    """A case where round(T - e_i) + 1 is NEGATIVE (found with the restatement on the CPU: synthetic_ref.clamp_seed), so that
    m_i = 0 is the work of the clamp in the chain's own kernel."""
    seed, i = R.clamp_seed()
    case = R.CLAMP_CASE
    want = R.random_graph(seed=seed, graph_index=0, **case)
    assert want["pre_clamp"][i] < 0
    g = _gen("random", case["n_classes"], case["npc"], case["degree_intra"], case["edge_homo"], seed=seed)
    _assert_random_equals(g, want)
    assert g.info["m"][i] == 0 and g.info["found"][i] == 0
    assert int(g.block_counts[i, i + 1:].sum()) == 0
    rows = np.repeat(np.arange(g.n), np.diff(_np(g.indptr)))
    assert not ((rows // case["npc"] == i) & (_np(g.indices) // case["npc"] > i)).any()      # no entry from class i to a later one


def test_recorded_facts_hold_on_device_output():
    with np.load(os.path.join(GOLDEN, "synthetic_cases.npz")) as f:
        rec = {k: f[k] for k in f.files}
    from acm_gnn_amd import homophily as H
    for h in HOMOS:
        g = _gen("regular", 5, 400, 2, h)
        d_inter = int(rec[f"regular:{h}:degree_inter"])
        b = _np(g.block_counts)
        assert np.diag(b).tolist() == [800] * 5 == np.diag(rec[f"regular:{h}:blocks"]).tolist()
        assert (b.sum(1) - np.diag(b)).tolist() == [400 * d_inter] * 5
        assert _np(g.degree).min() == _np(g.degree).max() == 2 + d_inter == int(rec[f"regular:{h}:degree_max"])
        assert H.census(g.adj, g.labels).edge == 2 / (2 + d_inter)       # exactly: every row has the same shares
        g = _gen("random", 5, 400, 2, h)
        b = _np(g.block_counts)
        want = round(800 * (1 - h) / h) + 1
        assert np.diag(b).tolist() == [800] * 5 and (b == b.T).all()
        assert (b.sum(1) - np.diag(b))[:-1].tolist() == [want] * 4 == (rec[f"random:{h}:blocks"].sum(1) - 800)[:-1].tolist()
        ip, ix = _np(g.indptr).astype(np.int64), _np(g.indices).astype(np.int64)
        key = np.repeat(np.arange(2000), np.diff(ip)) * 2000 + ix
        assert (np.diff(key) > 0).all() and not (np.repeat(np.arange(2000), np.diff(ip)) == ix).any()   # sorted rows, zero diagonal
        assert np.array_equal(np.sort(ix * 2000 + np.repeat(np.arange(2000), np.diff(ip))), key)         # symmetric
        census = H.census(g.adj, g.labels)
        assert census.host()[0].tolist() == b.tolist()
        assert census.edge == float(np.trace(b)) / float(b.sum()) and abs(census.edge - h) < 0.01


# ---- the select primitive ----------------------------------------------------------------------------------------------------
def _select_raw(keys, m, cap, guard=16):
    """acm_synth_select on hand-made keys with guard bands of -7 around out -> (out with bands, found, status)."""
    from acm_gnn_amd import _lib
    from acm_gnn_amd.synthetic import _launch
    g, t = keys.shape
    kt = torch.from_numpy(keys).to(DEV)
    sk, perm = torch.sort(kt, dim=1, stable=True)
    mt = torch.tensor(m, dtype=torch.int64, device=DEV)
    out = torch.full((guard + g * cap + guard,), -7, dtype=torch.int64, device=DEV)
    found = torch.full((g,), -7, dtype=torch.int64, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    nbytes = C.c_size_t()
    assert _lib.load().acm_synth_select_workspace_bytes(g, t, C.byref(nbytes)) == 0
    ws = torch.empty(nbytes.value // 8 + 1, dtype=torch.int64, device=DEV)
    _launch("acm_synth_select", kt.device, g, t, C.c_void_p(kt.data_ptr()), C.c_void_p(sk.data_ptr()), C.c_void_p(perm.data_ptr()),
            C.c_void_p(mt.data_ptr()), cap, C.c_void_p(out.data_ptr() + 8 * guard), C.c_void_p(found.data_ptr()),
            C.c_void_p(status.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel() * 8)
    torch.cuda.synchronize()
    out = _np(out)
    assert (out[:guard] == -7).all() and (out[guard + g * cap:] == -7).all()
    return out[guard:guard + g * cap].reshape(g, cap), _np(found).tolist(), int(status.cpu()[0])


def test_select_primitive_edges():
    inv = R.INVALID
    keys = np.array([[3, 3, inv, 5, 3, 5, 9]], np.int64)
    out, found, status = _select_raw(keys, [0], 4)
    assert found == [0] and status == 0 and (out == -7).all()                                  # M = 0: nothing written
    out, found, status = _select_raw(keys, [5], 6)                                             # more than the 3 distinct keys
    assert found == [3] and status == 1 and out[0].tolist() == [3, 5, 9, -7, -7, -7]
    out, found, status = _select_raw(keys, [2], 4)
    assert found == [2] and status == 0 and out[0].tolist() == [3, 5, -7, -7]
    wide = np.array([[8, 1, 8, 7, 2, 1, 6, 5]], np.int64)
    out, found, status = _select_raw(wide, [6], 4)                                             # M beyond the output: capped
    assert found == [4] and status == 2 and out[0].tolist() == [8, 1, 7, 2]
    out, found, status = _select_raw(wide, [-3], 4)                                            # a negative M counts as 0
    assert found == [0] and status == 0 and (out == -7).all()
    # three chunks of 4096 draws, two segments with their own M, against the restatement
    rng = np.random.default_rng(0)
    big = rng.integers(0, 3000, (2, 9000)).astype(np.int64)
    big[rng.random((2, 9000)) < 0.1] = inv
    out, found, status = _select_raw(big, [2500, 17], 2600)
    for s, m in enumerate((2500, 17)):
        want, short = R.first_distinct(big[s], m)
        assert not short and found[s] == m and out[s, :m].tolist() == want.tolist() and (out[s, m:] == -7).all()
    assert status == 0
    out, found, status = _select_raw(big, [3001, 17], 3100)                                    # one segment short, the other not
    assert status == 1 and found[1] == 17 and found[0] == len(np.unique(big[0][big[0] != inv])) < 3001
    assert (out[0, found[0]:] == -7).all()


def test_draws_equal_the_restatement():
    from acm_gnn_amd import synthetic as S
    for kind, a, b, first, segs, t in ((R.PAIR, 400, 1, 0, 5, 601), (R.RECT, 400, 1600, 2, 1, 8755), (R.RANGE, 17, 1, 60, 3, 64),
                                       (R.PAIR, 35_000, 1, 1, 1, 1000), (R.RECT, 35_000, 35_000, 0, 1, 1001)):
        got = _np(S.draw_keys(kind, a, b, first, segs, 2 ** 63 + 5, 2 ** 40 + 1, t, DEV))
        for s in range(segs):
            assert np.array_equal(got[s], R.draw_keys(kind, a, b, first + s, 2 ** 63 + 5, 2 ** 40 + 1, t)), (kind, s)


# ---- operators, features, training -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["regular", "random"])
def test_operators_are_the_row_normalised_identity_plus_adjacency(kind):
    from acm_gnn_amd.graph import explicit_arrays
    g = _gen(kind, 5, 400, 2, 0.3, seed=2)
    n = 2000
    dense = np.zeros((n, n))
    dense[np.repeat(np.arange(n), np.diff(_np(g.indptr))), _np(g.indices)] = 1.0
    dense += np.eye(n)
    dense /= dense.sum(1, keepdims=True)                                  # float64 D^-1 (I + A), synthetic-experiments/train.py:72-78
    ip, ix, v = (_np(t) for t in explicit_arrays(g.operators()))
    got = np.zeros((n, n))
    got[np.repeat(np.arange(n), np.diff(ip)), ix] = v
    assert (got != 0).sum() == len(v) == (dense != 0).sum()
    assert np.abs(got - dense).max() <= 2.0 ** -25                        # one fp32 rounding of a quotient in (0, 1]: half an ulp


def test_features_equal_the_restatement():
    from acm_gnn_amd import synthetic as S
    for n, f, begin in ((37, 1433, 0), (129, 64, 5), (3, 1, 70_000)):      # scalar tail, 16-byte stores, a row offset
        got = S.random_features(n, f, seed=9, graph_index=4, device=DEV, row_begin=begin)
        assert got.dtype == torch.float32 and np.array_equal(_np(got), R.uniform(n, f, 9, 4, begin))
    assert S.random_features(0, 7, device=DEV).shape == (0, 7)
    x = _np(S.random_features(2000, 1433, seed=0, device=DEV))
    assert 0.0 <= x.min() and x.max() < 1.0 and abs(x.mean() - 0.5) < 1e-3
    rng = np.random.default_rng(1)
    base_y = rng.integers(0, 4, 300).astype(np.int64)                     # about 75 members per base class
    base_x = rng.standard_normal((300, 7)).astype(np.float32)
    yt, xt = torch.from_numpy(base_y).to(DEV), torch.from_numpy(base_x).to(DEV)
    for npc in (40, 100):                                                 # more members than wanted; fewer: all + further ones
        rows = S.base_feature_rows(yt, n_classes=5, nodes_per_class=npc, seed=3, graph_index=1)
        want = R.base_feature_rows(base_y, 5, npc, 3, 1)
        assert _np(rows).tolist() == want.tolist()
        feats = S.generate_base_features(xt, yt, n_classes=5, nodes_per_class=npc, seed=3, graph_index=1)
        assert np.array_equal(_np(feats), base_x[want])
    with pytest.raises(ValueError, match="larger sample"):
        S.base_feature_rows(yt, n_classes=5, nodes_per_class=200, seed=3)


def test_fit_runs_on_a_generated_graph():
    import acm_gnn_amd
    from acm_gnn_amd import synthetic as S, train as T
    g = _gen("random", 5, 400, 2, 0.3, seed=1)
    ops, y = g.operators(), g.labels
    x = S.random_features(g.n, 64, seed=1, device=DEV)
    x[torch.arange(g.n, device=DEV), y] += 1.0                            # a weak class signal in the first five columns
    order = torch.randperm(g.n, generator=torch.Generator().manual_seed(0)).to(DEV)
    sets = (order[:1200].sort().values, order[1200:1600].sort().values, order[1600:].sort().values)
    torch.manual_seed(1)
    model = acm_gnn_amd.GCN(64, 64, 5, 2, g.n, 0.0, "acmgcn", 0, variant=False).to(DEV)
    opt = acm_gnn_amd.FusedAdamW(model.parameters(), lr=0.02, weight_decay=1e-3)
    best, hist = T.fit(model, opt, x, ops, y, *sets, epochs=4)
    assert len(hist) == 4 and 0.0 <= best <= 1.0
    assert all(np.isfinite(row[0]) and np.isfinite(row[4]) and all(0.0 <= v <= 1.0 for v in row[1:4]) for row in hist)


# ---- second trips of the grid-stride loops, several chunk sums per thread of the scan ------------------------------------------
@pytest.mark.parametrize("n,f", LF.SYN_FEATURES)
def test_features_equal_the_restatement_past_the_grid_cap(n, f):
    """More quads of columns than the capped grid has threads: 16-byte stores (F % 4 == 0) and the scalar tail."""
    from acm_gnn_amd import synthetic as S
    got = S.random_features(n, f, seed=9, graph_index=4, device=DEV)
    assert np.array_equal(_np(got).view(np.int32), R.uniform(n, f, 9, 4).view(np.int32))


@pytest.mark.parametrize("kind,a,b", [(R.RANGE, 300_000, 7), (R.PAIR, 35_000, 1)], ids=["range", "pair"])
def test_draws_equal_the_restatement_past_the_grid_cap(kind, a, b):
    from acm_gnn_amd import synthetic as S
    t = LF.SYN_DRAWS
    got = _np(S.draw_keys(kind, a, b, 3, 1, 2 ** 63 + 5, 2 ** 40 + 1, t, DEV))
    assert got.shape == (1, t) and np.array_equal(got[0], R.draw_keys(kind, a, b, 3, 2 ** 63 + 5, 2 ** 40 + 1, t))


def test_select_with_several_chunk_sums_per_thread_of_the_scan():
    """More than 256 chunks of 4096 draws: every thread of the scan adds, and later prefixes, several chunk sums."""
    a, t, m = LF.SYN_SELECT["a"], LF.SYN_SELECT["draws"], LF.SYN_SELECT["m"]
    keys = R.draw_keys(R.RANGE, a, 1, 2, 77, 1, t)
    want, short = R.first_distinct(keys, m)
    assert not short and len(want) == m
    out, found, status = _select_raw(keys[None, :], [m], m + 5)
    assert found == [m] and status == 0
    assert np.array_equal(out[0, :m], want) and (out[0, m:] == -7).all()
