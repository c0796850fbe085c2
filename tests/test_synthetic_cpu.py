"""The synthetic graph generator without a GPU: the new entry points are exported and fail loudly with their status codes, the
wrappers reject what they cannot take, the numpy restatement of the sampling contract (tests/synthetic_ref.py) reproduces the
facts recorded from the reference's ``graph_generation.py`` (tests/golden/make_synthetic_golden.py) that do not depend on its
unseeded generators, and its samples are uniform."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import synthetic_ref as R
from conftest import GOLDEN

EINVAL, ESHAPE, EUNSUPPORTED, ENOMEM = 1, 2, 4, 5
HOMOS = (0.1, 0.3, 0.5, 0.9)
NEW_SYMBOLS = ("acm_synth_regular", "acm_synth_uniform", "acm_synth_random_plan", "acm_synth_draw", "acm_synth_select_workspace_bytes",
               "acm_synth_select", "acm_synth_inter_count", "acm_synth_emit")
def _golden():
    with np.load(os.path.join(GOLDEN, "synthetic_cases.npz")) as f:
        return {k: f[k] for k in f.files}


def test_symbols_are_exported_and_the_abi_number_stays():
    from acm_gnn_amd import _lib
    import acm_gnn_amd
    lib = _lib.load()
    assert lib.acm_version() == 29 == _lib.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert acm_gnn_amd.synthetic.generate_graph and "synthetic" in acm_gnn_amd.__all__


def test_new_entry_points_fail_loudly_without_a_gpu():
    from acm_gnn_amd import _lib
    lib = _lib.load()
    buf = (C.c_double * 64)()                                             # a real host address: argument checks come before any launch
    p = C.cast(buf, C.c_void_p)
    # regular
    assert lib.acm_synth_regular(5, 400, 2, 18, 0, 0, 0, 2000, None, None) == EINVAL
    assert b"acm_synth_regular" in lib.acm_last_error()
    assert lib.acm_synth_regular(1, 400, 2, 18, 0, 0, 0, 400, p, None) == ESHAPE
    assert lib.acm_synth_regular(5, 400, 400, 18, 0, 0, 0, 2000, p, None) == ESHAPE          # degree_intra > npc - 1
    assert lib.acm_synth_regular(5, 40, 2, 161, 0, 0, 0, 200, p, None) == ESHAPE             # degree_inter > n - npc
    assert lib.acm_synth_regular(5, 400, 2, 18, 0, 0, 5, 2001, p, None) == ESHAPE            # rows beyond n
    assert lib.acm_synth_regular(5, 400, 2, 18, 0, 0, 7, 5, p, None) == ESHAPE
    assert lib.acm_synth_regular(2, 2 ** 30, 2, 18, 0, 0, 0, 5, p, None) == ESHAPE           # 2^31 nodes
    assert lib.acm_synth_regular(65, 400, 2, 18, 0, 0, 0, 2000, p, None) == EUNSUPPORTED
    assert lib.acm_synth_regular(5, 400, 57, 200, 0, 0, 0, 2000, p, None) == EUNSUPPORTED    # d = 257 > the cap
    assert b"257" in lib.acm_last_error()
    # uniform features
    assert lib.acm_synth_uniform(4, 8, 0, 0, 0, None, 8, None) == EINVAL
    assert lib.acm_synth_uniform(4, 0, 0, 0, 0, p, 8, None) == ESHAPE
    assert lib.acm_synth_uniform(4, 8, 0, 0, 0, p, 7, None) == ESHAPE                        # ld < F
    assert lib.acm_synth_uniform(4, 8, 0, 0, 2 ** 32, p, 8, None) == ESHAPE                  # the row field has 32 bits
    assert lib.acm_synth_uniform(4, 262145, 0, 0, 0, p, 262145, None) == EUNSUPPORTED
    # the random type's plan (host only: it answers)
    plan = (C.c_int64 * 2)()
    assert lib.acm_synth_random_plan(5, 400, 2, 0.3, None) == EINVAL
    assert lib.acm_synth_random_plan(5, 401, 3, 0.3, plan) == ESHAPE and b"even" in lib.acm_last_error()
    assert lib.acm_synth_random_plan(5, 400, 400, 0.3, plan) == ESHAPE
    assert lib.acm_synth_random_plan(5, 400, 2, 0.0, plan) == ESHAPE
    assert lib.acm_synth_random_plan(5, 400, 2, 1.5, plan) == ESHAPE
    assert lib.acm_synth_random_plan(3, 8, 6, 0.1, plan) == ESHAPE and b"slots" in lib.acm_last_error()   # 433 edges, 128 slots
    assert lib.acm_synth_random_plan(65, 400, 2, 0.3, plan) == EUNSUPPORTED
    for h, want in zip(HOMOS, (7201, 1868, 801, 90)):
        assert lib.acm_synth_random_plan(5, 400, 2, h, plan) == 0 and list(plan) == [400, want], h
    # streams of keys
    assert lib.acm_synth_draw(0, 8, 1, 0, 1, 0, 0, 16, None, None) == EINVAL
    assert lib.acm_synth_draw(3, 8, 1, 0, 1, 0, 0, 16, p, None) == EINVAL and b"kind" in lib.acm_last_error()
    assert lib.acm_synth_draw(0, 0, 1, 0, 1, 0, 0, 16, p, None) == ESHAPE
    assert lib.acm_synth_draw(1, 8, 2 ** 31, 0, 1, 0, 0, 16, p, None) == ESHAPE
    assert lib.acm_synth_draw(1, 8, 8, 0, 1, 0, 0, 2 ** 31, p, None) == ESHAPE
    assert lib.acm_synth_draw(1, 8, 8, 65535, 1, 0, 0, 16, p, None) == EUNSUPPORTED          # the block field has 16 bits
    nbytes = C.c_size_t()
    assert lib.acm_synth_select_workspace_bytes(1, 100, None) == EINVAL
    assert lib.acm_synth_select_workspace_bytes(0, 100, C.byref(nbytes)) == ESHAPE
    assert lib.acm_synth_select_workspace_bytes(65536, 100, C.byref(nbytes)) == EUNSUPPORTED
    sizes = []
    for t in (0, 1, 4096, 4097, 40_000_000):
        assert lib.acm_synth_select_workspace_bytes(1, t, C.byref(nbytes)) == 0
        sizes.append(nbytes.value)
    assert 0 < sizes[0] < sizes[1] == sizes[2] < sizes[3] < sizes[4] <= 40_000_000 * 1.01 + 4096 + 1024   # a byte per draw
    assert lib.acm_synth_select(1, 16, None, p, p, p, 4, p, p, p, p, 1 << 20, None) == EINVAL
    assert b"acm_synth_select" in lib.acm_last_error()
    assert lib.acm_synth_select(0, 16, p, p, p, p, 4, p, p, p, p, 1 << 20, None) == ESHAPE
    assert lib.acm_synth_select(1, 16, p, p, p, p, -1, p, p, p, p, 1 << 20, None) == ESHAPE
    assert lib.acm_synth_select(65536, 16, p, p, p, p, 4, p, p, p, p, 1 << 20, None) == EUNSUPPORTED
    assert lib.acm_synth_select(1, 16, p, p, p, p, 4, p, p, p, p, 8, None) == ENOMEM and b"workspace 8 B" in lib.acm_last_error()
    assert lib.acm_synth_select(1, 16, p, p, p, p, 4, p, p, p, None, 0, None) == ENOMEM
    odd = C.c_void_p(((p.value + 15) & ~15) + 8)
    assert lib.acm_synth_select(1, 16, p, p, p, p, 4, p, p, p, odd, 1 << 20, None) == EINVAL and b"aligned" in lib.acm_last_error()
    # the chain
    assert lib.acm_synth_inter_count(5, 0, 7200.0, None, p, None) == EINVAL
    assert lib.acm_synth_inter_count(5, 4, 7200.0, p, p, None) == ESHAPE                     # the last class sends nothing
    assert lib.acm_synth_inter_count(5, 0, -1.0, p, p, None) == ESHAPE
    assert lib.acm_synth_inter_count(65, 0, 7200.0, p, p, None) == EUNSUPPORTED
    assert lib.acm_synth_emit(0, 5, 400, 0, 5, None, p, 400, p, p, None) == EINVAL
    assert lib.acm_synth_emit(2, 5, 400, 0, 5, p, p, 400, p, p, None) == EINVAL and b"kind" in lib.acm_last_error()
    assert lib.acm_synth_emit(0, 5, 400, 0, 6, p, p, 400, p, p, None) == ESHAPE
    assert lib.acm_synth_emit(1, 5, 400, 4, 1, p, p, 400, p, p, None) == ESHAPE
    assert lib.acm_synth_emit(1, 5, 400, 0, 1, p, p, -1, p, p, None) == ESHAPE
    assert lib.acm_synth_emit(0, 65, 400, 0, 5, p, p, 400, p, p, None) == EUNSUPPORTED


def test_wrappers_reject_bad_arguments():
    from acm_gnn_amd import synthetic as S
    ok = dict(n_classes=5, nodes_per_class=400, degree_intra=2, edge_homo=0.3)
    for bad, match in ((dict(n_classes=1), "classes"), (dict(n_classes=65), "classes"), (dict(nodes_per_class=0), "nodes_per_class"),
                       (dict(nodes_per_class=2 ** 30), "nodes_per_class"), (dict(seed=-1), "seed"), (dict(graph_index=2 ** 64), "seed"),
                       (dict(degree_intra=-1), "degree_intra"), (dict(edge_homo=0.0), "edge_homo"), (dict(edge_homo=1.5), "edge_homo")):
        for kind in ("regular", "random"):
            with pytest.raises(ValueError, match=match):
                S.generate_graph(kind, **dict(ok, **bad))
    with pytest.raises(ValueError, match="graph_type"):
        S.generate_graph("ring", **ok)
    with pytest.raises(ValueError, match="degrees"):
        S.generate_graph("regular", **dict(ok, degree_intra=400))
    with pytest.raises(ValueError, match="degrees"):
        S.generate_graph("regular", **dict(ok, nodes_per_class=4, edge_homo=0.1))              # 18 of 16 outside nodes
    with pytest.raises(ValueError, match="degree 400"):
        S.generate_graph("regular", **dict(ok, degree_intra=200, edge_homo=0.5))
    with pytest.raises(ValueError, match="rows"):
        S.generate_graph("regular", rows=(5, 2001), **ok)
    with pytest.raises(ValueError, match="rows"):
        S.generate_graph("random", rows=(0, 5), **ok)
    with pytest.raises(ValueError, match="even"):
        S.generate_graph("random", **dict(ok, nodes_per_class=401, degree_intra=3))
    for kind in ("regular", "random"):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            S.generate_graph(kind, device="cpu", **ok)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.random_features(10, 4, device="cpu")
    with pytest.raises(ValueError, match="random_features"):
        S.random_features(10, 0)
    y = torch.arange(12, dtype=torch.int64) % 3
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.generate_base_features(torch.zeros(12, 4), y, n_classes=3, nodes_per_class=2)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.base_feature_rows(y, n_classes=3, nodes_per_class=2)
    with pytest.raises(ValueError, match="int64"):
        S.base_feature_rows(y.int(), n_classes=3, nodes_per_class=2)
    with pytest.raises(ValueError, match="one label per row"):
        S.generate_base_features(torch.zeros(11, 4), y, n_classes=3, nodes_per_class=2)
    with pytest.raises(ValueError, match="contiguous int64"):
        S.select_distinct(torch.zeros(2, 8), torch.zeros(2, dtype=torch.int64), 4)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        S.select_distinct(torch.zeros(2, 8, dtype=torch.int64), torch.zeros(2, dtype=torch.int64), 4)
    assert S.stream_draws(400, 79800, 1 - 1 / 400) < 700 and S.stream_draws(24, 28) > 60 and S.stream_draws(0, 10) == 64


@pytest.mark.parametrize("h", HOMOS)
def test_restatement_reproduces_the_recorded_facts_regular(h):
    g = _golden()
    c, npc, k = int(g["n_classes"]), int(g["nodes_per_class"]), int(g["degree_intra"])
    ref = {key: g[f"regular:{h}:{key}"] for key in ("blocks", "degree_min", "degree_max", "trace", "symmetric", "degree_inter")}
    d_inter = R.degree_inter_of(k, h)
    assert d_inter == int(ref["degree_inter"]) == {0.1: 18, 0.3: 4, 0.5: 2, 0.9: 0}[h]
    ix = R.regular(c, npc, k, d_inter, seed=0, graph_index=0)
    n = c * npc
    assert ix.shape == (n, k + d_inter) and int(ref["degree_min"]) == int(ref["degree_max"]) == k + d_inter
    assert (np.diff(ix.astype(np.int64), axis=1) > 0).all() and ix.min() >= 0 and ix.max() < n        # sorted, distinct, in range
    assert not (ix == np.arange(n)[:, None]).any() and int(ref["trace"]) == 0                        # no self loop
    blocks = R.block_counts(np.arange(n + 1) * ix.shape[1], ix.reshape(-1), c, npc)
    assert np.diag(blocks).tolist() == np.diag(ref["blocks"]).tolist() == [k * npc] * c
    off = blocks.sum(1) - np.diag(blocks)
    assert off.tolist() == (ref["blocks"].sum(1) - np.diag(ref["blocks"])).tolist() == [npc * d_inter] * c
    dense = np.zeros((n, n), bool)
    dense[np.arange(n)[:, None], ix] = True
    assert not bool(ref["symmetric"]) and not (dense == dense.T).all()                               # directed rows


@pytest.mark.parametrize("h", HOMOS)
def test_restatement_reproduces_the_recorded_facts_random(h):
    g = _golden()
    c, npc, k = int(g["n_classes"]), int(g["nodes_per_class"]), int(g["degree_intra"])
    ref = {key: g[f"random:{h}:{key}"] for key in ("blocks", "trace", "symmetric")}
    got = R.random_graph(c, npc, k, h, seed=0, graph_index=0)
    n, blocks = c * npc, got["block_counts"]
    assert np.diag(blocks).tolist() == np.diag(ref["blocks"]).tolist() == [k * npc] * c
    want = round(k * npc * (1 - h) / h) + 1
    assert want == {0.1: 7201, 0.3: 1868, 0.5: 801, 0.9: 90}[h]
    for b in (blocks, ref["blocks"]):                                     # every class but the last ends with round(T) + 1
        assert (b == b.T).all() and (b.sum(1) - np.diag(b))[:-1].tolist() == [want] * (c - 1)
    assert blocks.tolist() == R.block_counts(got["indptr"], got["indices"], c, npc).tolist()
    dense = np.zeros((n, n), bool)
    dense[np.repeat(np.arange(n), np.diff(got["indptr"])), got["indices"]] = True
    assert bool(ref["symmetric"]) and (dense == dense.T).all() and int(ref["trace"]) == 0 and not dense.diagonal().any()
    assert dense.sum() == len(got["indices"]) == blocks.sum()             # no duplicate entry
    rows = np.repeat(np.arange(n), np.diff(got["indptr"]))
    key = rows.astype(np.int64) * n + got["indices"]
    assert (np.diff(key) > 0).all()                                       # rows sorted by column


def test_restatement_is_uniform():
    """chi-square of the regular type's intra offsets over their 399 cells and inter offsets over 1 600 cells (5 x 400,
    degree_intra 2, h 0.1, seed 0), and of the random type's intra pair slots, against the 1 - 1e-6 quantile."""
    c, npc, k, d_inter = 5, 400, 2, 18
    j = np.arange(c * npc)
    intra = R.floyd(0, 0, R.TAG_REG_INTRA, j, k, npc - 1)
    inter = R.floyd(0, 0, R.TAG_REG_INTER, j, d_inter, c * npc - npc)
    for sample, cells in ((intra, npc - 1), (inter, c * npc - npc)):
        assert (np.sort(sample, 1)[:, 1:] != np.sort(sample, 1)[:, :-1]).all()                      # distinct inside a row
        stat, bound = R.chi2(np.bincount(sample.reshape(-1), minlength=cells)), R.chi2_quantile(cells - 1, 1e-6)
        print(f"chi2 over {cells} cells: {stat:.1f} < {bound:.1f}")
        assert stat < bound, (cells, stat, bound)
    # pair slots of a 9-node block: 20 000 draws of five streams -> keys uniform over the 36 pairs
    keys = np.concatenate([R.draw_keys(R.PAIR, 9, 1, b, 0, 0, 4000) for b in range(5)])
    valid = keys[keys != R.INVALID]
    assert abs(len(valid) / len(keys) - 8 / 9) < 0.01                     # x == y is one slot in nine
    x, y = valid // 9, valid % 9
    assert (x < y).all()
    cells = np.bincount(x * 9 + y, minlength=81)[np.triu(np.ones((9, 9), bool), 1).reshape(-1)]
    stat, bound = R.chi2(cells), R.chi2_quantile(35, 1e-6)
    print(f"chi2 over 36 pairs: {stat:.1f} < {bound:.1f}")
    assert stat < bound
    # ... and the selected S / 2 = 400 of 79 800 pairs of the golden shape touch every node about equally
    sel = np.concatenate([R.select(R.PAIR, npc, 1, b, 0, 0, 400) for b in range(c)])
    ends = np.bincount(np.concatenate([sel // npc, sel % npc]), minlength=npc)
    stat, bound = R.chi2(ends), R.chi2_quantile(npc - 1, 1e-6)
    print(f"chi2 of pair end points over {npc} nodes: {stat:.1f} < {bound:.1f}")
    assert stat < bound


def test_selection_does_not_depend_on_the_stream_length_and_the_chain_clamps():
    a = R.select(R.PAIR, 8, 1, 2, 7, 3, 24, n_draws=8)                    # the dense corner: 24 of 28 pairs, extended from 8 draws
    b = R.select(R.PAIR, 8, 1, 2, 7, 3, 24, n_draws=4096)
    assert a.tolist() == b.tolist() and len(set(a.tolist())) == 24
    assert R.select(R.PAIR, 8, 1, 2, 7, 3, 29) is None                    # more than there are
    assert R.first_distinct(R.draw_keys(R.RANGE, 5, 1, 0, 0, 0, 64), 0)[0].tolist() == []
    seed, i = R.clamp_seed()
    g = R.random_graph(seed=seed, graph_index=0, **R.CLAMP_CASE)
    npc = R.CLAMP_CASE["npc"]
    assert g["pre_clamp"][i] < 0 and g["m"][i] == 0                       # the clamp max(0, .), not the arithmetic
    assert g["block_counts"][i, i + 1:].sum() == 0                        # class i sends nothing toward later classes
    rows = np.repeat(np.arange(len(g["indptr"]) - 1), np.diff(g["indptr"]))
    sent = (rows // npc == i) & (g["indices"] // npc > i)
    assert not sent.any() and g["block_counts"][:i, i].sum() >= 4
    rows = R.base_feature_rows(np.arange(40) % 4, 5, 6, 1, 0)             # 10 members > 6: six distinct members of class j % 4
    assert rows.shape == (30,) and all(len(set(rows[6 * j:6 * j + 6].tolist())) == 6 and (rows[6 * j:6 * j + 6] % 4 == j % 4).all()
                                       for j in range(5))
    rows = R.base_feature_rows(np.arange(16) % 4, 5, 6, 1, 0)             # 4 members <= 6: all four, then two further ones
    assert rows[:4].tolist() == [0, 4, 8, 12] and len(set(rows[4:6].tolist())) == 2
    with pytest.raises(ValueError):
        R.base_feature_rows(np.arange(8) % 4, 5, 6, 1, 0)                 # 2 members, 4 further ones wanted
