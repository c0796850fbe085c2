#!/usr/bin/env python3
"""Homophily cases recorded from the REFERENCE's own ``synthetic-experiments/homophily.py``, imported at generation time --
none of its text is copied:

    python tests/golden/make_homophily_golden.py /path/to/synthetic-experiments      # -> tests/golden/homophily_cases.npz

Each case holds the directed edge list of a small seeded graph (tests/homophily_ref.py: planted_graph), its labels, fp32
features, the CSR of the dense-normalised operator D^-1 (A + I), and what the reference returned on the dense matrices:

    ref_edge     edge_homophily(A, one_hot)                                   (fully labeled cases)
    ref_node     node_homophily_edge_idx(off-diagonal edge index, labels, n)
    ref_compat   compat_matrix_edge_idx(off-diagonal edge index, labels)
    ref_class    class_homophily(A, labels)                                   (every case; negative labels = unlabeled there)
    ref_agg      aggregation_homophily(features, D^-1 (A + I), one_hot)
    ref_agg_onehot   the same with features = one_hot (the label-based form)

The four label measures are taken on fp32 tensors, as the reference's callers do.  The two aggregation values are taken on
float64 copies of the same fp32 numbers: the n x n product and its class means are then formed in float64.  The reference
still stores the means in an fp32 ``weight_matrix`` (homophily.py:119) whatever the inputs' type, so its arg-max is taken over
fp32-rounded means; the generator allows the recorded value two rows of difference from the float64 restatement for that.
The generator asserts that the numpy restatement agrees with every recorded value to 5e-7."""
import importlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import homophily_ref as R  # noqa: E402

TOL = 5e-7


def cases():
    """tag -> (n, C, edges, labels, features)"""
    out = {}
    for tag, n, c, f, seed, kw in (("hub", 1500, 5, 12, 11, dict(hub=500, isolated=5)),
                                   ("c3f7", 700, 3, 7, 12, dict(k=3, h=0.5)),
                                   ("c10", 1031, 10, 10, 13, dict(k=5, h=0.6, isolated=2)),
                                   ("unlabeled", 900, 4, 4, 14, dict(k=4, h=0.65, isolated=3, unlabeled=60))):
        edges, y = R.planted_graph(n, c, seed, **kw)
        rng = np.random.default_rng(seed + 100)
        centers = rng.normal(size=(c, f))
        x = (centers[np.maximum(y, 0)] * (y >= 0)[:, None] + 1.5 * rng.normal(size=(n, f))).astype(np.float32)
        out[tag] = (n, c, edges, y, x)
    # hand-made: a triangle 0-1-2 with a raw self-loop on 1, node 3 isolated, node 4 unlabeled and tied to 0
    pairs = [(0, 1), (1, 2), (2, 0), (0, 4)]
    edges = np.array([(a, b) for a, b in pairs] + [(b, a) for a, b in pairs] + [(1, 1)], np.int32)
    out["hand"] = (5, 3, edges, np.array([0, 0, 1, 2, -1], np.int64),
                   np.array([[1, 0], [0, 1], [1, 0.5], [0.25, 1], [2, 2]], np.float32))
    return out


def main(ref_path):
    sys.path.insert(0, ref_path)
    ref = importlib.import_module("homophily")
    rec = {}
    for tag, (n, c, edges, y, x) in cases().items():
        assert set(range(c)) <= set(y.tolist()), tag
        a = np.zeros((n, n), np.float32)
        a[edges[:, 0], edges[:, 1]] = 1.0
        ip, ix, vals = R.normalised_operator(edges, n)
        aip, aix = R.csr_of_edges(edges, n)
        cs = R.census(aip, aix, y, c)
        labeled = bool((y >= 0).all())
        A, lab = torch.from_numpy(a), torch.from_numpy(y)
        rec[f"{tag}:edges"], rec[f"{tag}:labels"], rec[f"{tag}:features"] = edges, y, x
        rec[f"{tag}:n_classes"] = np.int64(c)
        rec[f"{tag}:norm_indptr"], rec[f"{tag}:norm_indices"], rec[f"{tag}:norm_vals"] = ip, ix, vals
        v = float(ref.class_homophily(A, lab))
        assert abs(v - R.klass(cs)) <= TOL, (tag, "class", v, R.klass(cs))
        rec[f"{tag}:ref_class"] = np.float64(v)
        line = [tag, f"class {v:.7f}"]
        if labeled:
            off = edges[edges[:, 0] != edges[:, 1]].astype(np.int64)
            onehot = torch.from_numpy(R.one_hot(y, c))
            v = float(ref.edge_homophily(A, onehot))
            assert abs(v - R.edge(cs)) <= TOL, (tag, "edge", v, R.edge(cs))
            rec[f"{tag}:ref_edge"] = np.float64(v)
            line.append(f"edge {v:.7f}")
            v = float(ref.node_homophily_edge_idx(torch.from_numpy(off.T.copy()), lab, n))
            assert abs(v - R.node(cs)) <= TOL, (tag, "node", v, R.node(cs))
            rec[f"{tag}:ref_node"] = np.float64(v)
            line.append(f"node {v:.7f}")
            h = ref.compat_matrix_edge_idx(torch.from_numpy(off), lab).double().numpy()
            assert np.abs(h - R.compat(cs)).max() <= TOL, (tag, "compat")
            rec[f"{tag}:ref_compat"] = h
            dense = np.zeros((n, n))
            rows = np.repeat(np.arange(n), np.diff(ip))
            dense[rows, ix] = vals.astype(np.float64)
            adj64 = torch.from_numpy(dense)
            for key, feats in (("ref_agg", x), ("ref_agg_onehot", R.one_hot(y, c))):
                v = float(ref.aggregation_homophily(torch.from_numpy(feats.astype(np.float64)), adj64, onehot.double()))
                hits, _ = R.agg_rows(R.dense_times(ip, ix, vals, feats), y, c)
                assert abs(v - hits.mean()) <= 2.0 / n, (tag, key, v, hits.mean())
                rec[f"{tag}:{key}"] = np.float64(v)
                line.append(f"{key} {v:.7f}")
        print(*line)
    path = os.path.join(HERE, "homophily_cases.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
