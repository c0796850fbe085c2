"""Record summaries of the reference's synthetic graphs -> tests/golden/synthetic_cases.npz.

    python tests/golden/make_synthetic_golden.py /path/to/ACM-GNN

Imports ``synthetic-experiments/graph_generation.py`` of the reference checkout (both the checkout and its
``synthetic-experiments`` directory go on ``sys.path``), replaces its ``save_graphs`` with a capture and runs
``generate_graph`` for both graph types at 5 x 400 nodes, degree_intra = 2, h in {0.1, 0.3, 0.5, 0.9}, in a scratch working
directory (the reference creates ./logs and ./synthetic_graphs where it runs).  Only SUMMARIES are recorded: the C x C block
edge-count matrix, the per-row degree minimum and maximum, the trace, whether the matrix is symmetric, degree_inter and the
elapsed seconds per graph.  The reference's generators are seeded by nothing, so the inter-class cells differ from run to
run; the tests pin the facts that do not (tests/test_synthetic_cpu.py)."""
import argparse
import os
import sys
import tempfile
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
C, NPC, DEGREE_INTRA = 5, 400, 2
HOMOS = (0.1, 0.3, 0.5, 0.9)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="checkout of the reference repository")
    ap.add_argument("--out", default=os.path.join(HERE, "synthetic_cases.npz"))
    args = ap.parse_args()
    ref = os.path.abspath(args.reference)
    sys.path[:0] = [ref, os.path.join(ref, "synthetic-experiments")]
    rec = {"homos": np.array(HOMOS), "n_classes": np.int64(C), "nodes_per_class": np.int64(NPC), "degree_intra": np.int64(DEGREE_INTRA)}
    with tempfile.TemporaryDirectory() as scratch:
        os.chdir(scratch)
        import graph_generation as gg
        captured = []
        gg.save_graphs = lambda base, homo, num, adj, degree, label: captured.append(np.array(adj))
        for kind in ("regular", "random"):
            for h in HOMOS:
                ns = types.SimpleNamespace(num_class=C, num_node_total=C * NPC, degree_intra=DEGREE_INTRA, num_graph=1,
                                           graph_type=kind, edge_homos=[h])
                captured.clear()
                t0 = time.perf_counter()
                gg.generate_graph(ns)
                dt = time.perf_counter() - t0
                a = captured[0]
                assert set(np.unique(a)) <= {0.0, 1.0}
                tag = f"{kind}:{h}"
                rec[f"{tag}:blocks"] = a.reshape(C, NPC, C, NPC).sum((1, 3)).astype(np.int64)
                deg = a.sum(1)
                rec[f"{tag}:degree_min"], rec[f"{tag}:degree_max"] = np.int64(deg.min()), np.int64(deg.max())
                rec[f"{tag}:trace"] = np.int64(np.trace(a))
                rec[f"{tag}:symmetric"] = np.bool_((a == a.T).all())
                rec[f"{tag}:degree_inter"] = np.int64(int(DEGREE_INTRA / h - DEGREE_INTRA))
                rec[f"{tag}:seconds"] = np.float64(dt)
                print(tag, rec[f"{tag}:blocks"].tolist(), int(deg.min()), int(deg.max()), f"{dt:.3f} s")
        os.chdir(HERE)
    np.savez_compressed(args.out, **rec)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
