#!/usr/bin/env python3
"""ROC-AUC cases recorded from the REFERENCE's own ``data_utils.eval_rocauc`` (ACM-Geometric/data_utils.py:128-151), imported at
generation time -- none of its text is copied:

    python tests/golden/make_rocauc_golden.py /path/to/ACM-Geometric      # -> tests/golden/rocauc_cases.npz

Each case holds logits [n, C], labels [n], three index sets, the three values the reference returned for
``eval_rocauc(label[idx], out[idx])`` and the exact integer triples (U2, npos, nneg) of tests/rocauc_ref.py; the generator
asserts ``reference value == U2 / (2 npos nneg)`` to 1e-12 for every one.  ``data_utils`` imports two packages it does not
need for this function (torch_sparse, google_drive_downloader); where they are missing an empty stand-in is registered."""
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rocauc_ref as R  # noqa: E402


def reference_eval_rocauc(path):
    for name, attr in (("torch_sparse", "SparseTensor"), ("google_drive_downloader", "GoogleDriveDownloader")):
        try:
            importlib.import_module(name)
        except ImportError:
            mod = types.ModuleType(name)
            setattr(mod, attr, type(attr, (), {}))
            sys.modules[name] = mod
    sys.path.insert(0, path)
    return importlib.import_module("data_utils").eval_rocauc


def cases():
    rng = np.random.default_rng(7)
    out = {}
    # the tie-exact grid with the +/- 20..32 rows; five distinct scores; a third column far below (its exp adds nothing to a
    # sum >= 1); labels -1 outside the sets.  All on the grid: their order and ties are the same on any device.
    for tag, n, logits in (("grid", 1500, R.grid_logits(1500, 1)), ("fivelevels", 2000, R.grid_logits(2000, 2, False, levels=5)),
                           ("c3", 1200, np.concatenate([R.grid_logits(1200, 4), np.full((1200, 1), -120.0, np.float32)], 1)),
                           ("unlabeled", 900, R.grid_logits(900, 3))):
        y = rng.integers(0, 2, n).astype(np.int64)
        order = rng.permutation(n)
        used = n if tag != "unlabeled" else 600
        if tag == "unlabeled":
            y[order[used:]] = -1
        a, b = used // 2, used // 2 + used // 4
        out[tag] = (logits, y, [np.sort(order[:a]), np.sort(order[a:b]), np.sort(order[b:used])])
    return out


def main(ref_path):
    eval_rocauc = reference_eval_rocauc(ref_path)
    rec = {}
    for tag, (logits, y, sets) in cases().items():
        z, lab = torch.from_numpy(logits), torch.from_numpy(y).view(-1, 1)
        scores = R.cpu_scores(z)
        vals, triples = [], []
        for idx in sets:
            i = torch.from_numpy(idx)
            v = float(eval_rocauc(lab[i], z[i]))
            t = R.triple(scores, y, idx)
            assert abs(v - R.auc_of(t)) <= 1e-12, (tag, v, t)
            vals.append(v)
            triples.append(t)
        rec[f"{tag}:logits"], rec[f"{tag}:labels"] = logits, y
        for k, idx in enumerate(sets):
            rec[f"{tag}:set{k}"] = idx.astype(np.int64)
        rec[f"{tag}:reference"] = np.asarray(vals, np.float64)
        rec[f"{tag}:triples"] = np.asarray(triples, np.int64)
        print(tag, vals, triples)
    path = os.path.join(HERE, "rocauc_cases.npz")
    np.savez_compressed(path, **rec)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main(sys.argv[1])
