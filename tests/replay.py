"""Deterministic dropout masks shared by the golden generator (which patches them into the
reference) and the GPU accuracy test (which patches them into this package): the same CPU
generator stream on both sides, so two implementations train on identical masks."""
import numpy as np
import torch


def degree_order(degree):
    """The node numbering graph.relabel_by_degree gives the library's operators, computed on the host: ``perm`` = the nodes by
    decreasing degree (ties by id: a stable sort), ``inv[i]`` = the row node i gets.  The library draws its dropout masks by
    that row, so the masks handed to the reference for node i are those of row inv[i] (PhiloxDropout rows=)."""
    degree = np.asarray(degree, dtype=np.int64)
    perm = np.argsort(-degree, kind="stable")
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    return perm, inv


def load_twitch_syn(path):
    """tests/golden/graph_twitch_syn.npz (make_accuracy_golden.make_twitch_syn) -> (n, symmetric scipy adjacency, raw features
    float32 [n, 7], labels int64, [(train, val, test) boolean masks per split])."""
    import scipy.sparse as sp
    with np.load(path, allow_pickle=False) as f:
        g = {k: f[k] for k in f.files}
    n = int(g["n"])
    rows = np.repeat(np.arange(n), g["tri_count"].astype(np.int64))
    cols = g["tri_cols"].astype(np.int64)
    a = sp.coo_matrix((np.ones(len(rows), np.float32), (rows, cols)), shape=(n, n)).tocsr()
    a = (a + a.T).tocsr()
    a.sort_indices()
    x = g["feat_codes"].astype(np.float32) * np.float32(g["feat_scale"])
    labels = np.unpackbits(g["labels_bits"])[:n].astype(np.int64)
    masks = [tuple(np.unpackbits(g[f"{k}_mask_{s}"])[:n].astype(bool) for k in ("train", "val", "test"))
             for s in range(int(g["n_splits"]))]
    return n, a, x, labels, masks


class SeededDropout:
    """Drop-in for torch.nn.functional.dropout.  Mask k of epoch e comes from a CPU generator
    seeded with (seed, e, k); call .next_epoch() once per training step."""

    def __init__(self, seed, device="cpu"):
        self.seed, self.epoch, self.site, self.device = int(seed), 0, 0, device

    def next_epoch(self):
        self.epoch += 1
        self.site = 0

    def __call__(self, inp, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return inp
        g = torch.Generator().manual_seed(self.seed * 1_000_003 + self.epoch * 101 + self.site)
        self.site += 1
        keep = torch.bernoulli(torch.full(tuple(inp.shape), 1.0 - p), generator=g).to(inp.device)
        return inp * keep / (1.0 - p)


class PhiloxDropout:
    """Drop-in for torch.nn.functional.dropout that hands the REFERENCE the masks this library's kernels draw themselves
    (counter-based dropout: oracle/philox.py restates csrc/acm_common.h) -- so a reference run can be recorded that the
    fused small-graph step (acm_small_step: masks generated inside the kernels, never materialised) replays exactly.

    Two-layer acmgcn / acmgcnp models call F.dropout twice per training forward (ACM-Pytorch/models/models.py:116,160):
    site 0 = the input features (tag 0; the library keys the mask of a CSR feature matrix by the position of the entry in
    the row-major sorted nonzero list, column 0), site 1 = the hidden activations [n, 64] (tag 1, keyed by (row, column)).
    Step counter: 0 for the first optimizer step; call .next_epoch() before every training step.

    ``dense=True``: the input is a dense real-valued matrix that the library keeps dense (the narrow first layer of the
    ACM-Geometric headline configuration): site 0 is keyed by (row, column) with tag 0, like site 1 with tag 1.
    ``rows``: the mask row of every node, for both sites -- the library draws its masks in the numbering its operators work
    in, so with degree-relabelled operators (graph.relabel_by_degree) node i of the reference takes the mask of row
    rows[i] = inv_perm[i] (oracle.philox.dropout_factors(rows=...)); None: row i."""

    def __init__(self, seed, features, dense=False, rows=None):
        from oracle.philox import dropout_factors
        self._factors = dropout_factors
        self.seed, self.step, self.site = int(seed), -1, 0
        self.dense = bool(dense)
        self.rows = None if rows is None else np.asarray(rows, dtype=np.int64)
        self._shape = tuple(features.shape)
        if self.rows is not None:
            assert self.dense, "mask rows apply to (row, column)-keyed sites: a CSR input is keyed by nonzero position"
            assert self.rows.shape == (self._shape[0],)
        if not self.dense:
            nz = torch.nonzero(features)                # row-major sorted, like the coalesced COO behind SparseFeatures.auto
            self._flat = nz[:, 0] * features.shape[1] + nz[:, 1]

    def next_epoch(self):
        self.step += 1
        self.site = 0

    def __call__(self, inp, p=0.5, training=True, inplace=False):
        if not training or p == 0.0:
            return inp
        site, self.site = self.site, self.site + 1
        if site == 0:
            assert tuple(inp.shape) == self._shape, "site 0 is the input feature matrix"
            if self.dense:
                f = self._factors(self.seed, self.step, 0, p, inp.shape[0], inp.shape[1], rows=self.rows)
                return inp * torch.from_numpy(f).to(inp.dtype).to(inp.device)
            f = self._factors(self.seed, self.step, 0, p, self._flat.numel(), 1)[:, 0]
            m = torch.zeros(inp.numel(), dtype=inp.dtype)
            m[self._flat] = torch.from_numpy(f).to(inp.dtype)
            return inp * m.view(inp.shape).to(inp.device)
        assert site == 1, "two dropout sites per forward (acmgcn / acmgcnp)"
        assert self.rows is None or inp.shape[0] == len(self.rows)
        f = self._factors(self.seed, self.step, 1, p, inp.shape[0], inp.shape[1], rows=self.rows)
        return inp * torch.from_numpy(f).to(inp.dtype).to(inp.device)
