"""The synthetic study's graphs and features (``synthetic-experiments/graph_generation.py`` / ``feature_generation.py``) written
as CSR on the device, at any size: nothing dense, nothing on the host.

    from acm_gnn_amd import synthetic as S, homophily as H
    g = S.generate_graph("random", n_classes=5, nodes_per_class=400, degree_intra=2, edge_homo=0.3, seed=0, graph_index=0)
    g.adj, g.labels, g.degree, g.block_counts     # pattern-only CsrGraph (no self loops), int64 labels, degrees, C x C counts
    ops = g.operators()                            # D^-1 (I + A), as synthetic-experiments/train.py:72-78
    x = S.random_features(g.n, 1433, seed=0)       # or S.generate_base_features(base_x, base_y, ...)
    H.census(g.adj, g.labels).edge                 # ~ edge_homo

Every graph is a pure function of its arguments (the sampling contract is stated in ``include/acm_hip.h``): the same
``(seed, graph_index)`` gives the same bits on any device, and ``rows=(b, e)`` regenerates exactly those rows of a ``regular``
graph.  ``torch.sort`` is the only torch primitive on the path (the stable sort the first-M-distinct selection needs and the
final CSR ordering), as in ``filters_from_edge_index``."""
import ctypes as C
import math

import torch

from . import _lib
from .graph import CsrGraph, _require_cuda, filters_from_edge_index

MAX_CLASSES = 64
MAX_DEGREE = 256                 # ACM_SYNTH_MAX_DEGREE
PAIR, RECT, RANGE = 0, 1, 2      # ACM_SYNTH_*
SHORT, OVER = 1, 2
MAX_ATTEMPTS = 8                 # stream extensions (each doubles the stream) before giving up
_INVALID = torch.iinfo(torch.int64).max


def _launch(name, dev, *args):
    from .functional._launch import launch
    return launch(name, name[4:], dev, *args)


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _device(device):
    dev = torch.device(device)
    if dev.type != "cuda":
        raise RuntimeError(f"acm_gnn_amd: device is {dev}; the ACM operators run only on an AMD GPU (there is no CPU fallback)")
    return torch.device("cuda", torch.cuda.current_device()) if dev.index is None else dev


def _check_shape(who, n_classes, nodes_per_class, seed, graph_index):
    c, npc = int(n_classes), int(nodes_per_class)
    if not 2 <= c <= MAX_CLASSES:
        raise ValueError(f"{who}: {c} classes (2..{MAX_CLASSES})")
    if npc < 1 or c * npc >= 2 ** 31 - 1:
        raise ValueError(f"{who}: nodes_per_class = {npc} (at least 1, fewer than 2^31 nodes in all)")
    if not 0 <= int(seed) < 2 ** 64 or not 0 <= int(graph_index) < 2 ** 64:
        raise ValueError(f"{who}: seed and graph_index must fit 64 unsigned bits")
    return c, npc


def stream_draws(m, n_keys, valid=1.0):
    """A stream length that holds ``m`` distinct of ``n_keys`` equally likely keys with room to spare (coupon collector's
    expectation x 1.2 + 64; ``valid``: the share of draws that decode to a key)."""
    m = min(int(m), int(n_keys))
    if m <= 0:
        return 64
    expect = n_keys * (math.log(n_keys) - math.log(n_keys - m)) if m < n_keys else n_keys * (math.log(n_keys) + 1.0)
    return int(1.2 * expect / valid) + 64


# ---- the first M distinct keys of a stream -----------------------------------------------------------------------------------
def select_distinct(keys, m, out_cap, status=None):
    """The first ``m[g]`` distinct valid keys of every row of ``keys`` (int64 ``[G, T]`` on the GPU, INT64_MAX = invalid), in
    draw order: (out int64 ``[G, out_cap]``, found int64 ``[G]``, status int32 ``[1]``).  ``m``: int64 ``[G]`` on the device.
    Only ``out[g, :found[g]]`` is written.  status bit 1: a row held fewer than m distinct keys; bit 2: m > out_cap."""
    if not isinstance(keys, torch.Tensor) or keys.dim() != 2 or keys.dtype != torch.int64 or not keys.is_contiguous():
        raise ValueError("select_distinct: keys must be a contiguous int64 [G, T] tensor")
    _require_cuda(keys, "keys")
    g, t = keys.shape
    if not isinstance(m, torch.Tensor) or m.dtype != torch.int64 or m.shape != (g,) or not m.is_contiguous() or m.device != keys.device:
        raise ValueError("select_distinct: m must be a contiguous int64 [G] tensor on the keys' device")
    out_cap = int(out_cap)
    if g < 1 or t < 1 or out_cap < 0:
        raise ValueError("select_distinct: at least one row, one draw and out_cap >= 0 are needed")
    dev = keys.device
    sorted_keys, perm = torch.sort(keys, dim=1, stable=True)            # equal keys keep their draw order
    out = torch.empty(g, max(out_cap, 1), dtype=torch.int64, device=dev)
    found = torch.empty(g, dtype=torch.int64, device=dev)
    if status is None:
        status = torch.zeros(1, dtype=torch.int32, device=dev)
    nbytes = C.c_size_t()
    _lib.check(_lib.load().acm_synth_select_workspace_bytes(g, t, C.byref(nbytes)), "acm_synth_select_workspace_bytes")
    ws = torch.empty(nbytes.value // 8 + 1, dtype=torch.int64, device=dev)
    _launch("acm_synth_select", dev, g, t, _vp(keys), _vp(sorted_keys), _vp(perm), _vp(m), out_cap, _vp(out), _vp(found), _vp(status),
            _vp(ws), ws.numel() * 8)
    return out[:, :out_cap], found, status


def draw_keys(kind, a, b, block_first, n_segments, seed, graph_index, n_draws, device="cuda"):
    """int64 ``[n_segments, n_draws]`` keys of the streams ``block_first ..`` (``acm_synth_draw``)."""
    dev = _device(device)
    keys = torch.empty(int(n_segments), int(n_draws), dtype=torch.int64, device=dev)
    _launch("acm_synth_draw", dev, int(kind), int(a), int(b), int(block_first), int(n_segments), int(seed), int(graph_index), int(n_draws),
            C.c_void_p(keys.data_ptr()))
    return keys


# ---- graphs ------------------------------------------------------------------------------------------------------------------
class SyntheticGraph:
    """A generated graph: ``adj`` (pattern-only CsrGraph, no self loops), ``labels`` int64 ``[n]`` (all n nodes), ``degree`` int64
    per generated row, ``block_counts`` int64 ``[C, C]`` (entries from the rows' classes to the columns' classes; the whole
    graph's, or the slice's), ``indptr`` / ``indices`` int32 device tensors, ``rows`` = the generated row range.  For a row slice
    ``indptr`` is slice-local (``rows[1] - rows[0] + 1`` entries starting at 0), the column ids stay global, and ``adj`` /
    ``operators()`` are refused: they stand for the whole graph."""

    def __init__(self, kind, n_classes, nodes_per_class, indptr, indices, block_counts, rows, info):
        self.kind, self.n_classes, self.nodes_per_class = kind, n_classes, nodes_per_class
        self.n = n_classes * nodes_per_class
        self.indptr, self.indices, self._blocks, self.rows, self.info = indptr, indices, block_counts, rows, info
        self._adj = None

    @property
    def device(self):
        return self.indptr.device

    @property
    def block_counts(self):
        if self._blocks is None:                 # (regular: counted on first use, the generator itself writes the ids only)
            c, npc = self.n_classes, self.nodes_per_class
            row_class = torch.arange(self.rows[0], self.rows[1], device=self.device, dtype=torch.int64) // npc
            cell = torch.repeat_interleave(row_class, self.degree) * c + self.indices.to(torch.int64) // npc
            self._blocks = torch.bincount(cell, minlength=c * c).reshape(c, c)
        return self._blocks

    @property
    def adj(self):
        if self.rows != (0, self.n):
            raise ValueError("adj: a row slice is no operator of the whole graph (indptr is slice-local); generate the whole graph")
        if self._adj is None:
            self._adj = CsrGraph.from_csr(self.indptr, self.indices, None, self.n)
        return self._adj

    @property
    def labels(self):
        return torch.arange(self.n, device=self.device, dtype=torch.int64) // self.nodes_per_class

    @property
    def degree(self):
        return (self.indptr[1:] - self.indptr[:-1]).to(torch.int64)

    @property
    def edge_index(self):
        """int64 ``[2, nnz]``: (row, column) of every stored entry."""
        rows = torch.repeat_interleave(torch.arange(self.rows[0], self.rows[1], device=self.device, dtype=torch.int64), self.degree)
        return torch.stack([rows, self.indices.to(torch.int64)])

    def operators(self, chunk=0):
        """FilterOperators of D^-1 (I + A) (synthetic-experiments/train.py:72-78); the entries are taken as stored, a
        ``regular`` graph stays directed."""
        if self.rows != (0, self.n):
            raise ValueError("operators: a row slice is no square operator; generate the whole graph")
        return filters_from_edge_index(self.edge_index, self.n, undirected=False, chunk=chunk)


def generate_graph(graph_type, n_classes=5, nodes_per_class=400, degree_intra=2, edge_homo=0.5, seed=0, graph_index=0, device="cuda",
                   rows=None, stream_length=None):
    """One graph of ``graph_generation.py`` with the block size read as ``nodes_per_class`` -> :class:`SyntheticGraph`.

    ``regular``: every row takes ``degree_intra`` nodes of its own class and ``int(degree_intra / h - degree_intra)`` nodes of
    the others (directed, one launch; ``rows=(b, e)`` generates that slice).  ``random``: every class receives
    ``degree_intra * nodes_per_class / 2`` undirected intra-class edges, then class by class ``round(T - e_i) + 1`` edges
    toward the later classes, ``T = S (1 - h) / h``.  ``stream_length``: the first length of the random type's key streams
    (default: :func:`stream_draws`); a stream that turns out short is extended, which does not change the result."""
    if graph_type not in ("regular", "random"):
        raise ValueError(f"generate_graph: graph_type {graph_type!r} ('regular' or 'random')")
    c, npc = _check_shape("generate_graph", n_classes, nodes_per_class, seed, graph_index)
    degree_intra, edge_homo = int(degree_intra), float(edge_homo)
    if degree_intra < 0 or not 0.0 < edge_homo <= 1.0:
        raise ValueError(f"generate_graph: degree_intra = {degree_intra} (>= 0), edge_homo = {edge_homo} (in (0, 1]) ")
    if graph_type == "regular":
        return _regular(c, npc, degree_intra, edge_homo, int(seed), int(graph_index), device, rows)
    if rows is not None:
        raise ValueError("generate_graph: rows= is for the regular type (a random graph's rows depend on each other)")
    if degree_intra > npc - 1 or (degree_intra * npc) % 2:
        raise ValueError(f"generate_graph: degree_intra * nodes_per_class = {degree_intra * npc} must be even and degree_intra at most "
                         f"{npc - 1}")
    return _random(c, npc, degree_intra, edge_homo, int(seed), int(graph_index), _device(device), stream_length)


def _regular(c, npc, degree_intra, edge_homo, seed, graph_index, device, rows):
    n = c * npc
    degree_inter = int(degree_intra / edge_homo - degree_intra)          # graph_generation.py:25, exactly
    b, e = (0, n) if rows is None else (int(rows[0]), int(rows[1]))
    if not 0 <= b <= e <= n:
        raise ValueError(f"generate_graph: rows [{b}, {e}) of {n}")
    if degree_intra > npc - 1 or degree_inter > n - npc:
        raise ValueError(f"generate_graph: degrees {degree_intra} / {degree_inter} exceed the {npc - 1} / {n - npc} nodes to choose from")
    d = degree_intra + degree_inter
    if d > MAX_DEGREE or (e - b) * d >= 2 ** 31 - 1:
        raise ValueError(f"generate_graph: degree {d} (at most {MAX_DEGREE}) and {(e - b) * d} entries (fewer than 2^31)")
    dev = _device(device)
    indices = torch.empty((e - b) * d, dtype=torch.int32, device=dev)
    if indices.numel():
        _launch("acm_synth_regular", dev, c, npc, degree_intra, degree_inter, seed, graph_index, b, e, C.c_void_p(indices.data_ptr()))
    indptr = torch.arange(0, (e - b) * d + 1, max(d, 1), dtype=torch.int32, device=dev) if d else torch.zeros(e - b + 1, dtype=torch.int32, device=dev)
    return SyntheticGraph("regular", c, npc, indptr, indices, None, (b, e), dict(degree_inter=degree_inter, degree=d))


def _random(c, npc, degree_intra, edge_homo, seed, graph_index, dev, stream_length):
    n = c * npc
    plan = (C.c_int64 * 2)()
    _lib.check(_lib.load().acm_synth_random_plan(c, npc, degree_intra, edge_homo, plan), "acm_synth_random_plan")
    half, cap = int(plan[0]), int(plan[1])
    t_edges = degree_intra * npc * (1 - edge_homo) / edge_homo           # graph_generation.py:98, float64 on the host
    pairs = npc * (npc - 1) // 2
    widths = [(c - 1 - i) * npc for i in range(c - 1)]
    t_intra = stream_draws(half, pairs, 1.0 - 1.0 / npc) if stream_length is None else max(int(stream_length), 1)
    t_inter = [stream_draws(cap, npc * w) if stream_length is None else max(int(stream_length), 1) for w in widths]
    for attempt in range(MAX_ATTEMPTS):
        # state: block counts C x C | m of the C - 1 chained classes | found (C intra, C - 1 inter) | status
        state = torch.zeros(c * c + 3 * c, dtype=torch.int64, device=dev)
        blocks, m_inter = state[:c * c], state[c * c:c * c + c - 1]
        status = state[-1:].view(torch.int32)[:1]
        edges = torch.empty(2 * (c * half + (c - 1) * cap), dtype=torch.int64, device=dev)
        if half:
            keys = draw_keys(PAIR, npc, 1, 0, c, seed, graph_index, t_intra, dev)
            sel, found, _ = select_distinct(keys, torch.full((c,), half, dtype=torch.int64, device=dev), half, status)
            state[c * c + c:c * c + 2 * c] = found
            _launch("acm_synth_emit", dev, PAIR, c, npc, 0, c, _vp(sel), _vp(found), half, _vp(edges), _vp(blocks))
        for i, w in enumerate(widths):                                   # class i reads what classes < i placed: stream order
            _launch("acm_synth_inter_count", dev, c, i, t_edges, _vp(blocks), C.c_void_p(m_inter.data_ptr() + 8 * i))
            keys = draw_keys(RECT, npc, w, i, 1, seed, graph_index, t_inter[i], dev)
            sel, found, _ = select_distinct(keys, m_inter[i:i + 1], cap, status)
            state[c * c + 2 * c + i] = found[0]
            _launch("acm_synth_emit", dev, RECT, c, npc, i, 1, _vp(sel), _vp(found), cap,
                    C.c_void_p(edges.data_ptr() + 16 * (c * half + i * cap)), _vp(blocks))
        host = state.cpu()                                               # the one host read: counts, m, found, status
        if not int(host[-1:].view(torch.int32)[0]) & SHORT:
            break
        m_host = host[c * c:c * c + c - 1].tolist()
        f_host = host[c * c + 2 * c:c * c + 3 * c - 1].tolist()
        intra_done = not half or int(host[c * c + c:c * c + 2 * c].min()) >= half
        short = next((i for i in range(c - 1) if f_host[i] < m_host[i]), None)
        # the first short class's m is final (everything before it is complete): more edges than slots never fills
        if intra_done and short is not None and m_host[short] > npc * widths[short]:
            raise ValueError(f"generate_graph: class {short} needs {m_host[short]} inter-class edges and has {npc * widths[short]} slots")
        t_intra, t_inter = 2 * t_intra, [2 * t for t in t_inter]
    else:
        raise RuntimeError(f"generate_graph: a key stream stayed short after {MAX_ATTEMPTS} extensions")
    # a retry regenerates the whole chain, complete intra blocks included: it is rare (the default lengths hold 1.2 x the
    # expected draws) and keeps one code path; the final sort runs once, after the status is known
    nnz = int(host[:c * c].sum())
    ordered = torch.sort(edges).values[:nnz]                             # row * n + col ascending; the unused tail is INT64_MAX
    rows, cols = ordered // n, ordered % n
    indptr = torch.zeros(n + 1, dtype=torch.int64, device=dev)
    indptr[1:] = torch.cumsum(torch.bincount(rows, minlength=n), 0)
    info = dict(t_edges=t_edges, m=host[c * c:c * c + c - 1].tolist(), found=host[c * c + 2 * c:c * c + 3 * c - 1].tolist(), attempts=attempt + 1, stream_lengths=(t_intra, t_inter))
    return SyntheticGraph("random", c, npc, indptr.to(torch.int32), cols.to(torch.int32), state[:c * c].reshape(c, c).clone(), (0, n), info)


# ---- features ----------------------------------------------------------------------------------------------------------------
def random_features(n, n_features=1433, seed=0, graph_index=0, device="cuda", row_begin=0):
    """fp32 ``[n, n_features]`` uniform in [0, 1) (feature_generation.py:33), a pure function of (seed, graph_index, row,
    column): rows ``row_begin ..`` of the matrix any other range would give."""
    n, f = int(n), int(n_features)
    if n < 0 or f < 1 or int(row_begin) < 0:
        raise ValueError(f"random_features: {n} x {f} from row {row_begin}")
    if not 0 <= int(seed) < 2 ** 64 or not 0 <= int(graph_index) < 2 ** 64:
        raise ValueError("random_features: seed and graph_index must fit 64 unsigned bits")
    dev = _device(device)
    out = torch.empty(n, f, dtype=torch.float32, device=dev)
    if n:
            _launch("acm_synth_uniform", dev, n, f, int(seed), int(graph_index), int(row_begin), C.c_void_p(out.data_ptr()), f)
    return out


# ---- the study's split -------------------------------------------------------------------------------------------------------
_SPLIT_STREAM = 1 << 63          # graph_index of the split keys: the feature draws of the same seed use graph_index < 2^63


def disassortative_splits(labels, n_classes, seed, split_index=0):
    """The study's 60 / 20 / 20 split (synthetic-experiments/utils.py:440-461, ``random_disassortative_splits``) ->
    (train, val, test): three sorted int64 index tensors on the labels' device.

    Per class ``int(round(0.6 * n / C))`` training nodes (Python's ``round``, as there; a class with fewer members gives all of
    them); of the shuffled rest ``int(round(0.2 * n))`` validation nodes, the remainder is the test set.  Nodes whose label
    lies outside [0, C) are in no set, as in the reference.  The shuffles are a pure function of ``(seed, split_index)``: node i
    carries the two uniform keys ``acm_synth_uniform`` draws for row i under graph_index = 2^63 + split_index, a class's members
    (and the rest) are ordered by key with ``torch.sort`` (stable: equal keys keep the ascending node order).  The reference
    shuffles with ``torch.randperm`` on the unseeded global generator; that stream is NOT reproduced -- the split has its
    sizes and its per-class shares, not its members."""
    if not isinstance(labels, torch.Tensor) or labels.dim() != 1 or labels.dtype != torch.int64:
        raise ValueError("disassortative_splits: labels must be an int64 [n] tensor")
    _require_cuda(labels, "labels")
    c, n = int(n_classes), labels.numel()
    if c < 1 or not 0 <= int(seed) < 2 ** 64 or not 0 <= int(split_index) < _SPLIT_STREAM:
        raise ValueError(f"disassortative_splits: {c} classes, seed {seed}, split_index {split_index}")
    per_class, n_val = int(round(0.6 * (n / c))), int(round(0.2 * n))
    dev = labels.device
    keys = random_features(n, 2, seed=seed, graph_index=_SPLIT_STREAM + int(split_index), device=dev) if n else labels.new_zeros(0, 2, dtype=torch.float32)
    nodes = ((labels >= 0) & (labels < c)).nonzero().view(-1)
    lab = labels.index_select(0, nodes)
    by_key = torch.sort(keys[:, 0].index_select(0, nodes), stable=True).indices
    by_class = torch.sort(lab.index_select(0, by_key), stable=True).indices
    order = by_key.index_select(0, by_class)                             # grouped by class, shuffled inside
    lab_sorted = lab.index_select(0, order)
    first = torch.cumsum(torch.bincount(lab, minlength=c), 0) - torch.bincount(lab, minlength=c)
    rank = torch.arange(order.numel(), device=dev) - first.index_select(0, lab_sorted)
    shuffled = nodes.index_select(0, order)
    train = shuffled[rank < per_class]
    rest = shuffled[rank >= per_class]
    rest = rest.index_select(0, torch.sort(keys[:, 1].index_select(0, rest), stable=True).indices)
    return tuple(torch.sort(t).values for t in (train, rest[:n_val], rest[n_val:]))


def base_feature_rows(base_y, n_classes=5, nodes_per_class=400, seed=0, graph_index=0):
    """int64 ``[n_classes * nodes_per_class]`` rows of a base data set (feature_generation.py:36-54): class j draws from base
    class ``j % n_base``; with more than ``nodes_per_class`` members it takes that many without replacement, otherwise every
    member plus ``nodes_per_class - count`` further members without replacement (ValueError where numpy's ``choice`` raises).
    The choice is the first-k-distinct selection over the class's ascending member list, in draw order."""
    c, npc = _check_shape("generate_base_features", n_classes, nodes_per_class, seed, graph_index)
    if not isinstance(base_y, torch.Tensor) or base_y.dim() != 1 or base_y.dtype != torch.int64 or base_y.numel() == 0:
        raise ValueError("generate_base_features: base_y must be a non-empty int64 [n] tensor")
    _require_cuda(base_y, "base_y")
    dev = base_y.device
    # host reads: the class sizes here, then one status word per attempt.  The classes' streams have their own ranges (the
    # class sizes), so every class is its own draw / sort / select chain of one segment
    counts = torch.bincount(base_y[base_y >= 0]).tolist()
    n_base = len(counts)
    order = torch.argsort(base_y, stable=True)                            # members of a class, ascending, behind the negative labels
    first = [base_y.numel() - sum(counts)]
    for k in counts:
        first.append(first[-1] + k)
    members, wants = [], []
    for j in range(c):
        count = counts[j % n_base]
        m = npc if count > npc else npc - count
        if m > count:
            raise ValueError(f"generate_base_features: class {j} needs {m} further rows of base class {j % n_base}, which has {count} "
                             "(cannot take a larger sample than the population without replacement)")
        members.append(order[first[j % n_base]:first[j % n_base + 1]])
        wants.append(m)
    lengths = [stream_draws(m, max(counts[j % n_base], 1)) for j, m in enumerate(wants)]
    for _ in range(MAX_ATTEMPTS):
        status = torch.zeros(1, dtype=torch.int32, device=dev)
        picks = []
        for j, m in enumerate(wants):
            if m == 0:
                picks.append(None)
                continue
            keys = draw_keys(RANGE, counts[j % n_base], 1, j, 1, seed, graph_index, lengths[j], dev)
            picks.append(select_distinct(keys, torch.full((1,), m, dtype=torch.int64, device=dev), m, status)[0][0])
        if not int(status.cpu()[0]) & SHORT:
            break
        lengths = [2 * t for t in lengths]
    else:
        raise RuntimeError(f"generate_base_features: a key stream stayed short after {MAX_ATTEMPTS} extensions")
    out = []
    for j in range(c):
        if counts[j % n_base] <= npc:
            out.append(members[j])
        if picks[j] is not None:
            out.append(members[j][picks[j]])
    return torch.cat(out)


def generate_base_features(base_x, base_y, n_classes=5, nodes_per_class=400, seed=0, graph_index=0):
    """``base_x[rows]`` for the rows of :func:`base_feature_rows` (the gather is ``index_select``)."""
    if not isinstance(base_x, torch.Tensor) or base_x.dim() != 2:
        raise ValueError("generate_base_features: base_x must be a [n, F] tensor")
    if not isinstance(base_y, torch.Tensor) or base_y.shape[:1] != base_x.shape[:1]:
        raise ValueError("generate_base_features: one label per row of base_x is needed")
    _require_cuda(base_x, "base_x")
    rows = base_feature_rows(base_y, n_classes, nodes_per_class, seed, graph_index)
    return base_x.index_select(0, rows.to(base_x.device))
