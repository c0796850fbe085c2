"""The five graph measures of the reference's ``synthetic-experiments/homophily.py`` on the device, at any graph size.

The reference forms dense ``n x n`` matrices (``label @ label.T``, ``A.nonzero()``, ``(A X)(A X)^T``).  Here the four label
measures are ONE pass over the stored CSR pattern with a byte-label gather -- the *census* (``acm_homophily_census``) -- and
aggregation homophily is one SpMM, a per-class column mean and an ``n x F x C`` product with an arg-max (``acm_class_means``,
``acm_class_score``).  The rule of the census is stated in ``include/acm_hip.h``; in short: values are ignored, every stored
entry ``(i, j)`` counts once iff ``j != i`` and both ends are labeled (a negative label means "unlabeled").

    from acm_gnn_amd import homophily as H
    c = H.census(adj, labels)                    # three launches, exact integers on the device
    c.edge, c.node, c.klass, c.compat            # float64, after ONE host read
    H.aggregation_homophily(x, adj_low, labels)  # hits / n_labeled

The module functions carry the reference's names and argument order.
"""
import ctypes as C

import numpy as np
import torch

from . import _lib
from .graph import CsrGraph, FilterOperators, _require_cuda

MAX_CLASSES = 64
SCORE_MAX_FEATURES = 256


# ---- operands -----------------------------------------------------------------------------------------------------
def _graph_of(adj, who):
    """CsrGraph of ``adj`` (a CsrGraph, the ``low`` pattern of a FilterOperators, or a sparse / dense torch adjacency)."""
    if isinstance(adj, FilterOperators):
        if adj.sharded:
            raise NotImplementedError(f"{who}: row-sharded operators are not supported (the class means and the counts need a "
                                      "reduction over ranks)")
        return adj.low
    if isinstance(adj, CsrGraph):
        return adj
    if isinstance(adj, torch.Tensor):
        if adj.dim() != 2:
            raise ValueError(f"{who}: the adjacency must be a matrix, got {adj.dim()} dimensions")
        _require_cuda(adj, "adjacency")
        return CsrGraph.from_torch(adj)
    raise TypeError(f"{who}: unsupported adjacency {type(adj).__name__}")


def _labels_of(labels, n_classes, who):
    """(contiguous int64 [n] labels, C) from an index vector or a one-hot matrix (an all-zero row is unlabeled)."""
    if not isinstance(labels, torch.Tensor):
        raise TypeError(f"{who}: labels must be a torch tensor")
    if labels.dim() == 2 and labels.shape[1] == 1:
        labels = labels[:, 0]
    if labels.dim() == 2:
        width = labels.shape[1]
        y = torch.where(labels.sum(1) > 0, labels.argmax(1), torch.full((labels.shape[0],), -1, dtype=torch.int64, device=labels.device))
        if n_classes is None:
            n_classes = width
    elif labels.dim() == 1:
        if labels.dtype != torch.int64:
            raise ValueError(f"{who}: an index vector of labels must be int64, got {labels.dtype}")
        y = labels
        if n_classes is None:
            n_classes = int(labels.max()) + 1 if labels.numel() else 0
    else:
        raise ValueError(f"{who}: labels must be an int64 [n] vector or a one-hot [n, C] matrix")
    n_classes = int(n_classes)
    if not 2 <= n_classes <= MAX_CLASSES:
        raise ValueError(f"{who}: {n_classes} classes (2..{MAX_CLASSES})")
    return y.contiguous(), n_classes


def _launch(name, dev, *args):
    from .functional._launch import launch
    return launch(name, name[4:], dev, *args)


def _query(name, *args):
    nbytes = C.c_size_t()
    _lib.check(getattr(_lib.load(), name)(*args, C.byref(nbytes)), name)
    return nbytes.value


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


# ---- the census ---------------------------------------------------------------------------------------------------
class HomophilyCensus:
    """The integer census of a labeled pattern and the four measures it determines.

    Device tensors (``None`` when built by :meth:`from_counts`): ``counts`` int64 ``[C*C + 2C + 2]`` = ``M | cls | iso |
    n_labeled | n_deg``, ``row_same`` / ``row_deg`` int32 ``[n_rows]``, ``node_sum`` float64 ``[1]``.  ``edge``, ``node``,
    ``klass`` and ``compat`` are formed in float64 after one host read."""

    def __init__(self, n_classes, buf=None, row_same=None, row_deg=None, workspace=None):
        self.n_classes = int(n_classes)
        self._buf = buf                       # int64 [C*C + 2C + 3]: the counts, then the bits of node_sum
        self.row_same, self.row_deg = row_same, row_deg
        self._ws = workspace
        self._host = None

    @property
    def counts(self):
        return None if self._buf is None else self._buf[:-1]

    @property
    def node_sum(self):
        return None if self._buf is None else self._buf[-1:].view(torch.float64)

    @classmethod
    def from_counts(cls, M, cls_count, iso, n_labeled, n_deg, node_sum):
        """From host arrays: the finishing arithmetic without a device."""
        M = np.asarray(M, dtype=np.int64)
        if M.ndim != 2 or M.shape[0] != M.shape[1] or not 2 <= M.shape[0] <= MAX_CLASSES:
            raise ValueError("HomophilyCensus.from_counts: M must be a C x C matrix, 2 <= C <= 64")
        c = M.shape[0]
        cls_count, iso = np.asarray(cls_count, dtype=np.int64), np.asarray(iso, dtype=np.int64)
        if cls_count.shape != (c,) or iso.shape != (c,):
            raise ValueError("HomophilyCensus.from_counts: cls and iso must have C entries")
        out = cls(c)
        out._host = (M, cls_count, iso, int(n_labeled), int(n_deg), float(node_sum))
        return out

    def host(self):
        """(M, cls, iso, n_labeled, n_deg, node_sum) on the host -- the one read."""
        if self._host is None:
            c = self.n_classes
            raw = self._buf.cpu().numpy()
            self._host = (raw[:c * c].reshape(c, c).copy(), raw[c * c:c * c + c].copy(), raw[c * c + c:c * c + 2 * c].copy(),
                          int(raw[c * c + 2 * c]), int(raw[c * c + 2 * c + 1]), float(raw[-1:].view(np.float64)[0]))
        return self._host

    def invalidate(self):
        """Forget the host copy (the device buffers were written again)."""
        if self._buf is not None:
            self._host = None

    @property
    def edge(self):
        m = self.host()[0]
        total = int(m.sum())
        return float(np.trace(m)) / total if total else float("nan")

    @property
    def node(self):
        _, _, _, _, n_deg, node_sum = self.host()
        return node_sum / n_deg if n_deg else float("nan")

    @property
    def compat(self):
        m = self.host()[0].astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            return m / m.sum(1, keepdims=True)

    @property
    def klass(self):
        m, cls_count, iso, n_labeled, _, _ = self.host()
        c = self.n_classes
        h = (m + np.diag(iso)).astype(np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            h = h / h.sum(1, keepdims=True)
            p = cls_count.astype(np.float64) / float(n_labeled) if n_labeled else np.full(c, np.nan)
        val = 0.0
        for k in range(c):
            term = max(h[k, k] - p[k], 0.0) if not (np.isnan(h[k, k]) or np.isnan(p[k])) else float("nan")
            if not np.isnan(term):
                val += term
        return val / (c - 1)


def census_buffers(graph, n_classes):
    """An empty :class:`HomophilyCensus` with the device buffers of one operator: pass it as ``out=`` to reuse them (a captured
    census has their addresses baked in).  Nothing needs initialising."""
    c, dev = int(n_classes), graph.device
    nbytes = _query("acm_homophily_workspace_bytes", graph.n_rows, graph.n_cols, c)
    return HomophilyCensus(c, torch.empty(c * c + 2 * c + 3, dtype=torch.int64, device=dev),
                           torch.empty(graph.n_rows, dtype=torch.int32, device=dev),
                           torch.empty(graph.n_rows, dtype=torch.int32, device=dev),
                           torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=dev))


def census(adj, labels, n_classes=None, row_offset=0, out=None):
    """Count the labeled pattern of ``adj`` once (``acm_homophily_census``) -> :class:`HomophilyCensus`.

    ``adj``: a CsrGraph, a FilterOperators (its ``low`` pattern), or a sparse / dense torch adjacency on the GPU; values are
    ignored.  ``labels``: int64 ``[n_cols]`` (negative = unlabeled) or one-hot ``[n_cols, C]``.  ``row_offset``: the column of
    the operator's first row (a ``slice_rows`` block).  ``out``: buffers from :func:`census_buffers`."""
    graph = _graph_of(adj, "census")
    y, c = _labels_of(labels, n_classes, "census")
    if y.shape[0] != graph.n_cols:
        raise ValueError(f"census: {y.shape[0]} labels for an operator with {graph.n_cols} columns")
    row_offset = int(row_offset)
    if row_offset < 0 or row_offset + graph.n_rows > graph.n_cols:
        raise ValueError(f"census: rows [{row_offset}, {row_offset + graph.n_rows}) are no columns of the operator")
    _require_cuda(y, "labels")
    if y.device != graph.device:
        raise ValueError(f"census: labels are on {y.device}, the operator on {graph.device}")
    res = out if out is not None else census_buffers(graph, c)
    if res.n_classes != c or res._buf is None or res.row_same.shape[0] != graph.n_rows:
        raise ValueError("census: out was made for another shape (census_buffers(graph, n_classes))")
    _launch("acm_homophily_census", graph.device, graph.handle, _vp(y), row_offset, c, _vp(res._buf),
            C.c_void_p(res._buf.data_ptr() + 8 * (c * c + 2 * c + 2)), _vp(res.row_same), _vp(res.row_deg), _vp(res._ws),
            res._ws.numel() * 8)
    res.invalidate()
    return res


# ---- the reference's names and argument order (synthetic-experiments/homophily.py) ------------------------------------
def edge_homophily(adj, label):
    """homophily.py:8-19: the share of counted entries that stay inside a class."""
    return census(adj, label).edge


def node_homophily(A, labels):
    """homophily.py:40-60: the mean over nodes with a counted neighbour of their same-class share."""
    return census(A, labels).node


def compat_matrix(A, labels):
    """homophily.py:22-37 / :63-87: the row-normalised class-to-class counts (float64 ``[C, C]`` numpy array)."""
    return census(A, labels).compat


def class_homophily(A, label):
    """homophily.py:90-111: the paper's class-insensitive measure (negative labels are unlabeled, as there)."""
    return census(A, label).klass


# ---- aggregation homophily ----------------------------------------------------------------------------------------------
def _check_z(z, y, who):
    if not isinstance(z, torch.Tensor) or z.dim() != 2 or z.dtype != torch.float32 or z.shape[1] < 1 or z.stride(1) != 1 \
            or (z.shape[0] > 1 and z.stride(0) < z.shape[1]):
        raise ValueError(f"{who}: z must be fp32 [n, F >= 1] with stride(1) == 1")
    if y.dtype != torch.int64 or y.dim() != 1 or y.shape[0] != z.shape[0] or not y.is_contiguous():
        raise ValueError(f"{who}: labels must be a contiguous int64 [n] tensor")


def _check_on_device(z, y, who):
    _require_cuda(z, "z")
    if y.device != z.device:
        raise ValueError(f"{who}: labels are on {y.device}, z on {z.device}")


def class_means(z, labels, n_classes):
    """(mu fp32 ``[C, F]``, class_count int64 ``[C]``): mu_k = mean of the rows of ``z`` with label k (``acm_class_means``);
    bit-identical from run to run."""
    c = int(n_classes)
    if not 2 <= c <= MAX_CLASSES:
        raise ValueError(f"class_means: {c} classes (2..{MAX_CLASSES})")
    _check_z(z, labels, "class_means")
    _check_on_device(z, labels, "class_means")
    n, f = z.shape
    mu = torch.empty(c, f, dtype=torch.float32, device=z.device)
    count = torch.empty(c, dtype=torch.int64, device=z.device)
    ws = torch.empty(_query("acm_class_means_workspace_bytes", n, f, c) // 8 + 1, dtype=torch.int64, device=z.device)
    _launch("acm_class_means", z.device, n, f, c, _vp(z), z.stride(0) if n > 1 else f, _vp(labels), _vp(mu), f, _vp(count), _vp(ws),
            ws.numel() * 8)
    return mu, count


def class_score(z, mu, class_count, labels, return_rows=False):
    """int64 ``[2]`` = (hits, scored rows) of the first arg-max of ``z @ mu.T`` over the classes with a member against the
    labels (``acm_class_score``, F <= 256); with ``return_rows`` also the uint8 ``[n]`` hit flags."""
    _check_z(z, labels, "class_score")
    n, f = z.shape
    c = mu.shape[0]
    if mu.dtype != torch.float32 or mu.dim() != 2 or mu.shape[1] != f or not mu.is_contiguous() or not 2 <= c <= MAX_CLASSES:
        raise ValueError("class_score: mu must be a contiguous fp32 [C, F] matrix, 2 <= C <= 64")
    if f > SCORE_MAX_FEATURES:
        raise ValueError(f"class_score: {f} features > {SCORE_MAX_FEATURES} (score z @ mu.T against the identity instead)")
    if class_count.dtype != torch.int64 or class_count.shape != (c,) or not class_count.is_contiguous():
        raise ValueError("class_score: class_count must be a contiguous int64 [C] tensor")
    _check_on_device(z, labels, "class_score")
    counts = torch.empty(2, dtype=torch.int64, device=z.device)
    rows = torch.empty(n, dtype=torch.uint8, device=z.device) if return_rows else None
    _launch("acm_class_score", z.device, n, f, c, _vp(z), z.stride(0) if n > 1 else f, _vp(mu), f, _vp(class_count), _vp(labels),
            _vp(rows), _vp(counts))
    return (counts, rows) if return_rows else counts


def aggregated(features, adj, graph=None):
    """Z = A X with the operator's VALUES: a valued CsrGraph (or torch adjacency), or the pattern + row scale of an implicit
    FilterOperators, through the SpMM wrappers (which convert a features matrix of another floating type to fp32).
    ``graph``: the operator's CsrGraph where the caller has resolved it already."""
    from .functional import spmm
    if graph is None:
        graph = _graph_of(adj, "aggregation_homophily")
    if isinstance(adj, FilterOperators) and adj.implicit:
        return spmm(graph, features, row_scale=adj.row_scale)
    return spmm(graph, features)


def aggregation_homophily(features, adj, label, modified=True, return_rows=False, n_classes=None):
    """homophily.py:114-124 without the ``n x n`` inner-product matrix: Z = A X, mu_k = mean of Z_u over y_u = k,
    hit_v = [first arg-max_k Z_v . mu_k == y_v]; returns hits / n_labeled (a Python float; with ``return_rows`` also the
    uint8 hit flags).  ``features=None``: the one-hot labels (the paper's label-based form); features of another floating
    type (float64, bf16) are converted to fp32 by the SpMM wrapper, integer features are refused.  ``modified`` is accepted
    and ignored, as in the reference.  ``n_classes``: the class count where the labels do not say it -- an index vector whose
    highest classes have no member; without it C is ``label.max() + 1`` (one host read) or the one-hot width.  Unlabeled
    rows enter no mean and are not scored; a class without a member is never chosen (the reference produces NaN there)."""
    del modified
    graph = _graph_of(adj, "aggregation_homophily")            # (also: refuses a sharded operator before any work)
    y, c = _labels_of(label, n_classes, "aggregation_homophily")
    if graph.n_rows != graph.n_cols or y.shape[0] != graph.n_rows:
        raise ValueError(f"aggregation_homophily: a square operator and one label per node are needed "
                         f"({graph.n_rows} x {graph.n_cols}, {y.shape[0]} labels)")
    if features is None:
        features = torch.zeros(y.shape[0], c, dtype=torch.float32, device=y.device)
        lab = (y >= 0) & (y < c)
        features[lab] = torch.nn.functional.one_hot(y[lab], c).to(torch.float32)
    if not isinstance(features, torch.Tensor) or features.dim() != 2 or features.shape[0] != graph.n_cols:
        raise ValueError(f"aggregation_homophily: features must be [n, F] with n = {graph.n_cols}")
    if not features.is_floating_point():
        raise ValueError(f"aggregation_homophily: features must be floating point, got {features.dtype}")
    _require_cuda(features, "features")
    _require_cuda(y, "labels")
    z = aggregated(features, adj, graph)
    mu, count = class_means(z, y, c)
    if z.shape[1] > SCORE_MAX_FEATURES:                        # W = Z mu^T on acm_gemm, then the same kernel against I_C: exact
        from .functional import gemm
        z = gemm(z, mu, trans_b=True)
        mu = torch.eye(c, dtype=torch.float32, device=z.device)
    res = class_score(z, mu, count, y, return_rows=return_rows)
    counts, rows = res if return_rows else (res, None)
    hits, scored = (int(v) for v in counts.tolist())
    value = hits / scored if scored else float("nan")
    return (value, rows) if return_rows else value
