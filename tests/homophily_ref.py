"""numpy restatement of the homophily measures (include/acm_hip.h, "homophily measures on the device"): the sparse census in
exact integers, the four label measures in float64, and aggregation homophily per row in float64.  Independent of the
package: the CPU tests compare it with the reference's recorded values, the GPU tests compare the kernels with it."""
import numpy as np


def planted_graph(n, n_classes, seed, k=4, h=0.7, hub=0, isolated=0, unlabeled=0):
    """(directed edge list [m, 2] of a symmetric simple graph, labels): every node draws ``k`` partners, of its own class with
    probability ``h``; node 0 gets ``hub`` extra neighbours; ``isolated`` nodes from the middle lose every edge; ``unlabeled``
    nodes get the label -1.  Every class keeps a member and the last node keeps an edge."""
    rng = np.random.default_rng(seed)
    y = rng.integers(0, n_classes, n).astype(np.int64)
    y[:n_classes] = np.arange(n_classes)
    by_class = [np.flatnonzero(y == c) for c in range(n_classes)]
    src, dst = [], []
    for i in range(n):
        for _ in range(k):
            j = int(rng.choice(by_class[y[i]])) if rng.random() < h else int(rng.integers(0, n))
            if j != i:
                src.append(i), dst.append(j)
    if hub:
        for j in rng.choice(np.arange(1, n), hub, replace=False):
            src.append(0), dst.append(int(j))
    a = np.zeros((n, n), bool)
    a[src, dst] = True
    a |= a.T
    lonely = np.arange(n // 2, n // 2 + isolated)
    a[lonely, :] = False
    a[:, lonely] = False
    if not a[n - 1].any():
        a[n - 1, 1] = a[1, n - 1] = True
    if unlabeled:
        y[rng.choice(np.arange(n_classes, n), unlabeled, replace=False)] = -1
    e = np.argwhere(a).astype(np.int32)
    return e, y


def csr_of_edges(edges, n):
    """(indptr, indices) int32 of a directed edge list, rows sorted, columns sorted within a row."""
    order = np.lexsort((edges[:, 1], edges[:, 0]))
    e = edges[order]
    indptr = np.zeros(n + 1, np.int64)
    np.add.at(indptr, e[:, 0].astype(np.int64) + 1, 1)
    return np.cumsum(indptr).astype(np.int32), e[:, 1].astype(np.int32)


def normalised_operator(edges, n):
    """CSR (indptr, indices, fp32 vals) of D^-1 (A + I), D = rowsum(A + I) (a raw self-loop makes the diagonal count twice)."""
    import scipy.sparse as sp
    a = sp.coo_matrix((np.ones(len(edges)), (edges[:, 0], edges[:, 1])), shape=(n, n)).tocsr() + sp.identity(n, format="csr")
    a.sum_duplicates()
    a.sort_indices()
    d = np.asarray(a.sum(1)).ravel()
    vals = a.data / np.repeat(d, np.diff(a.indptr))
    return a.indptr.astype(np.int32), a.indices.astype(np.int32), vals.astype(np.float32)


def census(indptr, indices, y, n_classes, row_offset=0):
    """dict(M, cls, iso, n_labeled, n_deg, row_same, row_deg, node_sum) of the stored pattern; ``y`` has one label per column."""
    c = int(n_classes)
    indptr, indices, y = np.asarray(indptr, np.int64), np.asarray(indices, np.int64), np.asarray(y, np.int64)
    n_rows = len(indptr) - 1
    rows = np.repeat(np.arange(n_rows), np.diff(indptr))
    yl = np.where((y >= 0) & (y < c), y, -1)
    yr, yc = yl[rows + row_offset], yl[indices]
    offd = indices != rows + row_offset
    counted = offd & (yr >= 0) & (yc >= 0)
    m = np.zeros((c, c), np.int64)
    np.add.at(m, (yr[counted], yc[counted]), 1)
    row_deg = np.bincount(rows[counted], minlength=n_rows).astype(np.int32)
    row_same = np.bincount(rows[counted & (yr == yc)], minlength=n_rows).astype(np.int32)
    own = yl[row_offset:row_offset + n_rows]
    cls = np.bincount(own[own >= 0], minlength=c).astype(np.int64)
    stored_off = np.bincount(rows[offd], minlength=n_rows)
    iso = np.bincount(own[(own >= 0) & (stored_off == 0)], minlength=c).astype(np.int64)
    has = row_deg > 0
    return dict(M=m, cls=cls, iso=iso, n_labeled=int((own >= 0).sum()), n_deg=int(has.sum()), row_same=row_same, row_deg=row_deg,
                node_sum=float(np.sum(row_same[has].astype(np.float64) / row_deg[has].astype(np.float64))))


def counts_vector(cs):
    """The census as the library lays it out: int64 [C*C + 2C + 2]."""
    return np.concatenate([cs["M"].ravel(), cs["cls"], cs["iso"], [cs["n_labeled"], cs["n_deg"]]]).astype(np.int64)


def edge(cs):
    return float(np.trace(cs["M"])) / float(cs["M"].sum())


def node(cs):
    return cs["node_sum"] / cs["n_deg"]


def compat(cs):
    m = cs["M"].astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return m / m.sum(1, keepdims=True)


def klass(cs):
    c = cs["M"].shape[0]
    h = (cs["M"] + np.diag(cs["iso"])).astype(np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        h = h / h.sum(1, keepdims=True)
    p = cs["cls"].astype(np.float64) / cs["n_labeled"]
    terms = np.maximum(np.diag(h) - p, 0.0)
    return float(np.nansum(terms)) / (c - 1)


def class_means(z64, y, n_classes):
    """(mu float64 [C, F], count [C]); an empty class has mu = 0."""
    c = int(n_classes)
    mu = np.zeros((c, z64.shape[1]))
    count = np.zeros(c, np.int64)
    for k in range(c):
        sel = y == k
        count[k] = int(sel.sum())
        if count[k]:
            mu[k] = z64[sel].mean(0)
    return mu, count


def agg_rows(z64, y, n_classes):
    """(hits bool [n] -- False for an unlabeled row --, margins float64 [n]) of aggregation homophily in float64:
    W = Z mu^T with -inf for a class without a member, hit = [first arg-max == y], margin = (top1 - top2) / max|W|."""
    y = np.asarray(y, np.int64)
    yl = np.where((y >= 0) & (y < n_classes), y, -1)
    mu, count = class_means(z64, yl, n_classes)
    w = z64 @ mu.T
    scale = float(np.abs(w).max()) if w.size else 1.0
    w[:, count == 0] = -np.inf
    arg = w.argmax(1)                                          # numpy takes the first maximum, like torch.argmax
    top = np.sort(w, 1)[:, ::-1]
    with np.errstate(invalid="ignore"):
        margins = (top[:, 0] - top[:, 1]) / (scale if scale > 0 else 1.0)
    margins = np.where(np.isnan(margins), 0.0, margins)
    return (arg == yl) & (yl >= 0), margins


def dense_times(indptr, indices, vals, x):
    """float64 product of a CSR operator (its fp32 values read as float64) with x."""
    import scipy.sparse as sp
    n = len(indptr) - 1
    a = sp.csr_matrix((np.asarray(vals, np.float64), indices, indptr), shape=(n, int(x.shape[0])))
    return a @ np.asarray(x, np.float64)


def one_hot(y, n_classes):
    out = np.zeros((len(y), n_classes), np.float32)
    lab = y >= 0
    out[np.flatnonzero(lab), y[lab]] = 1.0
    return out
