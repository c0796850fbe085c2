"""TEST INFRASTRUCTURE: a numpy restatement of the sampling contract of the synthetic graph generator (include/acm_hip.h,
"synthetic graphs"; acm_gnn_amd/csrc/acm_synth.hip) on ``oracle.philox.philox7_words``.  Independent of the package: the tests
compare the device output with these arrays bit for bit.  Vectorised over rows / draws."""
import math

import numpy as np

from oracle.philox import philox7_words

TAG_REG_INTRA, TAG_REG_INTER, TAG_PAIR, TAG_RECT, TAG_UNIFORM, TAG_RANGE = 0x5301, 0x5302, 0x5303, 0x5304, 0x5305, 0x5306
PAIR, RECT, RANGE = 0, 1, 2
INVALID = np.iinfo(np.int64).max
MAX_DEGREE = 256


# ---- k distinct of [0, m) per row: Floyd ---------------------------------------------------------------------------------
def floyd(seed, graph_index, tag, rows, k, m):
    """int64 [len(rows), k]: the Floyd sample of every row, in step order (step s uses word s of the row's stream)."""
    rows = np.asarray(rows, dtype=np.int64)
    out = np.full((len(rows), k), -1, np.int64)
    if k == 0:
        return out
    calls = (k + 3) // 4
    w = philox7_words(seed, graph_index, tag, np.repeat(rows[:, None], calls, 1), np.repeat(np.arange(calls)[None], len(rows), 0))
    words = np.moveaxis(w, 0, -1).reshape(len(rows), calls * 4).astype(np.uint64)      # word s = call s >> 2, word s & 3
    for s in range(k):
        t = m - k + s
        r = ((words[:, s] * np.uint64(t + 1)) >> np.uint64(32)).astype(np.int64)
        taken = (out[:, :s] == r[:, None]).any(1)
        out[:, s] = np.where(taken, t, r)
    return out


def degree_inter_of(degree_intra, edge_homo):
    return int(degree_intra / edge_homo - degree_intra)                                # graph_generation.py:25


def regular(n_classes, npc, degree_intra, degree_inter, seed, graph_index, rows=None):
    """int32 [rows, d] column ids, every row ascending (the CSR indices; indptr is j * d)."""
    n = n_classes * npc
    b, e = (0, n) if rows is None else rows
    j = np.arange(b, e, dtype=np.int64)
    base = j // npc * npc
    a = floyd(seed, graph_index, TAG_REG_INTRA, j, degree_intra, npc - 1)
    a = base[:, None] + a + (a >= (j - base)[:, None])
    o = floyd(seed, graph_index, TAG_REG_INTER, j, degree_inter, n - npc)
    o = o + np.where(o >= base[:, None], npc, 0)
    return np.sort(np.concatenate([a, o], 1), 1).astype(np.int32)


# ---- the first M distinct keys of a stream ----------------------------------------------------------------------------------
def _mulhi64(v, r):
    m = np.uint64(0xFFFFFFFF)
    s = np.uint64(32)
    vh, vl, rh, rl = v >> s, v & m, np.uint64(r >> 32), np.uint64(r & 0xFFFFFFFF)
    mid1, mid2 = vh * rl, vl * rh
    carry = ((mid1 & m) + (mid2 & m) + ((vl * rl) >> s)) >> s
    return vh * rh + (mid1 >> s) + (mid2 >> s) + carry


def draw_keys(kind, a, b, block, seed, graph_index, n_draws):
    """int64 [n_draws]: the keys of draws 0 .. n_draws - 1 of one stream (INVALID where the slot decodes to nothing)."""
    tag = {PAIR: TAG_PAIR, RECT: TAG_RECT, RANGE: TAG_RANGE}[kind]
    calls = (n_draws + 1) // 2
    w = philox7_words(seed, graph_index, tag, np.arange(calls, dtype=np.int64), np.full(calls, block, np.int64)).astype(np.uint64)
    v = np.stack([(w[0] << np.uint64(32)) | w[1], (w[2] << np.uint64(32)) | w[3]], 1).reshape(-1)[:n_draws]
    r = a * a if kind == PAIR else a * b
    slot = _mulhi64(v, r).astype(np.int64)
    if kind != PAIR:
        return slot
    x, y = slot // a, slot % a
    return np.where(x == y, INVALID, np.minimum(x, y) * a + np.maximum(x, y))


def first_distinct(keys, m):
    """(the first ``m`` distinct valid keys in draw order, short): short = the stream held fewer than ``m``."""
    uniq, first = np.unique(keys, return_index=True)
    first = np.sort(first[uniq != INVALID])
    return keys[first[:max(m, 0)]], len(first) < m


def select(kind, a, b, block, seed, graph_index, m, n_draws=64):
    """The first ``m`` distinct keys of the stream, whatever length it takes (None if the key space is too small)."""
    n_keys = a * (a - 1) // 2 if kind == PAIR else a * b
    if m > n_keys:
        return None
    while True:
        got, short = first_distinct(draw_keys(kind, a, b, block, seed, graph_index, n_draws), m)
        if not short:
            return got
        n_draws *= 2


# ---- the random type ----------------------------------------------------------------------------------------------------
def random_graph(n_classes, npc, degree_intra, edge_homo, seed, graph_index):
    """dict(indptr int32, indices int32, block_counts int64 [C, C], m int64 [C - 1], t float) of the `random` type."""
    c, n = n_classes, n_classes * npc
    s_edges = degree_intra * npc
    assert s_edges % 2 == 0
    rows, cols = [], []
    blocks = np.zeros((c, c), np.int64)
    for i in range(c):
        key = select(PAIR, npc, 1, i, seed, graph_index, s_edges // 2)
        x, y = key // npc + i * npc, key % npc + i * npc
        rows += [x, y]
        cols += [y, x]
        blocks[i, i] = 2 * len(key)
    t = s_edges * (1 - edge_homo) / edge_homo                                           # graph_generation.py:98, float64
    ms, pre = [], []
    for i in range(c - 1):
        pre.append(round(t - float(blocks[:i, i].sum())) + 1)               # before the clamp: negative once e_i > T + 1.5
        m = max(0, pre[-1])
        ms.append(m)
        width = (c - 1 - i) * npc
        key = select(RECT, npc, width, i, seed, graph_index, m)
        x, y = key // width + i * npc, key % width + (i + 1) * npc
        rows += [x, y]
        cols += [y, x]
        dest = np.bincount(y // npc, minlength=c)
        blocks[i] += dest
        blocks[:, i] += dest
    k = np.sort(np.concatenate(rows) * n + np.concatenate(cols))
    assert len(np.unique(k)) == len(k)
    indptr = np.zeros(n + 1, np.int64)
    indptr[1:] = np.cumsum(np.bincount(k // n, minlength=n))
    return dict(indptr=indptr.astype(np.int32), indices=(k % n).astype(np.int32), block_counts=blocks, m=np.array(ms, np.int64),
                pre_clamp=np.array(pre, np.int64), t=t)


# four classes, T = 1.78: class 0 sends 3 edges, class 1 up to 3 more; five of them into block 2 give rint(T - 5) + 1 = -2
CLAMP_CASE = dict(n_classes=4, npc=8, degree_intra=2, edge_homo=0.9)


def clamp_seed():
    """(seed, class i): the first seed at which a class of CLAMP_CASE has round(T - e_i) + 1 < 0, so that m_i = 0 comes from
    the clamp max(0, .) and not from the arithmetic."""
    for seed in range(200):
        g = random_graph(seed=seed, graph_index=0, **CLAMP_CASE)
        neg = np.nonzero(g["pre_clamp"] < 0)[0]
        if len(neg):
            return seed, int(neg[0])
    raise AssertionError("no seed with a negative count before the clamp among the first 200")


def block_counts(indptr, indices, n_classes, npc, row_begin=0):
    rows = np.repeat(np.arange(len(indptr) - 1), np.diff(indptr)) + row_begin
    return np.bincount(rows // npc * n_classes + indices // npc, minlength=n_classes * n_classes).reshape(n_classes, n_classes)


# ---- features -------------------------------------------------------------------------------------------------------------
def uniform(n, f, seed, graph_index=0, row_begin=0):
    """fp32 [n, f] in [0, 1): column c of row r is word c & 3 of the call (row, block c >> 2), (word >> 8) * 2^-24."""
    f4 = (f + 3) // 4
    r, b = np.meshgrid(np.arange(row_begin, row_begin + n, dtype=np.int64), np.arange(f4), indexing="ij")
    w = philox7_words(seed, graph_index, TAG_UNIFORM, r, b)
    x = np.moveaxis(w, 0, -1).reshape(n, f4 * 4)[:, :f]
    return ((x >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)).astype(np.float32)


def base_feature_rows(base_y, n_classes, npc, seed, graph_index):
    """int64 [n_classes * npc] rows of the base data set (feature_generation.py:36-54): class j draws from base class
    j % n_base; more than npc members: the first npc distinct members of its RANGE stream (block j); otherwise every member,
    then npc - count further distinct ones.  ValueError where numpy's choice(replace=False) raises."""
    base_y = np.asarray(base_y)
    n_base = int(base_y.max()) + 1
    out = []
    for j in range(n_classes):
        members = np.where(base_y == j % n_base)[0]
        count = len(members)
        m = npc if count > npc else npc - count
        if m > count or (count == 0 and npc > 0):
            raise ValueError("Cannot take a larger sample than population when 'replace=False'")
        pick = members[select(RANGE, count, 1, j, seed, graph_index, m)] if m else members[:0]
        out += [pick] if count > npc else [members, pick]
    return np.concatenate(out).astype(np.int64)


# ---- uniformity -------------------------------------------------------------------------------------------------------------
def chi2(counts):
    counts = np.asarray(counts, dtype=np.float64)
    e = counts.sum() / len(counts)
    return float(((counts - e) ** 2).sum() / e)


def chi2_quantile(df, upper_tail):
    """Wilson-Hilferty quantile of chi-square with ``df`` degrees of freedom at upper tail probability ``upper_tail``
    (accurate to a fraction of a percent for df >= 100; z by bisection on erfc)."""
    lo, hi = 0.0, 10.0
    for _ in range(80):
        mid = (lo + hi) / 2
        lo, hi = (mid, hi) if 0.5 * math.erfc(mid / math.sqrt(2)) > upper_tail else (lo, mid)
    z = (lo + hi) / 2
    return df * (1 - 2 / (9 * df) + z * math.sqrt(2 / (9 * df))) ** 3
