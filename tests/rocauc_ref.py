"""numpy / CPU-torch expectations for the ROC-AUC tests: the score the reference uses (fp32 softmax, column 1), the exact integer
statistic from two ``searchsorted`` calls, and the inputs on which fp32 scores tie and order the same way on any device."""
import numpy as np
import torch


def cpu_scores(logits):
    """data_utils.eval_rocauc's score for single-column labels: F.softmax(out, dim=-1)[:, 1] in fp32, on the CPU."""
    return torch.softmax(torch.as_tensor(logits).detach().float().cpu(), dim=-1)[:, 1].numpy()


def triple(scores, labels, members):
    """(U2, npos, nneg) of one set: U2 = sum over positives of 2 #{negatives below} + #{negatives equal}; rows of the set with
    a label other than 0 / 1 are skipped.  ``members``: boolean mask or index array."""
    labels = np.asarray(labels).reshape(-1)
    mask = np.zeros(labels.shape[0], bool)
    mask[np.asarray(members)] = True
    pos = scores[mask & (labels == 1)]
    neg = np.sort(scores[mask & (labels == 0)])
    u2 = int(np.searchsorted(neg, pos, "left").sum()) + int(np.searchsorted(neg, pos, "right").sum())
    return u2, int(pos.size), int(neg.size)


def auc_of(t):
    u2, npos, nneg = (int(v) for v in t)
    return u2 / (2 * npos * nneg) if npos and nneg else float("nan")


def midrank_auc(y_true, score):
    """sklearn.metrics.roc_auc_score for binary labels."""
    y_true = np.asarray(y_true).reshape(-1)
    return auc_of(triple(np.asarray(score).reshape(-1), y_true, np.ones(y_true.shape[0], bool)))


def close_pairs(scores, labels, members, ulps=8):
    """Positive-negative pairs of the set whose scores differ by at most ``ulps`` fp32 ulps (relative): the pairs whose order
    another device's expf / divide may decide differently.  Each can move U2 by at most 2."""
    labels = np.asarray(labels).reshape(-1)
    mask = np.zeros(labels.shape[0], bool)
    mask[np.asarray(members)] = True
    pos = scores[mask & (labels == 1)].astype(np.float64)
    neg = np.sort(scores[mask & (labels == 0)]).astype(np.float64)
    rel = ulps * 2.0 ** -23
    return int((np.searchsorted(neg, pos * (1 + rel), "right") - np.searchsorted(neg, pos * (1 - rel), "left")).sum())


def auc_bound(scores, labels, members):
    """|AUC_device - AUC_cpu| <= (P_close + 1) / (npos nneg) (the + 1: the float64 quotient)."""
    _, npos, nneg = triple(scores, labels, members)
    return (close_pairs(scores, labels, members) + 1) / (npos * nneg)


def grid_logits(n, seed, extremes=True, levels=None):
    """[n, 2] fp32 logits with z_0 and z_1 - z_0 on a 0.25 grid, |z_1 - z_0| <= 8: neighbouring scores are >= 7e-5 apart and equal
    differences give bit-equal scores wherever the row maximum is subtracted first.  ``extremes`` (n >= 257): the last 64 rows get
    differences of +/- 20, 24, 28, 32 -- the positive ones all score exactly 1.0.  ``levels``: only that many distinct differences."""
    rng = np.random.default_rng(seed)
    z0 = rng.integers(-16, 17, n) * 0.25
    d = rng.integers(-32, 33, n) * 0.25 if levels is None else (rng.integers(0, levels, n) - levels // 2) * 1.0
    if extremes and n >= 257:
        d[-64:] = np.tile(np.array([20, 24, 28, 32, -20, -24, -28, -32], np.float64), 8)
    return np.stack([z0, z0 + d], 1).astype(np.float32)
