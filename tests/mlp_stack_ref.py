"""Deep mlpX stacks (Linear -> ReLU -> BatchNorm1d -> ... -> Linear, ACM-Pytorch/models/layers.py:245-285) restated in numpy
float64 -- TEST CODE: the yardstick of tests/test_mlp_stack_cpu.py and tests/test_gpu_mlp_stack.py, pinned to the reference's
own module by tests/golden/mlp_stack_cases.npz -- and ``StackFakeLib``, the CPU double of the library (tests/fake_lib.FakeLib)
with the acm_bnorm_* entry points on top.

The restatement is the TEXTBOOK form (normalise, then the next Linear; BatchNorm's three-term backward), not the folded
algebra the kernels use: agreement of the two is what the tests check."""
import numpy as np

from fake_lib import FakeLib, _vec, _view

EPS = 1e-5


def forward(x, lins, bns, train=True, running=None, momentum=0.1, eps=EPS, relu=True, factors=None):
    """y = factors * relu?(mlp(x)).  lins: [(W [out, in], b)], bns: [(gamma, beta)], running: [(mean, var)] per BatchNorm
    (read in evaluation mode; in training mode the UPDATED pairs are returned).  Returns (y, cache, new_running)."""
    z = np.asarray(x, np.float64)
    cache, new_running = [], []
    for i, (w, b) in enumerate(lins[:-1]):
        pre = z @ np.asarray(w, np.float64).T + np.asarray(b, np.float64)
        h = np.maximum(pre, 0.0)
        n = h.shape[0]
        if train:
            mu, var = h.mean(0), h.var(0)
            if running is not None:
                rm, rv = running[i]
                new_running.append(((1 - momentum) * np.asarray(rm, np.float64) + momentum * mu,
                                    (1 - momentum) * np.asarray(rv, np.float64) + momentum * var * n / (n - 1)))
        else:
            mu, var = (np.asarray(t, np.float64) for t in running[i])
        r = 1.0 / np.sqrt(var + eps)
        xhat = (h - mu) * r
        g, bt = (np.asarray(t, np.float64) for t in bns[i])
        cache.append((z, pre, xhat, r))
        z = xhat * g + bt
    w, b = lins[-1]
    pre = z @ np.asarray(w, np.float64).T + np.asarray(b, np.float64)
    y = np.maximum(pre, 0.0) if relu else pre
    if factors is not None:
        y = y * factors
    cache.append((z, pre, None, None))
    return y, cache, new_running


def backward(dy, lins, bns, cache, relu=True, factors=None):
    """Gradients of sum(dy * y) in TRAINING mode: (dx, [(dW, db)], [(dgamma, dbeta)])."""
    g = np.asarray(dy, np.float64)
    if factors is not None:
        g = g * factors
    z, pre, _, _ = cache[-1]
    if relu:
        g = g * (pre > 0)
    d_lins, d_bns = [None] * len(lins), [None] * len(bns)
    for i in range(len(lins) - 1, -1, -1):
        w = np.asarray(lins[i][0], np.float64)
        z = cache[i][0]
        d_lins[i] = (g.T @ z, g.sum(0))
        dz = g @ w
        if i == 0:
            return dz, d_lins, d_bns
        _, pre_prev, xhat, r = cache[i - 1]
        gamma = np.asarray(bns[i - 1][0], np.float64)
        d_bns[i - 1] = ((dz * xhat).sum(0), dz.sum(0))
        dxhat = dz * gamma
        n = dz.shape[0]
        dh = r * (dxhat - dxhat.mean(0) - xhat * (dxhat * xhat).sum(0) / n)
        g = dh * (pre_prev > 0)


def forward_torch(x, lins, bns, eps=EPS):
    """Training-mode mlp(x) on torch tensors (float64, differentiable): what the GPU tests compose with the oracle's layer
    functions.  tests/test_mlp_stack_cpu.py checks it against forward / backward above."""
    import torch
    z = x
    for (w, b), (gamma, beta) in zip(lins[:-1], bns):
        h = torch.relu(z @ w.T + b)
        z = (h - h.mean(0)) / torch.sqrt(h.var(0, unbiased=False) + eps) * gamma + beta
    return z @ lins[-1][0].T + lins[-1][1]


class StackFakeLib(FakeLib):
    """FakeLib + acm_bnorm_stats / _fold / _param_bwd / _bwd as include/acm_hip.h states them (float64 arithmetic, fp32 storage)."""

    def acm_bnorm_stats_workspace_bytes(self, n, f, out):
        if not 1 <= f <= 256:
            self._err = b"acm_bnorm_stats: f outside 1..256"
            return 4
        out._obj.value = 64
        return 0

    def acm_bnorm_stats(self, n, f, h, ldh, gamma, beta, eps, momentum, train, rm, rv, nbt, stats, ws, wsb, stream):
        out = _view(stats, 4, f, f)
        if train:
            if n < 2:
                self._err = b"acm_bnorm_stats: batch statistics need more than one row"
                return 2
            H = _view(h, n, f, ldh).astype(np.float64)
            mu, var = H.mean(0), H.var(0)
            if rm:
                m = _vec(rm, f)
                m[...] = (1 - momentum) * m.astype(np.float64) + momentum * mu
            if rv:
                v = _vec(rv, f)
                v[...] = (1 - momentum) * v.astype(np.float64) + momentum * var * n / (n - 1)
            if nbt:
                _vec(nbt, 1, np.int64)[0] += 1
        else:
            mu, var = _vec(rm, f).astype(np.float64), _vec(rv, f).astype(np.float64)
        r = 1.0 / np.sqrt(var + eps)
        a = _vec(gamma, f).astype(np.float64) * r
        out[0], out[1], out[2], out[3] = mu, r, a, _vec(beta, f).astype(np.float64) - mu * a
        return 0

    def acm_bnorm_fold(self, f_out, f_in, w, ldw, bias, stats, wf, ldwf, bf, stream):
        st = _view(stats, 4, f_in, f_in).astype(np.float64)
        W = _view(w, f_out, f_in, ldw).astype(np.float64)
        _view(wf, f_out, f_in, ldwf)[...] = W * st[2][None, :]
        _vec(bf, f_out)[...] = (_vec(bias, f_out).astype(np.float64) if bias else 0.0) + W @ st[3]
        return 0

    def acm_bnorm_param_bwd(self, f_out, f_in, m, ldm, s, w, ldw, stats, dw, lddw, d_beta, d_gamma, stream):
        mu, r, a, c = _view(stats, 4, f_in, f_in).astype(np.float64)
        M, W = _view(m, f_out, f_in, ldm).astype(np.float64), _view(w, f_out, f_in, ldw).astype(np.float64)
        sv = _vec(s, f_out).astype(np.float64)
        _view(dw, f_out, f_in, lddw)[...] = M * a[None, :] + np.outer(sv, c)
        db = sv @ W
        _vec(d_beta, f_in)[...] = db
        _vec(d_gamma, f_in)[...] = r * ((W * M).sum(0) - mu * db)
        return 0

    def acm_bnorm_bwd_workspace_bytes(self, n, f, out):
        if not 1 <= f <= 256:
            self._err = b"acm_bnorm_bwd: f outside 1..256"
            return 4
        out._obj.value = 64
        return 0

    def acm_bnorm_bwd(self, n, f, dz, lddz, h, ldh, stats, d_beta, d_gamma, keep_scale, relu, g, ldg, d_bias, ws, wsb, defer, stream):
        dZ, H = _view(dz, n, f, lddz).astype(np.float64), _view(h, n, f, ldh).astype(np.float64)
        if stats:
            mu, r, a, _ = _view(stats, 4, f, f).astype(np.float64)
            db, dg = _vec(d_beta, f).astype(np.float64), _vec(d_gamma, f).astype(np.float64)
            G = np.where(H > 0, a * (dZ - db / n - (H - mu) * r * dg / n), 0.0)
        elif relu:
            G = np.where(H > 0, dZ * keep_scale, 0.0)
        elif keep_scale != 1.0:
            G = np.where(H != 0, dZ * keep_scale, 0.0)
        else:
            G = dZ
        _view(g, n, f, ldg)[...] = G
        return self._emit(defer, [(_vec(d_bias, f), G.sum(0))])


def install(monkeypatch):
    """tests/fake_lib.install, then the double with the acm_bnorm_* symbols in its place and the stack's device seam lifted."""
    import fake_lib
    from acm_gnn_amd import _lib
    from acm_gnn_amd.functional import linear
    fake_lib.install(monkeypatch)
    fake = StackFakeLib()
    monkeypatch.setattr(_lib, "load", lambda build_if_missing=True: fake)
    monkeypatch.setattr(_lib, "check", lambda st, what="": (_ for _ in ()).throw(
        RuntimeError(f"{what}: {fake.acm_last_error().decode()} ({_lib.STATUS_NAMES.get(st, st)})")) if st else None)
    monkeypatch.setattr(linear, "_ON_DEVICE", lambda t: True)
    return fake
