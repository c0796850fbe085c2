"""Deep mlpX stacks (Linear -> ReLU -> BatchNorm1d -> ... -> Linear, ACM-Pytorch/models/layers.py:245-285) restated in numpy
float64 -- TEST CODE: the yardstick of tests/test_mlp_stack_cpu.py and tests/test_gpu_mlp_stack.py, pinned to the reference's
own module by tests/golden/mlp_stack_cases.npz -- and ``StackFakeLib``, the CPU double of the library (tests/fake_lib.FakeLib)
with the acm_bnorm_* entry points and the two shifted products (acm_linear_fwd_shift, acm_gemm_shift) on top.

The restatement is the TEXTBOOK form (normalise, then the next Linear; BatchNorm's three-term backward), not the folded
algebra the kernels use: agreement of the two is what the tests check."""
import numpy as np

from fake_lib import FakeLib, _vec, _view, dropout_factors

EPS = 1e-5


def matmul(a, b):
    """a @ b.  float32 operands: one chain of float32 additions in k order per element -- the plainest order there is, the one the
    fp32 matrix pipe uses (acm_gemm.hip), and the same on every machine (a BLAS picks its blocking by CPU; the float32 form's
    error is the unit of tests/bnorm_regimes.py and must not depend on where the tests run)."""
    if a.dtype != np.float32:
        return a @ b
    assert b.dtype == np.float32
    out = np.zeros((a.shape[0], b.shape[1]), np.float32)
    for k in range(a.shape[1]):
        out += a[:, k:k + 1] * b[k:k + 1, :]
    return out


def forward(x, lins, bns, train=True, running=None, momentum=0.1, eps=EPS, relu=True, factors=None, dtype=np.float64):
    """y = factors * relu?(mlp(x)).  lins: [(W [out, in], b)], bns: [(gamma, beta)], running: [(mean, var)] per BatchNorm
    (read in evaluation mode; in training mode the UPDATED pairs are returned).  Returns (y, cache, new_running).  ``dtype``:
    the precision of every operation (np.float32: the same textbook form as a float32 program would run it -- the unit of
    tests/bnorm_regimes.py)."""
    z = np.asarray(x, dtype)
    cache, new_running = [], []
    for i, (w, b) in enumerate(lins[:-1]):
        pre = matmul(z, np.asarray(w, dtype).T) + np.asarray(b, dtype)
        h = np.maximum(pre, 0.0)
        n = h.shape[0]
        if train:
            mu, var = h.mean(0), h.var(0)
            if running is not None:
                rm, rv = running[i]
                new_running.append(((1 - momentum) * np.asarray(rm, dtype) + momentum * mu,
                                    (1 - momentum) * np.asarray(rv, dtype) + momentum * var * n / (n - 1)))
        else:
            mu, var = (np.asarray(t, dtype) for t in running[i])
        r = 1.0 / np.sqrt(var + eps)
        xhat = (h - mu) * r
        g, bt = (np.asarray(t, dtype) for t in bns[i])
        cache.append((z, pre, xhat, r))
        z = xhat * g + bt
    w, b = lins[-1]
    pre = matmul(z, np.asarray(w, dtype).T) + np.asarray(b, dtype)
    y = np.maximum(pre, 0.0) if relu else pre
    if factors is not None:
        y = y * np.asarray(factors, dtype)
    cache.append((z, pre, None, None))
    assert y.dtype == dtype
    return y, cache, new_running


def backward(dy, lins, bns, cache, relu=True, factors=None, dtype=np.float64, trace=None):
    """Gradients of sum(dy * y) in TRAINING mode: (dx, [(dW, db)], [(dgamma, dbeta)]).  ``trace``: a dict that receives, per
    Linear i, "G{i}" = dL/d(its pre-activation) and, per BatchNorm i, "dZ{i}" = dL/d(its output)."""
    g = np.asarray(dy, dtype)
    if factors is not None:
        g = g * np.asarray(factors, dtype)
    z, pre, _, _ = cache[-1]
    if relu:
        g = g * (pre > 0)
    d_lins, d_bns = [None] * len(lins), [None] * len(bns)
    for i in range(len(lins) - 1, -1, -1):
        w = np.asarray(lins[i][0], dtype)
        z = cache[i][0]
        if trace is not None:
            trace[f"G{i}"] = g
        d_lins[i] = (matmul(g.T, z), g.sum(0))
        dz = matmul(g, w)
        if i == 0:
            assert dz.dtype == dtype
            return dz, d_lins, d_bns
        _, pre_prev, xhat, r = cache[i - 1]
        gamma = np.asarray(bns[i - 1][0], dtype)
        if trace is not None:
            trace[f"dZ{i - 1}"] = dz
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
    """FakeLib + acm_bnorm_stats / _fold / _param_bwd / _bwd, their centred forms and the two shifted products as include/acm_hip.h
    states them (float64 arithmetic, fp32 storage).  Three switches, all for tests/test_bnorm_regimes_cpu.py:
    ``fp32``      every operation of the stack's entry points in float32, as the kernels run them (the statistics themselves come
                  from float64 and are rounded: acm_bnorm_stats keeps their digits, tests/test_gpu_mlp_stack.py);
    ``centred``   False: a library without the centred symbols (_lib.BNORM_CENTRED_SYMBOLS) -- the package then takes the
                  stack's first form: both products on H itself, c = beta - mu a folded into the bias, dW = M a + s c,
                  dgamma = r (q - mu dbeta);
    ``bwd_shift`` False: a bug, not an algebra -- acm_gemm_shift forgets its shift while acm_bnorm_param_bwd_centred expects M_c."""

    fp32 = False
    centred = True
    bwd_shift = True
    CENTRED = ("acm_bnorm_fold_centred", "acm_linear_fwd_shift", "acm_gemm_shift", "acm_bnorm_param_bwd_centred")

    def __getattribute__(self, name):
        if name in StackFakeLib.CENTRED and not object.__getattribute__(self, "centred"):
            raise AttributeError(name)
        return object.__getattribute__(self, name)

    @property
    def _f(self):
        return np.float32 if self.fp32 else np.float64

    def _mm(self, a, b):
        return matmul(a.astype(self._f), b.astype(self._f))

    def acm_gemm(self, ta, tb, m, n, k, a, lda, b, ldb, c, ldc, relu, ws, wsb, stream):
        if not self.fp32:
            return super().acm_gemm(ta, tb, m, n, k, a, lda, b, ldb, c, ldc, relu, ws, wsb, stream)
        A = _view(a, k, m, lda).T if ta else _view(a, m, k, lda)
        B = _view(b, n, k, ldb).T if tb else _view(b, k, n, ldb)
        out = self._mm(A, B)
        _view(c, m, n, ldc)[...] = np.maximum(out, 0) if relu else out
        return 0

    def acm_gemm_shift(self, ta, tb, m, n, k, a, lda, b, ldb, shift, c, ldc, ws, wsb, stream):
        if not ta or tb:
            self._err = b"acm_gemm_shift: the shifted operand exists for A^T (B - 1 shift^T) only"
            return 4
        B = _view(b, k, n, ldb).astype(self._f)
        if self.bwd_shift:
            B = B - _vec(shift, n).astype(self._f)[None, :]
        _view(c, m, n, ldc)[...] = self._mm(_view(a, k, m, lda).T, B)
        return 0

    def _linear(self, n, f_in, f_out, X, w, ldw, bias, relu, drop, y, ldy):
        out = self._mm(X, _view(w, f_out, f_in, ldw).T)
        if bias:
            out = out + _vec(bias, f_out).astype(self._f)[None, :]
        if relu:
            out = np.maximum(out, 0)
        _view(y, n, f_out, ldy)[...] = out * dropout_factors(self._drop_obj(drop), n, f_out).astype(self._f)
        return 0

    def acm_linear_fwd(self, n, f_in, f_out, x, ldx, w, ldw, bias, relu, drop, y, ldy, ws, wsb, stream):
        if not self.fp32:
            return super().acm_linear_fwd(n, f_in, f_out, x, ldx, w, ldw, bias, relu, drop, y, ldy, ws, wsb, stream)
        return self._linear(n, f_in, f_out, _view(x, n, f_in, ldx), w, ldw, bias, relu, drop, y, ldy)

    def acm_linear_fwd_shift(self, n, f_in, f_out, x, ldx, shift, w, ldw, bias, relu, drop, y, ldy, ws, wsb, stream):
        X = _view(x, n, f_in, ldx).astype(self._f) - _vec(shift, f_in).astype(self._f)[None, :]
        return self._linear(n, f_in, f_out, X, w, ldw, bias, relu, drop, y, ldy)

    def acm_bnorm_stats_workspace_bytes(self, n, f, out):
        if not 1 <= f <= 256:
            self._err = b"acm_bnorm_stats: f outside 1..256"
            return 4
        out._obj.value = 64
        return 0

    def acm_bnorm_stats(self, n, f, h, ldh, gamma, beta, eps, momentum, train, rm, rv, nbt, stats, ws, wsb, stream):
        out = _view(stats, 4, f, f)
        F = self._f
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
        mu, var = mu.astype(F), var.astype(F)
        r = (1.0 / np.sqrt(var + F(eps))).astype(F)
        a = _vec(gamma, f).astype(F) * r
        out[0], out[1], out[2], out[3] = mu, r, a, _vec(beta, f).astype(F) - mu * a
        return 0

    def _fold(self, f_out, f_in, w, ldw, bias, beta, stats, wf, ldwf, bf):
        F = self._f
        st = _view(stats, 4, f_in, f_in).astype(F)
        W = _view(w, f_out, f_in, ldw).astype(F)
        _view(wf, f_out, f_in, ldwf)[...] = W * st[2][None, :]
        _vec(bf, f_out)[...] = (_vec(bias, f_out).astype(F) if bias else F(0.0)) + W @ (_vec(beta, f_in).astype(F) if beta else st[3])
        return 0

    def acm_bnorm_fold(self, f_out, f_in, w, ldw, bias, stats, wf, ldwf, bf, stream):
        return self._fold(f_out, f_in, w, ldw, bias, None, stats, wf, ldwf, bf)

    def acm_bnorm_fold_centred(self, f_out, f_in, w, ldw, bias, beta, stats, wf, ldwf, bf, stream):
        return self._fold(f_out, f_in, w, ldw, bias, beta, stats, wf, ldwf, bf)

    def _param_bwd(self, f_out, f_in, m, ldm, s, w, ldw, beta, stats, dw, lddw, d_beta, d_gamma):
        F = self._f
        mu, r, a, c = _view(stats, 4, f_in, f_in).astype(F)
        M, W = _view(m, f_out, f_in, ldm).astype(F), _view(w, f_out, f_in, ldw).astype(F)
        sv = _vec(s, f_out).astype(F)
        db = sv @ W
        _vec(d_beta, f_in)[...] = db
        if beta:                                                           # M = G^T (H - 1 mu^T)
            _view(dw, f_out, f_in, lddw)[...] = M * a[None, :] + np.outer(sv, _vec(beta, f_in).astype(F))
            _vec(d_gamma, f_in)[...] = r * (W * M).sum(0)
        else:                                                              # M = G^T H
            _view(dw, f_out, f_in, lddw)[...] = M * a[None, :] + np.outer(sv, c)
            _vec(d_gamma, f_in)[...] = r * ((W * M).sum(0) - mu * db)
        return 0

    def acm_bnorm_param_bwd(self, f_out, f_in, m, ldm, s, w, ldw, stats, dw, lddw, d_beta, d_gamma, stream):
        return self._param_bwd(f_out, f_in, m, ldm, s, w, ldw, None, stats, dw, lddw, d_beta, d_gamma)

    def acm_bnorm_param_bwd_centred(self, f_out, f_in, m, ldm, s, w, ldw, beta, stats, dw, lddw, d_beta, d_gamma, stream):
        return self._param_bwd(f_out, f_in, m, ldm, s, w, ldw, beta, stats, dw, lddw, d_beta, d_gamma)

    def acm_bnorm_bwd_workspace_bytes(self, n, f, out):
        if not 1 <= f <= 256:
            self._err = b"acm_bnorm_bwd: f outside 1..256"
            return 4
        out._obj.value = 64
        return 0

    def acm_bnorm_bwd(self, n, f, dz, lddz, h, ldh, stats, d_beta, d_gamma, keep_scale, relu, g, ldg, d_bias, ws, wsb, defer, stream):
        F = self._f
        dZ, H = _view(dz, n, f, lddz).astype(F), _view(h, n, f, ldh).astype(F)
        if stats:
            mu, r, a, _ = _view(stats, 4, f, f).astype(F)
            db, dg = _vec(d_beta, f).astype(F), _vec(d_gamma, f).astype(F)
            G = np.where(H > 0, a * (dZ - db / F(n) - (H - mu) * (r * dg / F(n))), F(0.0))
        elif relu:
            G = np.where(H > 0, dZ * F(keep_scale), F(0.0))
        elif keep_scale != 1.0:
            G = np.where(H != 0, dZ * F(keep_scale), F(0.0))
        else:
            G = dZ
        assert G.dtype == F
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
