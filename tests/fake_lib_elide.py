"""The test double's eliding branch: acm_conv_agg_out_optional, and acm_conv_agg_fwd / acm_conv_agg_bwd with ``out == NULL`` as
include/acm_hip.h states them, patched onto fake_lib.FakeLib -- whose own lack of the query symbol
(test_elide_hidden_cpu.py) stands for a library older than the entry point.  TEST DOUBLE, CPU suite only."""
import ctypes as C

import numpy as np

import fake_lib
from fake_lib import _head, _post_fwd, _view

_FWD, _BWD = fake_lib.FakeLib.acm_conv_agg_fwd, fake_lib.FakeLib.acm_conv_agg_bwd


def acm_conv_agg_out_optional(self, pp, n_rows, proj_f):
    """1 where the forward takes ``out == NULL`` and, with proj_f > 0, the backward that carries proj_dz does; launches nothing."""
    p = getattr(pp, "_obj", None)
    if p is None or n_rows < 0 or proj_f < 0:
        return 0
    ok = bool(p.agg_given) and p.n_channels == 3 and p.f_out == 64 and p.next_f > 0 and bool(p.next_zlh)
    if ok and proj_f > 0:
        ok = (p.f_pad == 8 and bool(p.post_relu) and not p.post_scale and bool(p.head_stats) and 1 <= proj_f <= 2
              and proj_f == p.next_f and (self._tuning["rows16"] & 2) != 0)
    return int(ok)


def _with_out(block, out):
    r = type(block).from_buffer_copy(block)
    r.out, r.ld_out = out.ctypes.data, out.shape[1]
    return r


def acm_conv_agg_fwd(self, h, pp, ws, wsb, stream):
    """``out == NULL``: the row is formed as ever and goes to next_zlh / next_zi only; nothing is stored through p.out."""
    p = pp._obj
    if p.out:
        return _FWD(self, h, pp, ws, wsb, stream)
    n = self._get(h).n_rows
    if not acm_conv_agg_out_optional(self, pp, n, 0):
        self._err = b"acm_conv_agg_fwd: out == NULL outside acm_conv_agg_out_optional"
        return 1
    row = np.empty((n, p.f_out), np.float32)                # (alive until the call returns: the block holds its address only)
    return _FWD(self, h, C.byref(_with_out(p, row)), ws, wsb, stream)


def acm_conv_agg_bwd(self, n, qq, ws, wsb, stream):
    """``out == NULL`` with proj_dz: the row (the projection gradient's operand; its post-op mask is the forward's by
    construction) is formed again by the forward's expression instead of read."""
    q = qq._obj
    if q.out or not q.proj_dz or q.n_channels != 3:
        return _BWD(self, n, qq, ws, wsb, stream)
    k = 3
    F, fi, fp, x, W = self._agg_common(q, n)
    P = _view(q.agg, n, fp, q.ld_agg).astype(np.float64)[:, :fi]
    raw = [P @ W[0], (x - P) @ W[1], x @ W[2]]
    H = [np.maximum(r, 0) if f else r for r, f in zip(raw, (q.relu_after, q.relu_after, q.relu_mlp))]
    hd = _head(H, k, q.layernorm, *self._params(q, k, F, q.layernorm))
    row = np.ascontiguousarray(_post_fwd(q, q.scale * sum(hd["alpha"][:, c:c + 1] * H[c] for c in range(k)), n, F), dtype=np.float32)
    return _BWD(self, n, C.byref(_with_out(q, row)), ws, wsb, stream)      # (_bwd16_ok sees the row)


def install(monkeypatch):
    """fake_lib.install with the eliding branch on the double."""
    monkeypatch.setattr(fake_lib.FakeLib, "acm_conv_agg_out_optional", acm_conv_agg_out_optional, raising=False)
    monkeypatch.setattr(fake_lib.FakeLib, "acm_conv_agg_fwd", acm_conv_agg_fwd)
    monkeypatch.setattr(fake_lib.FakeLib, "acm_conv_agg_bwd", acm_conv_agg_bwd)
    return fake_lib.install(monkeypatch)
