"""The test double's acm_proj_blocks_* entry points (include/acm_hip.h): float64 arithmetic on host pointers, added to
fake_lib.FakeLib by ``install`` before the double is put in place.  TEST DOUBLE, CPU suite only."""
import ctypes as C

import numpy as np

import fake_lib
from fake_lib import _view


def _blocks(p):
    p = p._obj if hasattr(p, "_obj") else p
    return p, [(j, int(p.width[j]), int(p.row0[j])) for j in range(p.n_blocks)]


def _shapes_ok(self, p, who):
    if any(p.row0[j] < 0 or p.row0[j] + p.width[j] > p.f_in for j in range(p.n_blocks)):
        self._err = who.encode() + b": rows beyond the weights"
        return False
    return True


def _supported(self, p, who):
    if p.n_blocks > 8 or not 1 <= p.f <= 64 or any(p.width[j] % 4 or not 4 <= p.width[j] <= 64 for j in range(p.n_blocks)):
        self._err = who.encode() + b": outside the envelope"
        return False
    return True


def _weights(p, r0, w):
    """[W_L | W_H | W_I][r0 : r0 + w] as float64 [w, 3 f]."""
    return np.concatenate([_view(wc, r0 + w, p.f, p.ldw)[r0:].astype(np.float64) for wc in (p.w_low, p.w_high, p.w_mlp)], 1)


def _channels(table, f, fb):
    return [table[:, c * fb:c * fb + f] for c in range(3)]


def acm_proj_blocks_fwd(self, n, p, z, ldz, accumulate, relu, stream):
    p, blocks = _blocks(p)
    if not _shapes_ok(self, p, "acm_proj_blocks_fwd"):
        return 2
    if not _supported(self, p, "acm_proj_blocks_fwd"):
        return 4
    f, fb = p.f, p.f_block
    zv = _view(z, n, 2 * fb + f, ldz)
    total = np.zeros((n, 3 * f))
    if accumulate:
        total += np.concatenate([c.astype(np.float64) for c in _channels(zv, f, fb)], 1)
    for j, w, r0 in blocks:
        total += _view(p.h[j], n, w, p.ld_h[j]).astype(np.float64) @ _weights(p, r0, w)
    if relu:
        total = np.maximum(total, 0)
    if not accumulate:
        zv[...] = 0
    for c, dst in enumerate(_channels(zv, f, fb)):
        dst[...] = total[:, c * f:(c + 1) * f]
    return 0


def acm_proj_blocks_bwd_workspace_bytes(self, n, p, out):
    p, _ = _blocks(p)
    if not _shapes_ok(self, p, "acm_proj_blocks_bwd"):
        return 2
    if not _supported(self, p, "acm_proj_blocks_bwd"):
        return 4
    out._obj.value = 16
    return 0


def acm_proj_blocks_bwd(self, n, p, dz, lddz, dw, lddw, cb, cbs, ws, wsb, defer, stream):
    p, blocks = _blocks(p)
    if not _shapes_ok(self, p, "acm_proj_blocks_bwd"):
        return 2
    if not _supported(self, p, "acm_proj_blocks_bwd"):
        return 4
    f, fb = p.f, p.f_block
    g = np.concatenate([c.astype(np.float64) for c in _channels(_view(dz, n, 2 * fb + f, lddz), f, fb)], 1)
    base = dw.value if isinstance(dw, C.c_void_p) else int(dw)
    writes = []
    for j, w, r0 in blocks:
        h = _view(p.h[j], n, w, p.ld_h[j]).astype(np.float64)
        if p.d_h[j]:
            _view(p.d_h[j], n, w, p.ld_dh[j])[...] = g @ _weights(p, r0, w).T
        rows = h.T @ g
        at = base + 4 * r0 * lddw
        if not cb:
            writes.append((_view(at, w, 3 * f, lddw), rows))
        else:
            for c, q0 in enumerate(range(0, 3 * f, cb)):
                wd = min(cb, 3 * f - q0)
                writes.append((_view(at + 4 * c * cbs, w, wd, lddw), rows[:, q0:q0 + wd]))
    return self._emit(defer, writes)


def install(monkeypatch):
    """fake_lib.install with the block projection's entry points on the double."""
    for fn in (acm_proj_blocks_fwd, acm_proj_blocks_bwd_workspace_bytes, acm_proj_blocks_bwd):
        monkeypatch.setattr(fake_lib.FakeLib, fn.__name__, fn, raising=False)
    return fake_lib.install(monkeypatch)
