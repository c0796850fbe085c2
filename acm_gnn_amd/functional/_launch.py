"""How every module of this package reaches the device: the ONE launch block with its per-launch timing, the workspace query
and argument marshalling.  ``_device_ctx`` / ``_require_cuda`` / ``_stream`` -- the seams a CPU test double replaces
(tests/fake_lib.install) -- live in the package's namespace alone and are looked up there, at call time, by this module alone.
``set_kernel_timer`` rebinds ``_TIMER`` and ``_Timed`` reads it: both live here, and nobody imports the global's value."""
import ctypes as C

import torch

from .. import _lib
from .. import functional as _pkg            # (the package: home of the seams, see above)

_F32 = torch.float32
EUNSUPPORTED = 4                      # ACM_EUNSUPPORTED: "not this shape after all" -- some callers then take another form


class KernelTimer:
    """Per-launch HIP-event timing (torch.cuda.Event on the stream the kernels are launched
    on).  ``only`` restricts timing to labels that start with it, so that the events around the
    one kernel under study do not perturb the rest of a timed region.

    ``external=True``: launches made while the stream is being CAPTURED are bracketed by *external* events (event-record
    nodes of the hipGraph, added through the HIP graph API: _HipEvent): every replay re-records them, so after a replay and a synchronize
    ``captured_ms(label)`` is that kernel's duration INSIDE the replayed graph -- the time that belongs next to a
    hipGraph-replay ``ms_per_step`` (bench.py's roofline).  Without it, launches under capture are not
    timed at all (a plain event recorded in a capture cannot be read)."""

    def __init__(self, only=None, external=False):
        self.only, self.events = only, {}
        self.external, self.captured = bool(external), {}
        self.bytes = {}                 # label -> bytes this rank SENT into collectives under that label

    def wants(self, label):
        return self.only is None or label.startswith(self.only)

    def summary(self):
        """label -> (launches, total ms); synchronises."""
        torch.cuda.synchronize()
        return {k: (len(v), sum(a.elapsed_time(b) for a, b in v)) for k, v in self.events.items()}

    def captured_ms(self, label):
        """ms of every captured launch under ``label`` in the LAST replay of the graph(s) that hold them; synchronises."""
        torch.cuda.synchronize()
        return [a.elapsed_time(b) for a, b in self.captured.get(label, [])]


class _HipEvent:
    """A timing hipEvent_t recorded by an EVENT-RECORD NODE of the hipGraph the current stream is being captured into:
    hipStreamGetCaptureInfo_v2 -> hipGraphAddEventRecordNode behind the capture's current dependencies ->
    hipStreamUpdateCaptureDependencies (ROCm 7.2 rejects hipEventRecordWithFlags(hipEventRecordExternal), hipError 1,
    and torch refuses Event(external=True) on ROCm; the explicit node is what both stand for)."""
    _hip = None

    def __init__(self):
        if _HipEvent._hip is None:
            hip = C.CDLL("libamdhip64.so")
            hip.hipEventCreate.argtypes = [C.POINTER(C.c_void_p)]
            hip.hipStreamGetCaptureInfo_v2.argtypes = [C.c_void_p, C.POINTER(C.c_int), C.POINTER(C.c_ulonglong),
                                                       C.POINTER(C.c_void_p), C.POINTER(C.POINTER(C.c_void_p)),
                                                       C.POINTER(C.c_size_t)]
            hip.hipGraphAddEventRecordNode.argtypes = [C.POINTER(C.c_void_p), C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t,
                                                       C.c_void_p]
            hip.hipStreamUpdateCaptureDependencies.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_size_t, C.c_uint]
            hip.hipEventElapsedTime.argtypes = [C.POINTER(C.c_float), C.c_void_p, C.c_void_p]
            hip.hipEventDestroy.argtypes = [C.c_void_p]
            _HipEvent._hip = hip
        self.handle = C.c_void_p()
        self._check(self._hip.hipEventCreate(C.byref(self.handle)), "hipEventCreate")

    @staticmethod
    def _check(status, what):
        if status != 0:
            raise RuntimeError(f"{what} failed with hipError_t {status}")

    def record(self):
        hip, stream = self._hip, _pkg._stream()
        status, cap_id, graph = C.c_int(), C.c_ulonglong(), C.c_void_p()
        deps, n_deps = C.POINTER(C.c_void_p)(), C.c_size_t()
        self._check(hip.hipStreamGetCaptureInfo_v2(stream, C.byref(status), C.byref(cap_id), C.byref(graph), C.byref(deps),
                                                   C.byref(n_deps)), "hipStreamGetCaptureInfo_v2")
        if status.value != 1:                          # hipStreamCaptureStatusActive
            raise RuntimeError("_HipEvent.record: the current stream is not being captured")
        node = C.c_void_p()
        self._check(hip.hipGraphAddEventRecordNode(C.byref(node), graph, deps, n_deps.value, self.handle),
                    "hipGraphAddEventRecordNode")
        self._check(hip.hipStreamUpdateCaptureDependencies(stream, C.byref(node), 1, 1),     # 1 = set (replace) dependencies
                    "hipStreamUpdateCaptureDependencies")

    def elapsed_time(self, other):
        ms = C.c_float()
        self._check(self._hip.hipEventElapsedTime(C.byref(ms), self.handle, other.handle), "hipEventElapsedTime")
        return ms.value

    def __del__(self):
        hip = getattr(type(self), "_hip", None)            # (module globals are gone at interpreter shutdown)
        if self.handle and hip is not None:
            hip.hipEventDestroy(self.handle)


_TIMER = None


def set_kernel_timer(timer):
    global _TIMER
    _TIMER = timer


class _Timed:
    def __init__(self, label, nbytes=0):
        self.label = label
        self.on = _TIMER is not None and label is not None and _TIMER.wants(label)
        self.capturing = False
        if self.on and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing():
            self.capturing = True
            self.on = _TIMER.external
        if self.on and nbytes:
            _TIMER.bytes[label] = _TIMER.bytes.get(label, 0) + int(nbytes)

    def __enter__(self):
        if self.on:
            if self.capturing:
                self.a, self.b = _HipEvent(), _HipEvent()
            else:
                self.a, self.b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            self.a.record()
        return self

    def __exit__(self, *exc):
        if self.on:
            self.b.record()
            (_TIMER.captured if self.capturing else _TIMER.events).setdefault(self.label, []).append((self.a, self.b))
        return False


def launch(name, label, dev, *args, unsupported_ok=False):
    """``lib.<name>(*args, stream)`` with ``dev`` current, under one ``_Timed(label)`` (``label=None``: not timed).  A non-zero
    status raises -- except, with ``unsupported_ok``, ACM_EUNSUPPORTED, which is returned for the caller to fall back on."""
    with _pkg._device_ctx(dev), _Timed(label):
        st = getattr(_lib.load(), name)(*args, _pkg._stream())
    if st and not (unsupported_ok and st == EUNSUPPORTED):
        _lib.check(st, name)
    return st


def _workspace_bytes(query, *args, or_none=False):
    """The byte count the ``acm_*_bytes`` companion ``query`` answers for the shape ``args`` (``or_none``: None if it fails)."""
    nbytes = C.c_size_t()
    st = getattr(_lib.load(), query)(*args, C.byref(nbytes))
    if st and or_none:
        return None
    _lib.check(st, query)
    return nbytes.value


def _workspace_sized(dev, query, *args):
    """(float32 workspace of at least one float, the byte count ``query`` answered for the shape ``args``)."""
    nbytes = _workspace_bytes(query, *args)
    return torch.empty(max(nbytes // 4, 1), dtype=_F32, device=dev), nbytes


def _workspace(dev, query, *args):
    return _workspace_sized(dev, query, *args)[0]


def _capturing(dev):
    return dev.type == "cuda" and torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def _vp(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def _ref(struct):
    return C.byref(struct) if struct is not None else None


def _check_device(t, name):
    _pkg._require_cuda(t, name)


def _as_f32c(t, name):
    _pkg._require_cuda(t, name)
    if t.dtype != _F32:
        t = t.to(_F32)
    return t.contiguous()


def _as_f32_rows(t, name):
    """fp32 with unit column stride: a column slice of a wider matrix is handed to the C ABI as (pointer, ld) instead of
    being copied."""
    _pkg._require_cuda(t, name)
    if t.dtype != _F32:
        t = t.to(_F32)
    if t.dim() == 2 and t.stride(1) == 1 and t.stride(0) >= t.shape[1] and t.shape[1] > 0:
        return t
    return t.contiguous()
