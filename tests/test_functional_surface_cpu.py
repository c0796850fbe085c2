"""acm_gnn_amd.functional as a package: every name the project and the tests reach through it still resolves there, the kernel
timer's state has one home, and what the tests replace in the package's namespace (the device seams, ``_gather_rows``) is what
its modules call."""
import importlib
import pkgutil

import torch

import fake_lib

# dir() of the single-module functional.py this package replaced, without leading underscores -- less the three foreign modules
# that file happened to import at its top (``C`` = ctypes, ``threading``, ``torch``), which nobody reaches through it
PUBLIC = [
    "AGG_WIDE_MIN_DEGREE", "AcmConfig", "CallContext", "CsrGraph", "DeferredReductions", "DropoutState", "FilterOperators",
    "InputPipeline", "KernelTimer", "SparseFeatures", "Tape", "TapeBroken", "acm_conv", "agg_pad_width", "agg_wide_supported",
    "cast_bf16", "deferred_reductions", "deferred_reductions_as", "dropout", "eval_metrics", "eval_metrics_buffers",
    "fused_loss_tail", "gemm", "gemm_drop_supported", "gemm_split", "in_drop_supported", "input_pipeline", "masked_nll", "mm",
    "nll_loss_and_grad", "on_tape", "proj3", "proj_bwd", "proj_bwd_supported", "proj_fwd", "residual_add_linear",
    "residual_add_supported", "residual_linear", "set_kernel_timer", "spmm", "spmm_v", "tuning"]
# the private names the package's neighbours (optim.py, small.py) and the tests use
PRIVATE = ["_Timed", "_ptr_array", "_drop_spec", "_flat_views", "_stream", "_conv_route", "_ambient", "_gather_rows", "_lib",
           "_AcmAggWide", "_AcmAcmii"]
SEAMS = ("_stream", "_require_cuda", "_device_ctx")


def _modules():
    from acm_gnn_amd import functional
    subs = [importlib.import_module(m.name) for m in pkgutil.iter_modules(functional.__path__, functional.__name__ + ".")]
    assert len(subs) >= 7
    return [functional] + subs


def test_every_name_reached_from_outside_resolves_on_the_package():
    from acm_gnn_amd import functional as AF
    missing = [n for n in PUBLIC + PRIVATE if not hasattr(AF, n)]
    assert not missing, missing
    from acm_gnn_amd import _lib, tuning
    assert AF._lib is _lib and AF.tuning is tuning
    from acm_gnn_amd.functional import KernelTimer, _Timed, cast_bf16, spmm  # noqa: F401  (the ``from`` form of the same)


def test_the_kernel_timer_has_one_home(monkeypatch):
    fake_lib.install(monkeypatch)
    from acm_gnn_amd import functional as AF
    from acm_gnn_amd.functional import _launch as _timing
    asked = []

    class Timer(AF.KernelTimer):
        def wants(self, label):
            asked.append(label)
            return False                      # (nothing to record on the CPU: only whether the timer is consulted)

    t = Timer()
    AF.set_kernel_timer(t)
    try:
        assert _timing._TIMER is t
        assert AF._Timed("probe").on is False and asked == ["probe"]
        st = AF.DropoutState("cpu", seed=1)
        AF.dropout(torch.ones(8, 4), 0.5, st)                   # a launch made through the package's launch helper
        assert asked == ["probe", "dropout/8x4"]
    finally:
        AF.set_kernel_timer(None)
    assert _timing._TIMER is None
    assert AF._Timed("probe").on is False and len(asked) == 2   # no timer: nobody asked
    # the global is read where set_kernel_timer writes it: no module holds a copy of its value
    assert [m.__name__ for m in _modules() if "_TIMER" in vars(m)] == [_timing.__name__]


def test_the_test_double_replaces_every_seam(monkeypatch):
    from acm_gnn_amd import functional as AF, graph
    real = {name: getattr(graph, name) for name in SEAMS}
    mods = _modules()
    # one home: only the package's own namespace holds the three names; the modules look them up there when they launch
    holders = {name: [m.__name__ for m in mods if name in vars(m)] for name in SEAMS}
    assert all(h == ["acm_gnn_amd.functional"] for h in holders.values()), holders
    fake_lib.install(monkeypatch)
    for m in mods:
        for name, fn in real.items():
            assert all(v is not fn for v in vars(m).values()), (m.__name__, name)
    assert AF._stream() is None


def test_a_replaced_gather_rows_is_what_the_routes_call(monkeypatch):
    """tests/test_gpu_train.py counts halo exchanges by replacing ``functional._gather_rows``: every call site must see it."""
    fake_lib.install(monkeypatch)
    from acm_gnn_amd import GCN, data as D, functional as AF
    from acm_gnn_amd.distributed import make_sharded_operators
    adj, x_np, y_np, _, n = D.synthetic_dataset("tiny", seed=4)
    low, deg = D.build_filters(adj)
    ops = make_sharded_operators(low, deg, torch.device("cpu"))
    torch.manual_seed(2)
    model = GCN(x_np.shape[1], 64, int(y_np.max()) + 1, 2, n, 0.3, "acmgcnp", 0, variant=False).eval()
    calls, orig = [], AF._gather_rows
    monkeypatch.setattr(AF, "_gather_rows", lambda o, t: (calls.append(tuple(t.shape)), orig(o, t))[1])
    with torch.no_grad():
        model(torch.from_numpy(x_np), ops)
    assert calls
