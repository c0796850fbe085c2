"""Operator-level host code: thin wrappers over the C ABI and the autograd
Functions that make the HIP kernels differentiable.

Every function here launches HIP kernels from libacm_hip.so on the current
torch stream.  There is deliberately no eager/torch fallback: a CPU tensor or a
missing library is an error.

Beside the three device seams (``_device_ctx`` / ``_require_cuda`` / ``_stream``: ``_launch`` looks them up HERE at call
time, so that a test double replaces them in one place) and ``_gather_rows`` (the routes call it through this namespace, where
a test counts halo exchanges), this file only re-exports what the project and the tests reach as ``functional.NAME``: ``_launch`` (the launch block, its
timing and argument marshalling), ``_context`` (step- and call-scoped state), ``_hidden`` (the hand-off between a hidden layer and the layer after it), ``ops`` (single-kernel operators), ``select`` (a run's selection state on the device), ``linear`` (the
residual branch), ``gcn`` (the one-channel layers of the study's baselines), ``blocks`` (the projection of a block input), ``conv`` (the layer's entry point) over ``_conv_shared``, ``conv_agg`` and ``conv_literal`` (its four routes).
"""
from .. import _lib, tuning  # noqa: F401
from ..graph import CsrGraph, FilterOperators, SparseFeatures, _device_ctx, _require_cuda, _stream  # noqa: F401  (the seams)
from ._launch import KernelTimer, _Timed, set_kernel_timer  # noqa: F401
from ._context import (CallContext, DeferredReductions, InputPipeline, Tape, TapeBroken, _ambient, deferred_reductions,  # noqa: F401
                       deferred_reductions_as, fused_loss_tail, input_pipeline, on_tape)
from ._hidden import HiddenLink, HiddenToken, ProjRequest, ensure_hidden_written, hidden_elision_why_not, lazy_hidden_why_not  # noqa: F401
from .ops import (DropoutState, _drop_spec, agg_pad_width, bce_loss, bce_loss_and_grad, cast_bf16, dropout, eval_metrics,  # noqa: F401
                  eval_metrics_buffers, eval_rocauc, gemm, gemm_drop_supported, gemm_split, masked_bce, masked_nll, mm, nll_loss_and_grad, proj3, proj_bwd,
                  proj_bwd_supported, proj_fwd, rocauc_buffers, spmm, spmm_v)
from .select import BatchMetrics, BatchSelection, SelectionState, copy_if  # noqa: F401
from .linear import residual_add_linear, residual_add_supported, residual_linear, residual_mlp, residual_mlp_supported  # noqa: F401
from .gcn import aggregate, dense_act, gcn_bwd, gcn_fwd, gcn_two_layer, gemm_act, low_t_product, mask_bwd, sparse_mm  # noqa: F401
from ._conv_shared import AcmConfig, _flat_views, _gather_rows, _ptr_array  # noqa: F401
from .conv_agg import AGG_WIDE_MIN_DEGREE, _AcmAggWide, agg_wide_supported  # noqa: F401
from .conv_literal import _AcmAcmii  # noqa: F401
from .blocks import check_blocks, project_blocks  # noqa: F401
from .conv import _conv_route, acm_conv, in_drop_supported  # noqa: F401
