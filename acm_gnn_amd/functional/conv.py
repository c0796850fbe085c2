"""The fused ACM layer's entry point: ``acm_conv`` picks the execution form of one layer (_conv_route) and runs it as that
route's autograd Function."""
import torch

from .. import tuning
from ..graph import SparseFeatures
from ._context import _call_or_ambient, _run
from ._hidden import ensure_hidden_written
from .blocks import project_blocks
from ._conv_shared import PROJECTED, _chan_block
from ._launch import _F32
from .conv_agg import _AcmAggFirst, _AcmAggWide, agg_wide_supported
from .conv_literal import _AcmAcmii, _AcmLiteral
from .ops import gemm_drop_supported


def _agg_first_shape(cfg, f_in, f_out):
    """Aggregate-first, A (X W) = (A X) W on the f_pad <= 16 kernels: legal without a ReLU between projection and filter, worth
    it when F_in < F."""
    return not cfg.relu_before and f_in <= 16 and f_in < f_out and f_out <= 64


def _acmii_shape(cfg, f_in, f_out):
    """ACMII first layer with a narrow input: gather the input rows and recompute relu(x_j [W_L | W_H]) per edge on the matrix
    pipe instead of gathering the 2F-wide projected rows (acm_conv_acmii_fwd = K1 + K2)."""
    return cfg.relu_before and not cfg.relu_after and cfg.relu_mlp and f_out == 64 and f_in <= 8


def _conv_route(x, ops, cfg, f_in, f_out, post_scale=None, call=None, tail_layer=False):
    """The execution form of one ACM layer: "wide" (_AcmAggWide), "agg" (_AcmAggFirst), "acmii" (_AcmAcmii) or "literal"
    (_AcmLiteral).  Aggregate-first needs an input that takes no gradient (its backward runs no SpMM); the k-hop chain, general
    operator pairs and CSR features take the literal form; tuning rewrites bits 1 / 2 switch the two narrow rewrites off."""
    if agg_wide_supported(x, ops, cfg, f_in, f_out, post_scale, call, tail_layer):
        return "wide"
    hops = int(getattr(ops, "hops", 1))
    if isinstance(x, SparseFeatures) or getattr(ops, "general", False) or hops > 1:
        return "literal"
    rewrites = tuning.HOST.rewrites
    if (_agg_first_shape(cfg, f_in, f_out) and not (isinstance(x, torch.Tensor) and x.requires_grad)
            and rewrites & tuning.REWRITE_AGG_FIRST):
        return "agg"
    if _acmii_shape(cfg, f_in, f_out) and hops == 1 and rewrites & tuning.REWRITE_ACMII_RECOMPUTE:
        return "acmii"
    return "literal"


def in_drop_supported(x, ops, cfg, f_in, f_out):
    """Whether a layer can take its caller's input dropout into its dense projection (acm_conv ``in_drop``): the
    literal form on the MFMA GEMM (not aggregate-first, not the narrow streaming projection, not CSR features), an input
    that needs no gradient, shapes the row-panel GEMMs cover.  (By shape alone, whatever the tuning switches say: a layer
    then takes the same launches under any of them.)"""
    if isinstance(x, SparseFeatures) or not isinstance(x, torch.Tensor) or x.requires_grad or x.dim() != 2:
        return False
    if x.shape[1] != f_in or x.dtype != _F32 or not x.is_contiguous():
        return False
    narrow = f_out <= 5 and f_in <= 64
    if _agg_first_shape(cfg, f_in, f_out) or _acmii_shape(cfg, f_in, f_out) or narrow or f_out in (2, 4, 8):
        return False
    fb = _chan_block(f_out)
    return gemm_drop_supported(x.shape[0], f_in, 2 * fb + f_out)


_ROUTES = {"wide": _AcmAggWide, "agg": _AcmAggFirst, "acmii": _AcmAcmii, "literal": _AcmLiteral}


def acm_conv(x, params, ops, cfg, post_relu=False, post_scale=None, post_drop=None, call=None, tail_layer=False,
             agg_holder=None, in_drop=None):
    """params: dict with the reference's parameter names (see layers.GraphConvolution).
    post_relu / post_scale: optional fused ``relu(out) * post_scale`` (the caller's inter-layer
    ReLU + dropout; post_scale = keep_mask / (1 - p)).  post_drop = (p, tag, DropoutState): the same
    dropout with the mask generated in registers (acm_dropout_t) instead of read from a tensor.
    call: the model call's CallContext (default: the thread's ambient one); tail_layer: the caller is an output layer without
    post-op working in the operator's numbering (it may take call.tail); agg_holder: layers.GraphConvolution's {"agg": P-or-None}
    of a pass over a static input; in_drop = (p, tag, DropoutState): the caller's input dropout, left to this layer
    (in_drop_supported).  The layer runs as the autograd Function of its route (_conv_route).  ``x`` may be a list / tuple of
    column blocks standing for their concatenation (functional.blocks.project_blocks): the literal route then."""
    p = params
    if isinstance(x, (list, tuple)):
        # column blocks [x | h_0 | ...] (ACM-Snowball): their projection without the concatenation (functional.blocks), adopted by
        # the literal layer, whose backward hands dZ back to the projection's
        if ops.sharded:
            raise NotImplementedError("row-sharded operators with a block input are out of scope: concatenate the blocks, or "
                                      "run the block input on one device")
        if in_drop is not None:
            raise NotImplementedError("in_drop with a block input: the caller applies the dropout to the feature block")
        call = _call_or_ambient(call)
        x = project_blocks(x, (p["weight_low"], p["weight_high"], p["weight_mlp"]), relu=cfg.relu_before, call=call, mask_grad=False)
        fn, agg_holder, pregathered = _AcmLiteral, None, PROJECTED
    else:
        fn = _ROUTES[_conv_route(x, ops, cfg, p["weight_low"].shape[0], p["weight_low"].shape[1], post_scale, call, tail_layer)]
        pregathered = getattr(ops, "_pregathered", None)                          # one-shot hand-over from models.GCN
        if fn is not _AcmLiteral:                 # (the literal route knows how to leave an unwritten hidden activation unread)
            ensure_hidden_written(call, x)
        if call is not None:
            call.grad_enabled = torch.is_grad_enabled()
    ops._pregathered = None
    return _run(
        fn, x, p["weight_low"], p["weight_high"], p["weight_mlp"], p["att_vec_low"], p["att_vec_high"],
        p["att_vec_mlp"], p["att_struc_low"], p["struc_low"], p["att_vec"],
        p["layer_norm_low.weight"], p["layer_norm_high.weight"], p["layer_norm_mlp.weight"],
        p["layer_norm_struc_low.weight"], p["layer_norm_low.bias"], p["layer_norm_high.bias"],
        p["layer_norm_mlp.bias"], p["layer_norm_struc_low.bias"], ops, cfg, post_relu, post_scale, post_drop,
        call, tail_layer, agg_holder, in_drop, pregathered)
