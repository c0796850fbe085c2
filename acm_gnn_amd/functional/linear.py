"""The ACM-GCN++ residual branch: dropout(relu(x W^T + b)) as autograd Functions over the acm_linear_* / acm_bias_act*
kernels, alone or added to the hidden activations in the same launch."""
import torch

from ..graph import SparseFeatures
from ._context import _call_or_ambient, _run, _sum_over_ranks
from ._launch import _F32, _as_f32_rows, _as_f32c, _ref, _vp, _workspace_sized, launch
from .ops import _drop_spec, _gemm_workspace, gemm, spmm_v


class _ResidualLinear(torch.autograd.Function):
    """y = dropout(relu(x W^T + b)) (ACM-Geometric/models.py:26-27,55-56): dense x through acm_linear_fwd (bias / ReLU /
    counter-based dropout in the GEMM epilogue), CSR features through acm_spmm_v + acm_bias_act.  Backward:
    acm_bias_act_bwd (masks read off y), then dW = G^T x; row-sharded runs sum [dW | db] over the ranks."""

    @staticmethod
    def forward(ctx, x, weight, bias, relu, drop, group, call=None, pipe=None):
        ctx.defer = call.defer if call is not None else None
        # ``pipe``: x is the input pipeline's table (InputPipeline.local_table()), which the first layer's forward refills
        # with the NEXT step's dropped input once it has adopted it -- this step's rows are then in pipe.saved[0]
        ctx.pipe = pipe
        sparse_x = isinstance(x, SparseFeatures)
        w = _as_f32c(weight, "weight")
        b = _as_f32c(bias, "bias") if bias is not None else None
        f_out, f_in = w.shape
        n = x.shape[0]
        dev = w.device
        y = torch.empty(n, f_out, dtype=_F32, device=dev)
        spec = _drop_spec(drop[:3], drop[3]) if drop is not None else None
        if sparse_x:
            spmm_v(x.csr, x.values, w.t().contiguous(), out=y)
            launch("acm_bias_act", f"bias_act/{n}x{f_out}", dev, n, f_out, _vp(y), y.stride(0), _vp(b), int(relu), _ref(spec))
        else:
            x = _as_f32c(x, "input")
            if x.shape[1] < f_in:
                raise ValueError(f"input has {x.shape[1]} columns but the Linear has {f_in} input features")
            ws, nbytes = _gemm_workspace(dev, 0, 1, n, f_out, f_in)
            launch("acm_linear_fwd", f"linear_fwd/{n}x{f_out}x{f_in}", dev, n, f_in, f_out, _vp(x), x.stride(0), _vp(w), w.stride(0), _vp(b),
                   int(relu), _ref(spec), _vp(y), y.stride(0), _vp(ws), nbytes)
        ctx.relu, ctx.group, ctx.has_bias = bool(relu), group, b is not None
        ctx.keep_scale = 1.0 / (1.0 - drop[0]) if (drop is not None and drop[0] > 0) else 1.0
        ctx.sparse_x = x if sparse_x else None
        ctx.save_for_backward(w if sparse_x else x, w, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        if ctx.pipe is not None and ctx.pipe.adopted:
            x = ctx.pipe.saved[0]                 # (the table itself holds step t + 1's rows by now)
        dy = _as_f32c(dy, "grad")
        n, f_out = y.shape
        f_in = w.shape[1]
        dev = y.device
        flat = torch.empty(f_out * f_in + f_out, dtype=_F32, device=dev)      # [dW | db]: one all-reduce when sharded
        d_w, d_b = flat[: f_out * f_in].view(f_out, f_in), flat[f_out * f_in:]
        if ctx.sparse_x is None and not ctx.needs_input_grad[0] and f_in <= 16 and f_out <= 256:
            # a narrow dense input that takes no gradient (the raw features): dW and db in ONE pass over (y, dy, x), the
            # [n, f_out] matrix G = dL/d(pre-activation) never stored (acm_linear_bwd)
            ws, nbytes = _workspace_sized(dev, "acm_linear_bwd_workspace_bytes", n, f_in, f_out)
            launch("acm_linear_bwd", f"linear_bwd/{n}x{f_out}x{f_in}", dev, n, f_in, f_out, _vp(x), x.stride(0), _vp(y), y.stride(0), _vp(dy),
                   dy.stride(0), float(ctx.keep_scale), int(ctx.relu), _vp(d_w), f_in, _vp(d_b), _vp(ws), nbytes,
                   ctx.defer.pointer() if ctx.defer is not None else None)
            if ctx.defer is not None:
                ctx.defer.hold(ws, [d_w, d_b], keep=[flat, x, y, dy])
            if ctx.group is not None:
                _sum_over_ranks(flat, ctx.group, ctx.defer)
            return None, d_w, (d_b if ctx.has_bias else None), None, None, None, None, None
        g = torch.empty(n, f_out, dtype=_F32, device=dev)
        ws, nbytes = _workspace_sized(dev, "acm_bias_act_bwd_workspace_bytes", n, f_out)
        launch("acm_bias_act_bwd", f"bias_act_bwd/{n}x{f_out}", dev, n, f_out, _vp(y), y.stride(0), _vp(dy), dy.stride(0), float(ctx.keep_scale),
               int(ctx.relu), _vp(g), g.stride(0), _vp(d_b), _vp(ws), nbytes, ctx.defer.pointer() if ctx.defer is not None else None)
        if ctx.defer is not None:
            ctx.defer.hold(ws, [d_b], keep=[flat])
        d_x = None
        if ctx.sparse_x is not None:                          # dW^T = X_csr^T G
            xs = ctx.sparse_x
            xt = xs.csr_t
            d_w.copy_(spmm_v(xt, xs.values.index_select(0, xt.src_pos), g).t())
        else:
            if x.shape[1] == f_in:
                gemm(g, x, trans_a=True, out=d_w)
            else:                                             # zero-padded input rows (dropout(..., pad_to=...))
                d_w.copy_(gemm(g, x, trans_a=True)[:, :f_in])
            if ctx.needs_input_grad[0]:
                d_x = gemm(g, w)
                if d_x.shape[1] != x.shape[1]:
                    d_x = torch.nn.functional.pad(d_x, (0, x.shape[1] - d_x.shape[1]))
        if ctx.group is not None:
            _sum_over_ranks(flat, ctx.group, ctx.defer)
        return d_x, d_w, (d_b if ctx.has_bias else None), None, None, None, None, None


class _ResidualAddLinear(torch.autograd.Function):
    """out = fea + dropout(relu(x W^T + b)) in ONE launch (acm_linear_fwd_add: the ACM-GCN++ hidden activations fea1 + xX,
    ACM-Geometric/models.py:55-56,73) for a narrow dense x that takes no gradient; the backward recomputes both masks
    (acm_linear_bwd_recompute: reads dY and x only) and hands dY through to fea."""

    @staticmethod
    def forward(ctx, fea, x, weight, bias, relu, drop, group, call):
        ctx.defer = call.defer if call is not None else None
        fea, x = _as_f32_rows(fea, "fea"), _as_f32c(x, "input")
        w = _as_f32c(weight, "weight")
        b = _as_f32c(bias, "bias") if bias is not None else None
        f_out, f_in = w.shape
        n, dev = x.shape[0], w.device
        out = torch.empty(n, f_out, dtype=_F32, device=dev)
        spec = _drop_spec(drop[:3], drop[3]) if drop is not None else None
        launch("acm_linear_fwd_add", f"linear_fwd_add/{n}x{f_out}x{f_in}", dev, n, f_in, f_out, _vp(x), x.stride(0), _vp(w), w.stride(0), _vp(b),
               int(relu), _ref(spec), _vp(fea), fea.stride(0), _vp(out), out.stride(0))
        ctx.relu, ctx.group, ctx.has_bias, ctx.spec = bool(relu), group, b is not None, spec
        ctx.save_for_backward(x, w, b if b is not None else w.new_zeros(0))
        return out

    @staticmethod
    def backward(ctx, dy):
        x, w, b = ctx.saved_tensors
        dy = _as_f32_rows(dy, "grad")
        f_out, f_in = w.shape
        n, dev = x.shape[0], w.device
        flat = torch.empty(f_out * f_in + f_out, dtype=_F32, device=dev)      # [dW | db]: one all-reduce when sharded
        d_w, d_b = flat[: f_out * f_in].view(f_out, f_in), flat[f_out * f_in:]
        ws, nbytes = _workspace_sized(dev, "acm_linear_bwd_workspace_bytes", n, f_in, f_out)
        launch("acm_linear_bwd_recompute", f"linear_bwd_recompute/{n}x{f_out}x{f_in}", dev, n, f_in, f_out, _vp(x), x.stride(0), _vp(w),
               w.stride(0), _vp(b) if ctx.has_bias else None, int(ctx.relu), _ref(ctx.spec), _vp(dy), dy.stride(0), _vp(d_w), f_in, _vp(d_b),
               _vp(ws), nbytes, ctx.defer.pointer() if ctx.defer is not None else None)
        if ctx.defer is not None:
            ctx.defer.hold(ws, [d_w, d_b], keep=[flat, x, dy])
        if ctx.group is not None:
            _sum_over_ranks(flat, ctx.group, ctx.defer)
        return dy, None, d_w, (d_b if ctx.has_bias else None), None, None, None, None


def residual_add_supported(x, weight):
    """Shapes acm_linear_fwd_add / acm_linear_bwd_recompute take: a dense input of <= 16 columns that needs no gradient,
    <= 256 outputs."""
    return (isinstance(x, torch.Tensor) and not x.requires_grad and x.dim() == 2 and weight.shape[1] <= 16
            and weight.shape[1] <= x.shape[1] and weight.shape[0] <= 256)


def residual_add_linear(fea, x, weight, bias, relu=True, drop=None, group=None, call=None):
    """fea + dropout(relu(x @ weight.T + bias)) as one launch, masks recomputed in the backward (see _ResidualAddLinear);
    arguments as residual_linear."""
    if drop is not None and not drop[0] > 0:
        drop = None
    return _run(_ResidualAddLinear, fea, x, weight, bias, bool(relu), drop, group, _call_or_ambient(call))


def residual_linear(x, weight, bias, relu=True, drop=None, group=None, call=None, pipe=None):
    """dropout(relu(x @ weight.T + bias)) on the HIP kernels.  ``drop = (p, tag, DropoutState, row_offset)`` draws the
    counter-based mask in the epilogue; ``group``: row-sharded run (the parameter gradients are summed over it);
    ``call``: the model call's CallContext (its deferral list; default: the thread's ambient one); ``pipe``: x is the
    table of that InputPipeline (the backward then reads this step's rows from its saved copy once the first layer's forward
    has refilled the table)."""
    if drop is not None and not drop[0] > 0:
        drop = None
    return _run(_ResidualLinear, x, weight, bias, bool(relu), drop, group, _call_or_ambient(call), pipe)
