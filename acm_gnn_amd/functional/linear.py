"""The ACM-GCN++ residual branch: dropout(relu(x W^T + b)) as autograd Functions over the acm_linear_* / acm_bias_act*
kernels, alone or added to the hidden activations in the same launch."""
import torch

from .. import _lib, tuning
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


# ---- deep mlpX stacks: Linear -> ReLU -> BatchNorm1d -> ... -> Linear (ACM-Pytorch/models/layers.py:245-285) ----------------
_ON_DEVICE = lambda t: t.is_cuda          # noqa: E731  (a CPU test double of the library with the acm_bnorm_* symbols lifts this guard)


class _StackMeta:
    """What _MlpStack needs beside its flat tensor arguments (one object: a Tape record or autograd sees no tensor in it)."""
    __slots__ = ("n_lins", "relu", "drop", "call", "buffers")

    def __init__(self, n_lins, relu, drop, call, buffers):
        # buffers: per BatchNorm (running_mean, running_var, num_batches_tracked, eps, momentum)
        self.n_lins, self.relu, self.drop, self.call, self.buffers = n_lins, relu, drop, call, buffers


def _linear_into(x, w, b, relu, spec, shift=None):
    """dropout(relu?(x W^T + b)) of a dense x (leading w.shape[1] columns) or SparseFeatures: the forward of _ResidualLinear.
    ``shift`` (dense x): x is read as x - 1 shift^T (acm_linear_fwd_shift)."""
    f_out, f_in = w.shape
    n, dev = x.shape[0], w.device
    y = torch.empty(n, f_out, dtype=_F32, device=dev)
    if isinstance(x, SparseFeatures):
        spmm_v(x.csr, x.values, w.t().contiguous(), out=y)
        launch("acm_bias_act", f"bias_act/{n}x{f_out}", dev, n, f_out, _vp(y), y.stride(0), _vp(b), int(relu), _ref(spec))
    elif shift is not None:
        ws, nbytes = _gemm_workspace(dev, 0, 1, n, f_out, f_in)
        launch("acm_linear_fwd_shift", f"linear_fwd/{n}x{f_out}x{f_in}", dev, n, f_in, f_out, _vp(x), x.stride(0), _vp(shift), _vp(w),
               w.stride(0), _vp(b), int(relu), _ref(spec), _vp(y), y.stride(0), _vp(ws), nbytes)
    else:
        ws, nbytes = _gemm_workspace(dev, 0, 1, n, f_out, f_in)
        launch("acm_linear_fwd", f"linear_fwd/{n}x{f_out}x{f_in}", dev, n, f_in, f_out, _vp(x), x.stride(0), _vp(w), w.stride(0), _vp(b),
               int(relu), _ref(spec), _vp(y), y.stride(0), _vp(ws), nbytes)
    return y


def _stack_centred():
    """Whether the library has the centred form of the stack (_lib.BNORM_CENTRED_SYMBOLS: the real one does).  A library or a
    test double without them gets the stack's first form: both products on H itself, c = beta - mu a folded into the bias."""
    lib = _lib.load()
    return all(getattr(lib, name, None) is not None for name in _lib.BNORM_CENTRED_SYMBOLS)


def _bnorm_fold(h, gamma, beta, buf, train, w_next, b_next, centred):
    """(stats [4, f] = mu | r | a | c of BatchNorm(h), W' = W_next diag(a), b'): acm_bnorm_stats (which also updates the running
    buffers when ``train``) + the fold.  ``centred``: b' = b_next + W_next beta (acm_bnorm_fold_centred), for a Linear that reads
    h - 1 mu^T; otherwise b' = b_next + W_next c (acm_bnorm_fold), for one that reads h."""
    n, f = h.shape
    dev = h.device
    rm, rv, nbt, eps, momentum = buf
    stats = torch.empty(4, f, dtype=_F32, device=dev)
    ws, nbytes = _workspace_sized(dev, "acm_bnorm_stats_workspace_bytes", n, f) if train else (None, 0)
    launch("acm_bnorm_stats", f"bnorm_stats/{n}x{f}", dev, n, f, _vp(h), h.stride(0), _vp(gamma), _vp(beta), float(eps), float(momentum),
           int(train), _vp(rm), _vp(rv), _vp(nbt), _vp(stats), _vp(ws), nbytes)
    f_out = w_next.shape[0]
    wf = torch.empty(f_out, f, dtype=_F32, device=dev)
    bf = torch.empty(f_out, dtype=_F32, device=dev)
    if centred:
        launch("acm_bnorm_fold_centred", f"bnorm_fold/{f_out}x{f}", dev, f_out, f, _vp(w_next), w_next.stride(0), _vp(b_next), _vp(beta),
               _vp(stats), _vp(wf), wf.stride(0), _vp(bf))
    else:
        launch("acm_bnorm_fold", f"bnorm_fold/{f_out}x{f}", dev, f_out, f, _vp(w_next), w_next.stride(0), _vp(b_next), _vp(stats), _vp(wf),
               wf.stride(0), _vp(bf))
    return stats, wf, bf


def _stack_forward(x, lin_params, bn_params, buffers, train, relu, spec, centred):
    """The stack's forward: H_0 = relu(x W_0^T + b_0), then per BatchNorm its statistics folded into the next Linear, which reads
    H_i - 1 mu_i^T (the mean subtracted where its product stages H_i; ``centred`` False: H_i itself).  Returns
    (y, [H_0 .. H_{L-2}], [stats_0 .. stats_{L-2}])."""
    n_lins = len(lin_params)
    w0, b0 = lin_params[0]
    h = _linear_into(x, w0, b0, True, None)
    hs, stats = [], []
    for i in range(n_lins - 1):
        gamma, beta = bn_params[i]
        w, b = lin_params[i + 1]
        st, wf, bf = _bnorm_fold(h, gamma, beta, buffers[i], train, w, b, centred)
        hs.append(h)
        stats.append(st)
        last = i + 1 == n_lins - 1
        h = _linear_into(h, wf, bf, relu if last else True, spec if last else None, shift=st[0] if centred else None)
    return h, hs, stats


class _MlpStack(torch.autograd.Function):
    """y = dropout(relu?(mlp(x))) for mlp = L >= 2 Linears with ReLU -> BatchNorm1d between them, in TRAINING mode
    (ACM-Pytorch/models/layers.py:279-284, models.py:150-152).  Arguments: x, a _StackMeta, then W_0, b_0, ..., W_{L-1}, b_{L-1},
    gamma_0, beta_0, ..., gamma_{L-2}, beta_{L-2}.  The normalised activations are never written: forward =
    per layer acm_bnorm_stats + acm_bnorm_fold_centred + acm_linear_fwd_shift on the centred ReLU output; backward = per layer one
    acm_gemm_shift(transA) for M_c = G^T (H - 1 mu^T), acm_bnorm_param_bwd_centred (dW, d_beta, d_gamma from f x f matrices), one
    acm_gemm for dZ = G W and the row-local acm_bnorm_bwd (``_stack_centred`` False: the uncentred entry points on H itself).  Only the first Linear's bias gradient honours the call's deferral list: every other column sum is read
    by the next acm_bnorm_param_bwd at once."""

    @staticmethod
    def forward(ctx, x, meta, *params):
        n_lins = meta.n_lins
        ctx.defer = meta.call.defer if meta.call is not None else None
        sparse_x = isinstance(x, SparseFeatures)
        ps = [_as_f32c(p, "parameter") for p in params]
        lin_params = [(ps[2 * i], ps[2 * i + 1]) for i in range(n_lins)]
        bn_params = [(ps[2 * n_lins + 2 * i], ps[2 * n_lins + 2 * i + 1]) for i in range(n_lins - 1)]
        f_in = lin_params[0][0].shape[1]
        if not sparse_x:
            x = _as_f32c(x, "input")
            if x.shape[1] < f_in:
                raise ValueError(f"input has {x.shape[1]} columns but the first Linear has {f_in} input features")
        if x.shape[0] < 2:
            raise ValueError(f"Expected more than 1 value per channel when training, got input size {tuple(x.shape)}")
        drop = meta.drop
        spec = _drop_spec(drop[:3], drop[3]) if drop is not None else None
        ctx.centred = _stack_centred()
        y, hs, stats = _stack_forward(x, lin_params, bn_params, meta.buffers, True, meta.relu, spec, ctx.centred)
        ctx.n_lins, ctx.relu = n_lins, bool(meta.relu)
        ctx.keep_scale = 1.0 / (1.0 - drop[0]) if (drop is not None and drop[0] > 0) else 1.0
        ctx.sparse_x = x if sparse_x else None
        ctx.save_for_backward(*([] if sparse_x else [x]), y, *hs, *stats, *[w for w, _ in lin_params], *[bt for _, bt in bn_params])
        return y

    @staticmethod
    def backward(ctx, dy):
        n_lins = ctx.n_lins
        saved = list(ctx.saved_tensors)
        x = saved.pop(0) if ctx.sparse_x is None else None
        y = saved.pop(0)
        hs, stats, ws_ = saved[:n_lins - 1], saved[n_lins - 1:2 * (n_lins - 1)], saved[2 * (n_lins - 1):3 * n_lins - 2]
        betas = saved[3 * n_lins - 2:]
        dy = _as_f32_rows(dy, "grad")
        n, dev = y.shape[0], y.device
        d_w, d_b, d_gamma, d_beta = [None] * n_lins, [None] * n_lins, [None] * (n_lins - 1), [None] * (n_lins - 1)

        def row_pass(dz, h, st, dbt, dgm, keep, relu, out, d_bias, defer, keep_alive):
            f = h.shape[1]
            ws, nbytes = _workspace_sized(dev, "acm_bnorm_bwd_workspace_bytes", n, f)
            launch("acm_bnorm_bwd", f"bnorm_bwd/{n}x{f}", dev, n, f, _vp(dz), dz.stride(0), _vp(h), h.stride(0), _vp(st), _vp(dbt), _vp(dgm),
                   float(keep), int(relu), _vp(out), out.stride(0), _vp(d_bias), _vp(ws), nbytes, defer.pointer() if defer is not None else None)
            if defer is not None:
                defer.hold(ws, [d_bias], keep=keep_alive)

        # the output epilogue: G = dY * keep / (1 - p) * [Y > 0], masks read off Y
        f_last = y.shape[1]
        g = torch.empty(n, f_last, dtype=_F32, device=dev)
        d_b[n_lins - 1] = torch.empty(f_last, dtype=_F32, device=dev)
        row_pass(dy, y, None, None, None, ctx.keep_scale, ctx.relu, g, d_b[n_lins - 1], None, None)
        flat0 = None
        for i in range(n_lins - 2, -1, -1):
            h, st, w = hs[i], stats[i], ws_[i + 1]
            f = h.shape[1]
            m = gemm(g, h, trans_a=True, b_shift=st[0] if ctx.centred else None)     # M_c = G^T (H - 1 mu^T): [f_{i+1}, f_i]
            d_w[i + 1] = torch.empty_like(w)
            d_beta[i], d_gamma[i] = torch.empty(f, dtype=_F32, device=dev), torch.empty(f, dtype=_F32, device=dev)
            launch("acm_bnorm_param_bwd_centred" if ctx.centred else "acm_bnorm_param_bwd", f"bnorm_param_bwd/{w.shape[0]}x{f}", dev, w.shape[0],
                   f, _vp(m), m.stride(0), _vp(d_b[i + 1]), _vp(w), w.stride(0), *([_vp(betas[i])] if ctx.centred else []), _vp(st), _vp(d_w[i + 1]), d_w[i + 1].stride(0), _vp(d_beta[i]), _vp(d_gamma[i]))
            dz = gemm(g, w)                                                  # [n, f_i]; becomes G_i in place
            if i == 0:
                f_in = ws_[0].shape[1]
                flat0 = torch.empty(f * f_in + f, dtype=_F32, device=dev)    # [dW_0 | db_0]
                d_w[0], d_b[0] = flat0[: f * f_in].view(f, f_in), flat0[f * f_in:]
                row_pass(dz, h, st, d_beta[i], d_gamma[i], 1.0, 1, dz, d_b[0], ctx.defer, [flat0])
            else:
                d_b[i] = torch.empty(f, dtype=_F32, device=dev)
                row_pass(dz, h, st, d_beta[i], d_gamma[i], 1.0, 1, dz, d_b[i], None, None)
            g = dz
        d_x = None
        f_in = ws_[0].shape[1]
        if ctx.sparse_x is not None:                                         # dW_0^T = X_csr^T G_0
            xs = ctx.sparse_x
            xt = xs.csr_t
            d_w[0].copy_(spmm_v(xt, xs.values.index_select(0, xt.src_pos), g).t())
        else:
            if x.shape[1] == f_in:
                gemm(g, x, trans_a=True, out=d_w[0])
            else:                                                            # zero-padded input rows (dropout(..., pad_to=...))
                d_w[0].copy_(gemm(g, x, trans_a=True)[:, :f_in])
            if ctx.needs_input_grad[0]:
                d_x = gemm(g, ws_[0])
                if d_x.shape[1] != x.shape[1]:
                    d_x = torch.nn.functional.pad(d_x, (0, x.shape[1] - d_x.shape[1]))
        grads = []
        for i in range(n_lins):
            grads += [d_w[i], d_b[i]]
        for i in range(n_lins - 1):
            grads += [d_gamma[i], d_beta[i]]
        return (d_x, None, *grads)


def _stack_modules(mlp):
    lins = list(getattr(mlp, "lins", ()))
    return lins, list(getattr(mlp, "bns", ()))[:max(len(lins) - 1, 0)]


def residual_mlp_supported(x, mlp, training):
    """The envelope of residual_mlp: >= 2 Linears (with bias, every output width <= 256) with affine, statistics-tracking,
    numeric-momentum BatchNorm1d between them, the stack's own dropout inactive; fp32 dense x (pad columns allowed) or
    SparseFeatures, everything on the device; in evaluation mode only where no gradient is taken.  ``tuning.HOST.mlp_stack = 0``
    forces the torch modules."""
    if tuning.HOST.mlp_stack <= 0:
        return False
    lins, bns = _stack_modules(mlp)
    if len(lins) < 2 or len(bns) != len(lins) - 1:
        return False
    if training and float(getattr(mlp, "dropout", 0) or 0) > 0:
        return False
    nn = torch.nn
    tensors = []
    for k, lin in enumerate(lins):
        if not isinstance(lin, nn.Linear) or lin.bias is None or lin.out_features > 256:
            return False
        if k and lin.in_features != lins[k - 1].out_features:
            return False
        tensors += [lin.weight, lin.bias]
    for bn, lin in zip(bns, lins):
        if (not isinstance(bn, nn.BatchNorm1d) or not bn.affine or not bn.track_running_stats or bn.momentum is None
                or bn.running_mean is None or bn.num_batches_tracked is None or bn.num_features != lin.out_features):
            return False
        tensors += [bn.weight, bn.bias, bn.running_mean, bn.running_var]
    if isinstance(x, SparseFeatures):
        xt = x.values
        if x.shape[1] != lins[0].in_features:
            return False
    elif isinstance(x, torch.Tensor) and x.dim() == 2 and x.layout == torch.strided and x.shape[1] >= lins[0].in_features:
        xt = x
    else:
        return False
    if xt.dtype != _F32 or not _ON_DEVICE(xt) or any(t.dtype != _F32 or t.device != xt.device for t in tensors):
        return False
    if not training and torch.is_grad_enabled() and (xt.requires_grad or any(t.requires_grad for t in tensors)):
        return False
    return True


def residual_mlp(x, mlp, relu=True, drop=None, call=None):
    """dropout(relu?(mlp(x))) for a deep Linear-ReLU-BatchNorm stack on the HIP kernels (see _MlpStack; check
    residual_mlp_supported first).  Training mode (``mlp.training``): batch statistics, the running buffers and
    ``num_batches_tracked`` updated on the device, differentiable.  Evaluation mode: the running statistics folded into the
    Linears, only the products run, no gradient.  ``drop`` / ``call`` as residual_linear."""
    if drop is not None and not drop[0] > 0:
        drop = None
    lins, bns = _stack_modules(mlp)
    buffers = [(bn.running_mean, bn.running_var, bn.num_batches_tracked, bn.eps, bn.momentum) for bn in bns]
    if not mlp.training:
        with torch.no_grad():
            if not isinstance(x, SparseFeatures):
                x = _as_f32c(x, "input")
            spec = _drop_spec(drop[:3], drop[3]) if drop is not None else None
            lp = [(_as_f32c(lin.weight, "weight"), _as_f32c(lin.bias, "bias")) for lin in lins]
            bp = [(_as_f32c(bn.weight, "weight"), _as_f32c(bn.bias, "bias")) for bn in bns]
            return _stack_forward(x, lp, bp, buffers, False, bool(relu), spec, _stack_centred())[0]
    params = [t for lin in lins for t in (lin.weight, lin.bias)] + [t for bn in bns for t in (bn.weight, bn.bias)]
    meta = _StackMeta(len(lins), bool(relu), drop, _call_or_ambient(call), buffers)
    return _run(_MlpStack, x, meta, *params)
