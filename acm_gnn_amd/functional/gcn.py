"""The one-channel graph layers of the synthetic study's baselines (synthetic-experiments/baseline_models: gcn, sgc, mlp) over
acm_gcn_fwd / acm_gcn_bwd / acm_gemm_act: raw launches and the autograd Functions ``baselines.GCN`` is made of.

Every op takes ``fused=True``.  Its ``False`` arm computes the same thing from the entry points that existed before
(acm_spmm_ex, acm_bias_act, acm_gemm, acm_bias_act_bwd): the comparison arm of scripts/bench_baselines.py and of the tests."""
import ctypes as C

import torch

from .. import _lib
from ..graph import SparseFeatures
from ._context import _call_or_ambient, _run
from ._launch import _F32, _as_f32_rows, _as_f32c, _ref, _vp, _workspace_sized, launch
from .ops import _drop_spec, _gemm_workspace, gemm, spmm, spmm_v

NEXT_MAX = 8            # columns of the projection acm_gcn_fwd takes along; also the widest dY of acm_gcn_bwd
MASK_MAX = 256          # acm_bias_act_bwd's column budget (the comparison arm, and the hidden layer of mlp)
# Work items up to which the fused arm is the two-layer model's default.  Measured per captured gcn step (EXPERIMENTS.md, "Baselines
# of the synthetic study"): at 2 000 rows the fused arm is the faster one, at 168 114 rows the composed arm -- so above this many
# work items the WHOLE step takes the composed arm, the one that measured faster there.  Nothing was measured in between; the
# switch sits where acm_gcn_bwd's grid cap (256 blocks x 32 groups) starts to bind.  ``fused="always"`` forces the fused arm
# (scripts/bench_baselines.py); the raw ops below do what their ``fused`` says at any size.
FUSE_MAX_ITEMS = 8192


def fusion_pays(graph):
    return graph.n_items <= FUSE_MAX_ITEMS


def resolve_fused(fused, graph):
    """``True``: fused where it measured faster; ``"always"``: fused; ``False``: composed."""
    return True if fused == "always" else (bool(fused) and fusion_pays(graph))


# ---- raw launches ----
def gemm_act(x, w, relu=False, drop=None, out=None):
    """out = dropout(relu?(x @ w)) for w stored [f_in, f_out]: ReLU and the counter-based mask of ``drop`` (an acm_dropout_t or
    None) in the product's epilogue (acm_gemm_act)."""
    x, w = _as_f32_rows(x, "x"), _as_f32_rows(w, "w")
    n, k = x.shape
    if w.shape[0] != k:
        raise ValueError(f"gemm_act: inner dimensions differ ({k} vs {w.shape[0]})")
    f = w.shape[1]
    if out is None:
        out = torch.empty(n, f, dtype=_F32, device=x.device)
    ws, nbytes = _gemm_workspace(x.device, 0, 0, n, f, k)
    launch("acm_gemm_act", f"gemm_act/{n}x{f}x{k}", x.device, n, k, f, _vp(x), x.stride(0), _vp(w), w.stride(0), int(relu), _ref(drop),
           _vp(out), out.stride(0), _vp(ws), nbytes)
    return out


def gcn_fwd(graph, z, row_scale=None, relu=False, drop=None, w_next=None, fused=True, out=None, out_next=None):
    """(y, z_next): y = dropout(relu?(diag(row_scale) (A @ z))) for a CsrGraph A, and -- ``w_next`` [width, f_next] given --
    z_next = y @ w_next.  One launch (acm_gcn_fwd) where f_next <= 8 and 8 < width <= 256, the projection a GEMM behind it
    otherwise; without a post-op acm_gcn_fwd is acm_spmm_ex; a post-op on at most 8 columns is composed (the entry point refuses
    it: see acm_hip.h).  ``out`` / ``out_next``: fp32 buffers with unit column stride (any row pitch).  ``fused=False``: acm_spmm_ex +
    acm_bias_act (+ acm_gemm)."""
    z = _as_f32_rows(z, "z")
    if z.shape[0] != graph.n_cols:
        raise ValueError(f"gcn_fwd: z has {z.shape[0]} rows, the operator has {graph.n_cols} columns")
    n, width, dev = graph.n_rows, z.shape[1], z.device
    y = torch.empty(n, width, dtype=_F32, device=dev) if out is None else out
    f_next, z_next = 0, None
    if w_next is not None:
        w_next = _as_f32_rows(w_next, "w_next")
        if w_next.shape[0] != width:
            raise ValueError(f"gcn_fwd: w_next has {w_next.shape[0]} rows for {width} columns")
        f_next = w_next.shape[1]
        z_next = torch.empty(n, f_next, dtype=_F32, device=dev) if out_next is None else out_next
    if n == 0 or width == 0:
        return y, (z_next.zero_() if z_next is not None else None)
    if row_scale is not None:
        row_scale = _as_f32c(row_scale, "row_scale")
    post_op = bool(relu) or drop is not None or f_next > 0
    if not fused or (post_op and width <= NEXT_MAX):
        spmm(graph, z, out=y, row_scale=row_scale)
        if relu or drop is not None:
            launch("acm_bias_act", f"bias_act/{n}x{width}", dev, n, width, _vp(y), y.stride(0), None, int(relu), _ref(drop))
        if f_next:
            gemm(y, w_next, out=z_next)
        return y, z_next
    ride = 0 < f_next <= NEXT_MAX and width <= 256
    p = _lib.GcnFwd()
    p.width, p.relu = width, int(relu)
    p.z, p.ld_z, p.y, p.ld_y = z.data_ptr(), z.stride(0), y.data_ptr(), y.stride(0)
    p.row_scale = row_scale.data_ptr() if row_scale is not None else None
    if drop is not None:
        p.drop = drop
    if ride:
        p.f_next, p.w_next, p.ld_w_next = f_next, w_next.data_ptr(), w_next.stride(0)
        p.z_next, p.ld_z_next = z_next.data_ptr(), z_next.stride(0)
    ws = graph.workspace(min(width, 256))
    launch("acm_gcn_fwd", f"gcn_fwd/W{width}" + (f"+{f_next}" if ride else ""), dev, graph.handle, C.byref(p), _vp(ws), ws.numel() * 4)
    if f_next and not ride:
        gemm(y, w_next, out=z_next)
    return y, z_next


def gcn_bwd(graph_t, dy, h, w2, keep_scale=1.0, relu=True, fused=True, defer=None, want_dz=False):
    """(g, d_w2, dz): dz = A^T dy for the CsrGraph ``graph_t`` of A^T and a narrow dy, g = (dz @ w2.T) * keep_scale [h > 0] --
    the masks read off the stored forward output ``h`` -- and d_w2 = h.T @ dz, as ONE gather launch (acm_gcn_bwd; dy of at
    most 8 columns).  ``defer``: a DeferredReductions the sum of d_w2 is appended to.  ``dz`` is None unless ``want_dz``.
    ``fused=False`` (any width of dy, h of at most 256 columns): acm_spmm + acm_gemm + acm_bias_act_bwd + acm_gemm."""
    dy, h, w2 = _as_f32_rows(dy, "dy"), _as_f32_rows(h, "h"), _as_f32_rows(w2, "w2")
    n, hidden, dev = graph_t.n_rows, h.shape[1], dy.device
    width = dy.shape[1]
    if dy.shape[0] != graph_t.n_cols or h.shape[0] != n or tuple(w2.shape) != (hidden, width):
        raise ValueError("gcn_bwd: shape mismatch")
    if hidden > MASK_MAX:
        raise NotImplementedError(f"gcn_bwd: at most {MASK_MAX} hidden columns (got {hidden})")
    if not fused or width > NEXT_MAX:
        dz = spmm(graph_t, dy)
        g = mask_bwd(h, gemm(dz, w2, trans_b=True), keep_scale, relu)
        return g, gemm(h, dz, trans_a=True), (dz if want_dz else None)
    g = torch.empty(n, hidden, dtype=_F32, device=dev)
    flat = torch.empty(hidden * width, dtype=_F32, device=dev)
    d_w2 = flat.view(hidden, width)
    dz = torch.empty(n, width, dtype=_F32, device=dev) if want_dz else None
    ws, nbytes = _workspace_sized(dev, "acm_gcn_bwd_workspace_bytes", graph_t.handle, width, hidden)
    p = _lib.GcnBwd()
    p.width, p.hidden, p.keep_scale, p.relu = width, hidden, float(keep_scale), int(relu)
    p.dy, p.ld_dy, p.h, p.ld_h, p.w2, p.ld_w2 = dy.data_ptr(), dy.stride(0), h.data_ptr(), h.stride(0), w2.data_ptr(), w2.stride(0)
    p.g, p.ld_g, p.d_w2, p.ld_dw2 = g.data_ptr(), g.stride(0), d_w2.data_ptr(), width
    if dz is not None:
        p.dz, p.ld_dz = dz.data_ptr(), dz.stride(0)
    p.defer = defer.pointer() if defer is not None else None
    launch("acm_gcn_bwd", f"gcn_bwd/W{width}H{hidden}", dev, graph_t.handle, C.byref(p), _vp(ws), nbytes)
    if defer is not None:
        defer.hold(ws, [d_w2], keep=[flat])
    return g, d_w2, dz


def mask_bwd(y, dy, keep_scale, relu):
    """dy * keep_scale * [y > 0] (without a ReLU: [y != 0]) -- the backward of dropout(relu?(.)) read off its stored output
    (acm_bias_act_bwd; the bias sum it also forms is dropped)."""
    if not relu and keep_scale == 1.0:
        return dy
    y, dy = _as_f32_rows(y, "y"), _as_f32_rows(dy, "dy")
    n, f = y.shape
    if f > MASK_MAX:
        raise NotImplementedError(f"mask_bwd: at most {MASK_MAX} columns (got {f})")
    g = torch.empty(n, f, dtype=_F32, device=y.device)
    d_b = torch.empty(f, dtype=_F32, device=y.device)
    ws, nbytes = _workspace_sized(y.device, "acm_bias_act_bwd_workspace_bytes", n, f)
    launch("acm_bias_act_bwd", f"bias_act_bwd/{n}x{f}", y.device, n, f, _vp(y), y.stride(0), _vp(dy), dy.stride(0), float(keep_scale), int(relu),
           _vp(g), g.stride(0), _vp(d_b), _vp(ws), nbytes, None)
    return g


def low_t_product(ops, g, fused=True):
    """A_low^T g for a FilterOperators: the transposed handle, or -- implicit form, symmetric pattern -- the pattern itself
    over the source-scaled operand, A_low^T g = P (diag(row_scale) g)."""
    graph, src = _transposed(ops, g)
    return gcn_fwd(graph, src, fused=fused)[0]


def _transposed(ops, g):
    # (low_t: the pattern itself for the symmetric implicit form, the transposed handle otherwise, or the caller's override)
    return ops.low_t, (torch.mul(g, ops.row_scale[:, None]) if ops.implicit else g)


def _keep_scale(drop):
    return 1.0 / (1.0 - drop[0]) if (drop is not None and drop[0] > 0) else 1.0


def _spec(drop):
    return _drop_spec(drop[:3], drop[3]) if drop is not None else None


def _project(x, w):
    """x @ w for dense or CSR features."""
    if isinstance(x, SparseFeatures):
        return spmm_v(x.csr, x.values, w)
    return gemm(x, w)


def _project_bwd(x, w, dz, need_dx):
    """(dx, dw) of z = x @ w."""
    if isinstance(x, SparseFeatures):
        xt = x.csr_t
        return None, spmm_v(xt, x.values.index_select(0, xt.src_pos), dz)
    return (gemm(dz, w, trans_b=True) if need_dx else None), gemm(x, dz, trans_a=True)


# ---- autograd Functions ----
class _SparseMm(torch.autograd.Function):
    """z = X_csr @ w (acm_spmm_v); dw = X_csr^T dz on the transposed feature handle."""

    @staticmethod
    def forward(ctx, xs, w):
        ctx.xs = xs
        w = _as_f32c(w, "weight")
        ctx.save_for_backward(w)
        return spmm_v(xs.csr, xs.values, w)

    @staticmethod
    def backward(ctx, dz):
        (w,) = ctx.saved_tensors
        return None, _project_bwd(ctx.xs, w, _as_f32c(dz, "grad"), False)[1]


class _Aggregate(torch.autograd.Function):
    """out = A_low^hops z as a chain of one-hop gathers; backward: the transposed chain."""

    @staticmethod
    def forward(ctx, z, ops, hops, fused):
        ctx.ops, ctx.hops, ctx.fused = ops, int(hops), bool(fused)
        y = z
        for _ in range(ctx.hops):
            y = gcn_fwd(ops.low, y, row_scale=ops.row_scale, fused=fused)[0]
        return y

    @staticmethod
    def backward(ctx, dy):
        g = _as_f32_rows(dy, "grad")
        for _ in range(ctx.hops):
            g = low_t_product(ctx.ops, g, ctx.fused)
        return g, None, None, None


class _DenseAct(torch.autograd.Function):
    """y = dropout(relu?(x @ w)) for dense x (acm_gemm_act: one launch) or CSR x (acm_spmm_v + acm_bias_act).  Backward:
    the masks off y (acm_bias_act_bwd), dw = x^T g, dx = g w^T."""

    @staticmethod
    def forward(ctx, x, w, relu, drop):
        w = _as_f32c(w, "weight")
        spec = _spec(drop)
        sparse = isinstance(x, SparseFeatures)
        if sparse:
            y = spmm_v(x.csr, x.values, w)
            if relu or spec is not None:
                launch("acm_bias_act", f"bias_act/{y.shape[0]}x{y.shape[1]}", y.device, y.shape[0], y.shape[1], _vp(y), y.stride(0), None,
                       int(relu), _ref(spec))
        else:
            x = _as_f32_rows(x, "input")
            y = gemm_act(x, w, relu, spec)
        ctx.relu, ctx.ks, ctx.xs = bool(relu), _keep_scale(drop), (x if sparse else None)
        ctx.save_for_backward(w if sparse else x, w, y)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w, y = ctx.saved_tensors
        g = mask_bwd(y, _as_f32_rows(dy, "grad"), ctx.ks, ctx.relu)
        dx, dw = _project_bwd(ctx.xs if ctx.xs is not None else x, w, g, ctx.needs_input_grad[0])
        return dx, dw, None, None


class _Gcn(torch.autograd.Function):
    """The two-layer GCN  out = A (dropout(relu(A (x w1))) w2)  (baseline_models/models.py:29-33) in its two execution forms.

    ``cached``: ``operand`` is P = A x, constant over the run: h = dropout(relu(P w1)) is a dense product (acm_gemm_act) and its
    backward has no gather, dw1 = P^T g.  Otherwise ``operand`` is x (dense or CSR): project first, z1 = x w1, then ONE gather
    launch forms h and z2 = h w2 (acm_gcn_fwd).  Either way the output layer is a plain acm_gcn_fwd and the backward starts
    with acm_gcn_bwd: dz2 = A^T dout, g = dL/d(pre-activation of h) and dw2 = h^T dz2 from one gather launch.  ``fused=True`` on
    an operator of more than FUSE_MAX_ITEMS work items takes the composed arm for the whole step (it measured faster there);
    ``fused="always"`` forces the fused arm."""

    @staticmethod
    def forward(ctx, operand, w1, w2, ops, cached, drop, fused, call):
        ctx.defer = call.defer if call is not None else None
        fused = resolve_fused(fused, ops.low)             # one arm for the whole step
        ctx.ops, ctx.cached, ctx.fused, ctx.ks = ops, bool(cached), fused, _keep_scale(drop)
        w1, w2 = _as_f32c(w1, "weight"), _as_f32c(w2, "weight")
        spec = _spec(drop)
        sparse = isinstance(operand, SparseFeatures)
        if cached:
            operand = _as_f32_rows(operand, "P")
            h = gemm_act(operand, w1, True, spec)
            z2 = gemm(h, w2)
        else:
            if not sparse:
                operand = _as_f32_rows(operand, "input")
            h, z2 = gcn_fwd(ops.low, _project(operand, w1), row_scale=ops.row_scale, relu=True, drop=spec, w_next=w2, fused=fused)
        out = gcn_fwd(ops.low, z2, row_scale=ops.row_scale, fused=fused)[0]
        ctx.xs = operand if sparse else None
        ctx.save_for_backward(w1 if sparse else operand, w1, w2, h)
        return out

    @staticmethod
    def backward(ctx, dout):
        x, w1, w2, h = ctx.saved_tensors
        ops, fused = ctx.ops, ctx.fused
        graph_t, dys = _transposed(ops, _as_f32_rows(dout, "grad"))
        g, d_w2, _ = gcn_bwd(graph_t, dys, h, w2, ctx.ks, True, fused=fused, defer=ctx.defer)
        if ctx.cached:
            dx, d_w1 = None, gemm(x, g, trans_a=True)
        else:
            dx, d_w1 = _project_bwd(ctx.xs if ctx.xs is not None else x, w1, low_t_product(ops, g, fused), ctx.needs_input_grad[0])
        return dx, d_w1, d_w2, None, None, None, None, None


def sparse_mm(xs, w):
    """SparseFeatures @ w, differentiable in w."""
    return _run(_SparseMm, xs, w)


def aggregate(z, ops, hops=1, fused=True):
    """A_low^hops z for a FilterOperators (either form), differentiable in z."""
    return _run(_Aggregate, z, ops, int(hops), resolve_fused(fused, ops.low))


def dense_act(x, w, relu=False, drop=None):
    """dropout(relu?(x @ w)); ``drop = (p, tag, DropoutState, row_offset)`` or None; x dense or SparseFeatures."""
    if drop is not None and not drop[0] > 0:
        drop = None
    return _run(_DenseAct, x, w, bool(relu), drop)


def gcn_two_layer(operand, w1, w2, ops, cached=False, drop=None, fused=True, call=None):
    """A_low (dropout(relu(A_low (x w1))) w2) -- see _Gcn.  ``operand``: P = A_low x with ``cached``, else x."""
    if drop is not None and not drop[0] > 0:
        drop = None
    return _run(_Gcn, operand, w1, w2, ops, bool(cached), drop, fused, _call_or_ambient(call))
