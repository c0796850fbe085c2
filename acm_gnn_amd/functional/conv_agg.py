"""The two aggregate-first routes of the ACM layer, A (X W) = (A X) W for an input that takes no gradient: _AcmAggFirst for
F_in <= 16 (the f_pad <= 16 kernels, with the input pipeline's carried gather) and _AcmAggWide for 16 < F_in <= 128."""
import ctypes as C

import torch

from .. import _lib, tuning
from .. import functional as _pkg
from ._context import _call_or_ambient
from ._hidden import HiddenToken, PreProj, hidden_elision_why_not
from ._conv_shared import _NO_GRADS, _conv_prologue, _flat_views, _gathered_input, _grads, _head_params, _k3_setup, \
    _narrow_tables, _pack_head, _reduce_replicated, _set_head, _set_post, _struc_grad, _struc_rows, _unpack_head
from ._launch import EUNSUPPORTED, _F32, _as_f32c, _vp, _workspace, launch
from .ops import _drop_spec, cast_bf16, gemm, proj_bwd, spmm


def _out_optional_query(p, n):
    """proj_f -> the library's answer to acm_conv_agg_out_optional for the argument block ``p``; None without the symbol."""
    fn = getattr(_lib.load(), _lib.OUT_OPTIONAL_SYMBOL, None)
    if fn is None:
        return None
    return lambda proj_f: int(fn(C.byref(p), n, int(proj_f))) == 1


class _WriteOut:
    """What writes a hidden activation its forward left unwritten, should a consumer turn out to need its bytes
    (_hidden.HiddenToken): one more launch of the row-local stage over the rows the forward worked on -- ``xs`` / ``agg``, the
    copies it left for the backward -- with only ``out`` requested.  The post-op's counter does not move between a step's
    forward and its backward, so the mask and every bit are the forward's."""

    def __init__(self, p, graph, shape, label, dev, xs, agg, keep):
        q = self.q = _lib.ConvAggFwd()
        C.memmove(C.byref(q), C.byref(p), C.sizeof(q))
        q.xs, q.ld_xs = xs.data_ptr(), xs.stride(0)
        q.agg, q.ld_agg, q.agg_given = agg.data_ptr(), agg.stride(0), 1
        q.agg_copy = q.xs_copy = q.next_x = q.head_stats = None
        q.next_f, q.next_w_low, q.next_w_high, q.next_w_mlp, q.next_zlh, q.next_zi = 0, None, None, None, None, None
        self.graph, self.shape, self.label, self.dev, self.keep = graph, shape, label, dev, (xs, agg) + tuple(keep)

    def fresh(self):
        return torch.empty(*self.shape, dtype=_F32, device=self.dev)

    def __call__(self, out):
        q = self.q
        att = torch.empty(self.shape[0], 4, dtype=_F32, device=self.dev)
        q.out, q.ld_out, q.att = out.data_ptr(), out.stride(0), att.data_ptr()
        launch("acm_conv_agg_fwd", self.label, self.dev, self.graph.handle, C.byref(q), None, 0)    # (P is given: no workspace)


class _AcmAggFirst(torch.autograd.Function):
    """out, att = ACM layer in the aggregate-first form for F_in <= 16 (_agg_first_shape): the input takes no gradient.

    forward : acm_conv_agg_fwd (P = A_low X, the three projections of P / X and the head in one kernel; the row-local stage only
              when P is given) [-> the next layer's narrow projection in its epilogue]
    backward: acm_conv_agg_bwd (one row-local kernel, no SpMM for the three filterbank channels) [-> spmm_sub for d struc_low]

    Argument list (shared by the four layer Functions): x, the three weights, att_vec_low / high / mlp, att_struc_low,
    struc_low, att_vec (the k x k mix), the four LayerNorm weights and biases, ops, cfg, post_relu, post_scale, post_drop, call,
    tail_layer, agg_holder, in_drop, pregathered -- see acm_conv."""

    @staticmethod
    def forward(ctx, x, w_low, w_high, w_mlp, v_low, v_high, v_mlp, v_struc, struc_low, att_mix, lnw_low, lnw_high, lnw_mlp,
                lnw_struc, lnb_low, lnb_high, lnb_mlp, lnb_struc, ops, cfg, post_relu, post_scale, post_drop, call, tail_layer,
                agg_holder, in_drop, pregathered):
        x = _conv_prologue(ctx, x, w_low, ops, post_relu, post_scale, post_drop, call, in_drop)
        call = ctx.call
        link = ctx.link = call.link if (call.link is not None and not call.link.sealed) else None     # the HiddenLink it produces for
        dev, n = x.device, x.shape[0]
        f_in, f = w_low.shape
        k = cfg.n_channels
        four = k == 4
        fp = 4 if f_in <= 4 else (8 if f_in <= 8 else 16)
        x, xpad, xg, agg_given, agg_holder = _gathered_input(ctx, x, ops, f_in, f, fp, agg_holder, pregathered, True)
        wl, wh, wm = (_as_f32c(t, "weight") for t in (w_low, w_high, w_mlp))
        if four:
            s_local, s_gath = _struc_rows(ops, struc_low, n)
        vecs, lnw, lnb, mix = _head_params(cfg, (v_low, v_high, v_mlp, v_struc), att_mix, (lnw_low, lnw_high, lnw_mlp, lnw_struc),
                                           (lnb_low, lnb_high, lnb_mlp, lnb_struc))
        out = torch.empty(n, f, dtype=_F32, device=dev)
        att = torch.empty(n, 4, dtype=_F32, device=dev)
        p = _lib.ConvAggFwd()
        p.f_in, p.f_pad, p.f_out = f_in, fp, f
        _set_head(p, cfg, vecs, lnw, lnb, mix)
        p.xg, p.ld_xg = xg.data_ptr(), xg.stride(0)
        p.xs, p.ld_xs = xpad.data_ptr(), xpad.stride(0)
        p.w_low, p.w_high, p.w_mlp, p.ld_w = wl.data_ptr(), wh.data_ptr(), wm.data_ptr(), f
        agg = agg_given if agg_given is not None else torch.empty(n, fp, dtype=_F32, device=dev)
        p.agg_given = int(agg_given is not None)
        refill = False
        if ctx.pipe is not None:                  # the backward's operands: copies the row-local kernel leaves
            p.agg_copy, p.ld_agg_copy = ctx.pipe.saved[1].data_ptr(), ctx.pipe.saved[1].stride(0)
            p.xs_copy, p.ld_xs_copy = ctx.pipe.saved[0].data_ptr(), ctx.pipe.saved[0].stride(0)
            # ... and (one device: the table IS this rank's rows) it refills the table with dropout_{t+1}(x) over the rows
            # it has just copied: make_next()'s acm_dropout launch is gone
            refill = ctx.pipe.refill_spec(p)
        p.out, p.ld_out = out.data_ptr(), out.stride(0)
        p.agg, p.ld_agg = agg.data_ptr(), agg.stride(0)
        p.att = att.data_ptr()
        if ops.implicit:
            p.row_scale = ops.row_scale.data_ptr()
        extra = ()
        if four:                                  # pre_S = deg * (A_low S) - S: one F-wide gather of S
            ps = torch.empty(n, f, dtype=_F32, device=dev)
            if cfg.gather_bf16 and f % 2 == 0 and f > 8:
                sgt = cast_bf16(s_gath)
                p.sg_bf16 = 1
            else:
                sgt = s_gath
            p.sg, p.ld_sg = sgt.data_ptr(), sgt.stride(0)
            p.ss, p.ld_ss = s_local.data_ptr(), s_local.stride(0)
            p.deg = ops.deg.data_ptr()
            p.ps, p.ld_ps = ps.data_ptr(), ps.stride(0)
            extra = (ps, s_local)
        _set_post(p, ctx.post_relu, ctx.post_scale, ctx.post_drop, ops.row_offset)
        # the row's head statistics (mean | rstd | sigmoid | alpha per channel): 16 k bytes per row that save
        # the backward three 16-lane reductions per channel and row
        stats = torch.empty(n, 4 * k, dtype=_F32, device=dev) if any(ctx.needs_input_grad) else None
        if stats is not None:
            p.head_stats, p.ld_head_stats = stats.data_ptr(), stats.stride(0)
        ctx.head_stats = stats
        # (the row-local stage is a kernel of its own when P is given, and always with the structure channel)
        nxt = link.take_request(f, dev, f == 64 and (agg_given is not None or four)) if link is not None else None
        pre = None
        if nxt is not None:
            f2 = nxt.f2
            n_zlh, _ = _narrow_tables(n, f2, f2, dev, nxt.pack4)
            n_zi = torch.empty(n, f2, dtype=_F32, device=dev)
            p.next_w_low, p.next_w_high, p.next_w_mlp = ptrs = tuple(w.data_ptr() for w in nxt.w3)
            p.next_ld_w, p.next_f, p.next_relu = nxt.w3[0].stride(0), f2, int(nxt.relu)
            p.next_zlh, p.ld_next_zlh = n_zlh.data_ptr(), n_zlh.stride(0)
            p.next_zi, p.ld_next_zi = n_zi.data_ptr(), n_zi.stride(0)
            pre = PreProj(n_zlh, n_zi, ptrs, nxt.relu)
        # the output stays unwritten where only the following layer consumes it and does so through next_zlh / next_zi
        # (forward) and this layer's own backward kernel (acm_conv_agg_bwd_t.proj_*): decided here, before the launch
        # (a backward may follow: the caller's grad mode as acm_conv saw it -- in here gradients are always switched off)
        will_backward = any(ctx.needs_input_grad) and call.grad_enabled
        why = hidden_elision_why_not(call, nxt, agg_given is not None, ops.sharded, will_backward,
                                     int(getattr(ops, "hops", 1)), ctx.post_relu, ctx.post_scale, stats is not None, f,
                                     _out_optional_query(p, n))
        call.elision = (why is None, why)
        if why is None:
            p.out = None
        ws = ops.low.workspace(max(fp, f) if four else fp)
        launch("acm_conv_agg_fwd", f"conv_agg_{'epi' if agg_given is not None else 'fwd'}/F{f}k{k}i{f_in}", dev, ops.low.handle, C.byref(p),
               _vp(ws), ws.numel() * 4)
        if refill:
            ctx.pipe.next_table_ready = True
        if agg_holder is not None and agg_given is None:
            agg_holder["agg"] = agg
        ctx.ops, ctx.cfg, ctx.f_in = ops, cfg, f_in
        # with a fused ReLU the output itself records which elements the post-op let through: the backward reads it
        # instead of regenerating the dropout mask (no extra memory: the next layer keeps the same tensor alive)
        # (an unwritten output is an identity token only: not saved, never read -- the link's HiddenToken writes it for a
        #  consumer that needs its bytes after all)
        ctx.out_mask = bool(ctx.post_relu) and ctx.post_scale is None and why is not None
        if ctx.pipe is not None:
            xpad, agg = ctx.pipe.saved[0], ctx.pipe.saved[1]
        if link is not None:
            token = None
            if why is None:
                token = HiddenToken(out, _WriteOut(p, ops.low, (n, f), f"conv_agg_out/F{f}k{k}i{f_in}", dev, xpad, agg,
                                                   (wl, wh, wm, mix, *vecs, *lnw, *lnb, ctx.post_drop)))
            link.produced(out, will_backward, pre, token)
        ctx.save_for_backward(xpad, agg, wl, wh, wm, *_pack_head(vecs, lnw, lnb, mix), *extra, *((out,) if ctx.out_mask else ()))
        ctx.mark_non_differentiable(att)
        return out, att

    @staticmethod
    def backward(ctx, grad_out, _grad_att):
        """One row-local kernel and no SpMM for the three filterbank channels; the structure channel (k = 4) adds one F-wide
        transposed product for d struc_low.  Collectives: the all-reduce of the replicated-parameter gradients, plus the
        all-gather of D*G_S when sharded with k = 4."""
        if grad_out is None:
            return _NO_GRADS
        ops, cfg, f_in = ctx.ops, ctx.cfg, ctx.f_in
        k = cfg.n_channels
        four = k == 4
        saved = ctx.saved_tensors
        out_fwd = None
        if ctx.out_mask:
            out_fwd, saved = saved[-1], saved[:-1]
        xpad, agg, wl, wh, wm = saved[:5]
        vecs, lnw, lnb, mix = _unpack_head(saved, cfg, 5)
        dev = xpad.device
        n, f, fp = xpad.shape[0], wl.shape[1], xpad.shape[1]
        link = ctx.link
        lazy = link.take_lazy() if link is not None else None
        if lazy is not None and (grad_out is not lazy.placeholder and grad_out.data_ptr() != lazy.placeholder.data_ptr()):
            raise RuntimeError("acm_conv: the hidden activation marked private (HiddenLink.grad_private) received a gradient "
                               "from somewhere else as well")
        elide = link.token if link is not None else None        # the HiddenToken of an `out` the forward left unwritten
        elided = elide is not None and not elide.written        # ... and nobody has written since
        defer = ctx.call.defer
        token_x = lazy.x if lazy is not None else None          # (the token itself, where the following layer handed it back)
        if elide is not None and not elided:              # a consumer asked for its bytes in the meantime: read like a stored one
            out_fwd = elide.write(token_x)
        fuse_proj = (lazy is not None and fp == 8 and f == 64 and (out_fwd is not None or elided) and ctx.post_scale is None
                     and ctx.head_stats is not None and bool(ctx.post_relu))
        if elided and not fuse_proj:                      # no kernel here forms the row again: written now, the mask is read
            out_fwd, elided = elide.write(token_x), False
        if lazy is not None and not fuse_proj:            # the kernel cannot take it: materialise dX and dW' now
            proj_bwd(lazy.x, lazy.dz, lazy.w3, lazy.d_w, defer=defer, dx_out=lazy.placeholder)
            lazy = None
        grad_out = _as_f32c(grad_out, "grad_out")
        # [dW_L | dW_H | dW_I | d att_vec | d LayerNorm weights | biases | d att_mix] (the LayerNorm parts whether used or not)
        nw = 3 * f_in * f
        d_params = torch.empty(nw + 3 * k * f + k * k, dtype=_F32, device=dev)
        q = _lib.ConvAggBwd()
        q.f_in, q.f_pad, q.f_out = f_in, fp, f
        _set_head(q, cfg, vecs, lnw, lnb, mix)
        q.grad_out, q.ld_grad_out = grad_out.data_ptr(), grad_out.stride(0)
        if lazy is not None:                              # the following layer's projection backward rides this launch
            dz2, w32 = lazy.dz, lazy.w3
            q.grad_out = None
            q.proj_dz, q.ld_proj_dz = dz2.data_ptr(), dz2.stride(0)
            q.proj_w_low, q.proj_w_high, q.proj_w_mlp = (w.data_ptr() for w in w32)
            q.proj_ld_w, q.proj_f = w32[0].stride(0), w32[0].shape[1]
            q.proj_d_w = lazy.d_w.data_ptr()
        q.agg, q.ld_agg = agg.data_ptr(), agg.stride(0)
        if ctx.head_stats is not None:
            q.head_stats, q.ld_head_stats = ctx.head_stats.data_ptr(), ctx.head_stats.stride(0)
        q.xs, q.ld_xs = xpad.data_ptr(), xpad.stride(0)
        q.w_low, q.w_high, q.w_mlp, q.ld_w = wl.data_ptr(), wh.data_ptr(), wm.data_ptr(), f
        q.d_params = d_params.data_ptr()
        _set_post(q, ctx.post_relu, ctx.post_scale, ctx.post_drop, ops.row_offset)
        if out_fwd is not None:
            q.out, q.ld_out = out_fwd.data_ptr(), out_fwd.stride(0)
        if four:
            ps, s_local = saved[-2], saved[-1]
            gs = torch.empty(n, f, dtype=_F32, device=dev)            # D * dL/dpre_S
            q.ps, q.ld_ps = ps.data_ptr(), ps.stride(0)
            q.ss, q.ld_ss = s_local.data_ptr(), s_local.stride(0)
            q.deg = ops.deg.data_ptr()
            q.g_struc, q.ld_g_struc = gs.data_ptr(), gs.stride(0)
            q.g_struc_scale = None if ops.implicit else ops.deg.data_ptr()
        ws = _workspace(dev, "acm_conv_agg_bwd_workspace_bytes", n, f_in, f)
        q.defer = defer.pointer() if defer is not None else None
        pipe = ctx.pipe
        carry = pipe is not None and pipe.next_table_ready and not pipe.next_agg_ready
        if carry:                                     # the next step's P = A_low dropout(x) rides this launch
            q.next_a = ops.low.handle
            q.next_xg, q.ld_next_xg = pipe.table().data_ptr(), pipe.table().stride(0)
            q.next_row_scale = ops.row_scale.data_ptr()
            q.next_agg, q.ld_next_agg = pipe.agg().data_ptr(), pipe.agg().stride(0)
        st = launch("acm_conv_agg_bwd", f"conv_agg_bwd{'+gather' if carry else ''}{'+proj' if lazy is not None else ''}/F{f}k{k}i{f_in}", dev, n,
                    C.byref(q), _vp(ws), ws.numel() * 4, unsupported_ok=lazy is not None or carry)
        if st == EUNSUPPORTED:                            # not with these riders after all: the plain launch(es)
            if elided:                                    # (acm_conv_agg_out_optional said otherwise: the row is written first)
                out_fwd, elided = elide.write(token_x), False
                q.out, q.ld_out = out_fwd.data_ptr(), out_fwd.stride(0)
            if lazy is not None:
                proj_bwd(lazy.x, lazy.dz, lazy.w3, lazy.d_w, defer=defer, dx_out=lazy.placeholder)
                q.grad_out, q.proj_dz, lazy = grad_out.data_ptr(), None, None
            if carry:                                     # the gather as its own launch, right here: the pipeline stays valid
                q.next_a, q.next_xg, q.next_row_scale, q.next_agg = None, None, None, None          # (also inside a capture, where
                spmm(ops.low, pipe.table(), out=pipe.agg(), row_scale=ops.row_scale)                 # nobody could prime() it again)
            launch("acm_conv_agg_bwd", f"conv_agg_bwd/F{f}k{k}i{f_in}", dev, n, C.byref(q), _vp(ws), ws.numel() * 4)
        if carry:
            pipe.next_agg_ready = True
        if defer is not None:
            defer.hold(ws, [d_params] + ([lazy.d_w] if lazy is not None else []),
                       keep=[d_params] + ([lazy.d_w._base if lazy.d_w._base is not None else lazy.d_w] if lazy is not None else []))
        d_struc = _struc_grad(ops, cfg, gs) if four else None
        _reduce_replicated(d_params, ops, defer)
        d_w = d_params[:nw].view(3, f_in, f)
        d_vec, d_lnw, d_lnb, d_mix = _flat_views(d_params, nw, k, f, True)
        if not cfg.layernorm:
            d_lnw = d_lnb = []
        return _grads(None, (d_w[0], d_w[1], d_w[2]), d_vec, d_struc, d_mix, d_lnw, d_lnb)


# ---- aggregate-first for WIDE dense inputs (16 < F_in <= 128) ----
AGG_WIDE_MIN_DEGREE = 12          # stored entries of A_low per row from which the wide aggregate-first form is taken


def agg_wide_supported(x, ops, cfg, f_in, f_out, post_scale=None, call=None, tail_layer=False):
    """The first layer of the arXiv-year / pokec class (ACM-Geometric/layers.py:101-104 with 128 / 65 input features, 64
    hidden): without a ReLU between projection and filter, A (X W) = (A X) W.  P = A_low drop(X) is ONE gather of F_in floats
    per edge (the literal form gathers 2 F = 128), and because the input takes no gradient the backward needs NO transposed
    gather at all:  dW_L = P^T G_L,  dW_H = X^T G_H - P^T G_H,  dW_I = X^T G_I  -- three tall-skinny products on the split-bf16
    matrix pipe.  Three-channel ACM layers; row-sharded: the ONE halo exchange of the layer is the all-gather of the dropped
    F_in-wide input rows (the literal form all-gathers 2 F-wide rows forward AND backward); tuning rewrites bit 1 switches it off."""
    from ..graph import FilterOperators
    if not (tuning.HOST.rewrites & tuning.REWRITE_AGG_FIRST) or not isinstance(ops, FilterOperators):
        return False
    if not isinstance(x, torch.Tensor) or x.layout != torch.strided or x.dim() != 2 or x.dtype != _F32 or x.requires_grad:
        return False
    # (gather_dtype="bf16" takes this form too: its ONE gather reads the fp32 input, F_in x 4 bytes per edge -- no more than the
    #  2 F x 2 bytes of the literal form's bf16 tables, and exact)
    if cfg.relu_before or cfg.n_channels != 3 or f_out != 64 or not 16 < f_in <= 128 or x.shape[1] != f_in:
        return False
    if getattr(ops, "general", False) or int(getattr(ops, "hops", 1)) != 1 or x.shape[0] != ops.n_local:
        return False
    if tail_layer:
        return False
    if ops.sharded:
        # every rank must take the same form (its collectives differ from the literal form's): decided by what all ranks know,
        # the longest row block of the plan -- and row-sharded the rewrite pays at any degree (one F_in-wide halo exchange
        # instead of two 2 F-wide ones)
        import torch.distributed as dist
        return ops.n_gathered // dist.get_world_size(ops.group) >= 8192
    if x.shape[0] < 8192:
        return False
    # Where it pays (measured, profiles/r05_agg_wide.txt): the rewrite trades 4 F - F_in gathered floats per EDGE for one more
    # pass over ~3 KB per ROW (the dropped copy of X, the head as its own launch, a third more projection flops).  pokec-shaped
    # (mean degree 38, F_in 65): 12.1 -> 7.0 ms per step; arXiv-year-shaped (mean degree 15, F_in 128): 0.822 -> 0.792.
    return ops.low.nnz >= AGG_WIDE_MIN_DEGREE * x.shape[0]


class _AcmAggWide(torch.autograd.Function):
    """out, att = three-channel ACM layer in the aggregate-first form for a wide dense input (see agg_wide_supported).

    forward : [acm_dropout] -> acm_spmm_ex (P = A_low Xd) -> acm_conv_aggw_fwd (projections on the split-bf16 matrix pipe + head,
              one row-local kernel: pre_L = P W_L, pre_H = (Xd - P) W_H); with tuning rewrites bit 8 off: 2 x acm_gemm
              ([P W_L | P W_H], [Xd W_H | Xd W_I]) -> acm_conv_head_fwd
    backward: acm_conv_aggw_bwd (K3 + the three weight gradients, one kernel); with tuning rewrites bit 8 off (or a post_scale mask
              tensor): acm_conv_bwd_local (K3) -> 2 x acm_gemm TN ([P^T G_L | P^T G_H], [Xd^T G_H | Xd^T G_I])"""

    @staticmethod
    def forward(ctx, x, w_low, w_high, w_mlp, v_low, v_high, v_mlp, v_struc, struc_low, att_mix, lnw_low, lnw_high, lnw_mlp,
                lnw_struc, lnb_low, lnb_high, lnb_mlp, lnb_struc, ops, cfg, post_relu, post_scale, post_drop, call, tail_layer,
                agg_holder, in_drop, pregathered):
        ctx.set_materialize_grads(False)
        call = ctx.call = _call_or_ambient(call)
        if call.link is not None:                  # consumed unheard: the narrow projection rides the f_pad <= 16 kernels only
            call.link.take_request(0, None)
        x = _as_f32c(x, "input")
        dev = x.device
        n, f_in = x.shape
        f, k = w_low.shape[1], 3
        fp = -(-f_in // 4) * 4                     # rows of 16-byte blocks for the gather and the split-bf16 products
        spec = _drop_spec(in_drop, ops.row_offset) if (in_drop is not None and in_drop[0] > 0) else None
        # ``agg_holder`` (layers.GraphConvolution._eval_agg_holder): P = A_low X and the padded copy of a STATIC input from the
        # previous pass over it -- every evaluation pass after the first and every training step of a model without input
        # dropout then skips the layer's gather (a third of the arXiv-year evaluation forward, two thirds of pokec's)
        if spec is not None or ops.sharded:
            agg_holder = None
        agg = None
        if spec is not None:                       # the caller's input dropout, written straight into the padded rows
            xd = torch.empty(n, fp, dtype=_F32, device=dev)
            launch("acm_dropout", f"dropout/{n}x{f_in}", dev, n, f_in, _vp(x), x.stride(0), _vp(xd), xd.stride(0), fp, C.byref(spec))
        elif fp == f_in:
            xd = x
        else:
            xd = agg_holder.get("xpad") if agg_holder is not None else None
            if xd is None or tuple(xd.shape) != (n, fp):
                xd = torch.nn.functional.pad(x, (0, fp - f_in))
                if agg_holder is not None:
                    agg_holder["xpad"], agg_holder["agg"] = xd, None
        if agg_holder is not None:
            agg = agg_holder.get("agg")
            if agg is not None and tuple(agg.shape) != (n, fp):
                agg = None
        if agg is None:
            # P = A_low Xd  [n, fp]; row-sharded: the operator's columns are the all-gathered rows (the layer's only halo exchange)
            agg = spmm(ops.low, _pkg._gather_rows(ops, xd), row_scale=ops.row_scale if ops.implicit else None)
            if agg_holder is not None:
                agg_holder["agg"] = agg
        w3 = [_as_f32c(w, "weight") for w in (w_low, w_high, w_mlp)]
        vecs, lnw, lnb, mix = _head_params(cfg, (v_low, v_high, v_mlp), att_mix, (lnw_low, lnw_high, lnw_mlp),
                                           (lnb_low, lnb_high, lnb_mlp))
        if post_scale is not None:
            post_scale = _as_f32c(post_scale, "post_scale")
        ctx.post_relu, ctx.post_scale = bool(post_relu), post_scale
        ctx.post_drop = post_drop if (post_drop is not None and post_drop[0] > 0) else None
        out = torch.empty(n, f, dtype=_F32, device=dev)
        att = torch.empty(n, 4, dtype=_F32, device=dev)
        pre = torch.empty(n, 2 * f, dtype=_F32, device=dev)
        p = _lib.ConvFwd()
        p.f_out, p.row_offset = f, ops.row_offset
        _set_head(p, cfg, vecs, lnw, lnb, mix)
        p.out, p.ld_out = out.data_ptr(), out.stride(0)
        p.pre, p.ld_pre = pre.data_ptr(), pre.stride(0)
        p.att = att.data_ptr()
        _set_post(p, ctx.post_relu, post_scale, ctx.post_drop, ops.row_offset)
        same_pitch = w3[0].stride(0) == w3[1].stride(0) == w3[2].stride(0)
        if (tuning.HOST.rewrites & tuning.REWRITE_AGGW_FUSED) and same_pitch:
            # projections + head behind the gather as ONE row-local kernel: pre_L = P W_L, pre_H = (Xd - P) W_H, Z_I = Xd W_I
            zi = torch.empty(n, f, dtype=_F32, device=dev)
            launch("acm_conv_aggw_fwd", f"conv_aggw/F{f}k{k}i{f_in}", dev, n, f_in, fp, _vp(agg), agg.stride(0), _vp(xd), xd.stride(0),
                   _vp(w3[0]), _vp(w3[1]), _vp(w3[2]), w3[0].stride(0), _vp(zi), zi.stride(0), C.byref(p))
        else:
            pad = (0, 0, 0, fp - f_in)
            wa = torch.nn.functional.pad(torch.cat((w3[0], w3[1]), 1), pad) if fp != f_in else torch.cat((w3[0], w3[1]), 1)
            wb = torch.nn.functional.pad(torch.cat((w3[1], w3[2]), 1), pad) if fp != f_in else torch.cat((w3[1], w3[2]), 1)
            za = gemm(agg, wa)                         # [P W_L | P W_H]
            zb = gemm(xd, wb)                          # [Xd W_H | Xd W_I]
            zi = zb[:, f:]
            p.g_low, p.ld_g_low = za.data_ptr(), za.stride(0)                 # "gathered" over I: pre_L = 1 * (P W_L)
            p.g_high, p.ld_g_high = za.data_ptr() + 4 * f, za.stride(0)       #                    pre_H = Xd W_H - 1 * (P W_H)
            p.s_high, p.ld_s_high = zb.data_ptr(), zb.stride(0)
            p.s_mlp, p.ld_s_mlp = zb.data_ptr() + 4 * f, zb.stride(0)
            launch("acm_conv_head_fwd", f"conv_head/F{f}k{k}", dev, n, C.byref(p))     # the fused epilogue as its own row-local kernel
        ctx.ops, ctx.cfg, ctx.f_in, ctx.fp = ops, cfg, f_in, fp
        ctx.save_for_backward(xd, agg, zi, pre, *_pack_head(vecs, lnw, lnb, mix))
        ctx.mark_non_differentiable(att)
        return out, att

    @staticmethod
    def backward(ctx, grad_out, _grad_att):
        if grad_out is None:
            return _NO_GRADS
        ops, cfg, f_in, fp = ctx.ops, ctx.cfg, ctx.f_in, ctx.fp
        saved = ctx.saved_tensors
        xd, agg, zi, pre = saved[:4]
        k = 3
        vecs, lnw, lnb, mix = _unpack_head(saved, cfg, 4)
        n, dev = xd.shape[0], xd.device
        f = pre.shape[1] // 2
        defer = ctx.call.defer
        grad_out = _as_f32c(grad_out, "grad_out")
        st3 = _k3_setup(cfg, ops, k, f, n, dev, f_in, pre, zi, vecs, lnw, lnb, mix, grad_out, ctx.post_relu, ctx.post_scale,
                        ctx.post_drop)
        q, flat, nw = st3["q"], st3["flat"], st3["nw"]
        q.g_scale = None                           # (the filter was applied before the projection: no transposed gather here)
        d_vec, d_lnw, d_lnb, d_mix = _flat_views(flat, nw, k, f, cfg.layernorm)
        q.defer = defer.pointer() if defer is not None else None
        dw = flat[:nw].view(3, f_in, f)            # the weight gradients lead the layer's flat gradient buffer
        if n == 0:                                 # a rank without rows (row-sharded, degenerate plan): zero partial sums, same collectives
            flat.zero_()
            del st3
        elif (tuning.HOST.rewrites & tuning.REWRITE_AGGW_FUSED) and ctx.post_scale is None:
            # K3 and the three weight gradients in ONE kernel: [G_L | G_H | G_I] never reach memory
            q.g_low = q.g_high = q.g_mlp = None
            ws = _workspace(dev, "acm_conv_aggw_bwd_workspace_bytes", n, fp)
            launch("acm_conv_aggw_bwd", f"conv_aggw_bwd/F{f}k{k}i{f_in}", dev, n, f_in, fp, _vp(agg), agg.stride(0), _vp(xd), xd.stride(0),
                   C.byref(q), _vp(dw[0]), _vp(dw[1]), _vp(dw[2]), f, _vp(ws), ws.numel() * 4)
            if defer is not None:
                defer.hold(ws, [d_mix, *d_vec, *d_lnw, *d_lnb, dw], keep=[flat])
            del st3
        else:
            # K3 writes [G_L | G_H | G_I] side by side, UNSCALED; two transposed split-bf16 products read them back
            gcat = torch.empty(n, 3 * f, dtype=_F32, device=dev)
            q.g_low, q.ld_g_low = gcat.data_ptr(), gcat.stride(0)
            q.g_high, q.ld_g_high = gcat.data_ptr() + 4 * f, gcat.stride(0)
            q.g_mlp, q.ld_g_mlp = gcat.data_ptr() + 8 * f, gcat.stride(0)
            ws = _workspace(dev, "acm_conv_bwd_local_workspace_bytes", n, f, k)
            launch("acm_conv_bwd_local", f"conv_bwd_local/F{f}k{k}", dev, n, C.byref(q), _vp(ws), ws.numel() * 4)
            if defer is not None:
                defer.hold(ws, [d_mix, *d_vec, *d_lnw, *d_lnb], keep=[flat])
            del st3
            a1 = gemm(agg, gcat[:, : 2 * f], trans_a=True, col_blocks=2)          # [P^T G_L | P^T G_H]   as [2, fp, f]
            a2 = gemm(xd, gcat[:, f:], trans_a=True, col_blocks=2)                # [Xd^T G_H | Xd^T G_I]
            dw[0].copy_(a1[0][:f_in])
            torch.sub(a2[0][:f_in], a1[1][:f_in], out=dw[1])
            dw[2].copy_(a2[1][:f_in])
        # the weight gradients sit with the head's in the layer's flat buffer: ONE all-reduce when row-sharded
        _reduce_replicated(flat, ops, defer)
        return _grads(None, (dw[0], dw[1], dw[2]), d_vec, None, d_mix, d_lnw, d_lnb)
