"""The two routes of the ACM layer that leave the literal form's saved layout and share its backward: _AcmLiteral (project,
then gather, as the reference does) and _AcmAcmii (the ACMII first layer that recomputes the projection per edge)."""
import ctypes as C

import torch

from .. import _lib, tuning
from .. import functional as _pkg
from ..graph import SparseFeatures
from ._hidden import LazyGrad, ensure_hidden_written, lazy_hidden_why_not
from ._conv_shared import _NO_GRADS, _chan_block, _conv_prologue, _flat_views, _gathered_input, _grads, _head_params, _hop_buffer, \
    _k3_setup, _low_product, _narrow_tables, _pack_head, _reduce_replicated, _set_head, _set_post, _struc_grad, _struc_rows, \
    _unpack_head, _z_pitch, PROJECTED
from ._launch import _F32, EUNSUPPORTED, _as_f32c, _capturing, _vp, _workspace, _workspace_bytes, launch
from .ops import _drop_now, _drop_spec, cast_bf16, gemm, gemm_drop_supported, gemm_split, proj3, proj_bwd, proj_bwd_supported, \
    proj_fwd, spmm, spmm_v


def _literal_project(ctx, x, w3, ops, cfg):
    """K1 of the literal form: Z = X [W_L | W_H | W_I] (ReLU'd for ACMII), with the caller's input dropout drawn in the operand
    load where the projection can (else applied here first), then the k-hop chain's low-pass products.  Returns
    (x as saved for the backward, [Z_L | Z_H], Z_I, the gathered [Z_L | Z_H] or [A_low^(k-1) Z_L | Z_H]); sets ctx.fb.
    A block input (ctx.blocks_z): ``x`` IS Z, projected by functional.blocks.project_blocks in the CSR route's one-table layout."""
    call, hops = ctx.call, ctx.hops
    if ctx.blocks_z:
        f = w3[0].shape[1]
        fb = ctx.fb = _chan_block(f)
        if x.shape[1] != 2 * fb + f:
            raise ValueError(f"the projected block input has {x.shape[1]} columns, the layer's Z has {2 * fb + f}")
        return x, x[:, : 2 * fb], x[:, 2 * fb:], _hop_chain(ops, x[:, : 2 * fb], f, fb, hops)
    sparse_x = isinstance(x, SparseFeatures)
    n, dev = x.shape[0], w3[0].device
    f_in, f = w3[0].shape
    four = cfg.n_channels == 4
    # narrow dense layers (F <= 5) project with the streaming kernel straight from the three weights; everything
    # else packs [W_L | W_H | W_I] for the MFMA GEMM / the CSR-feature product
    use_proj = (not sparse_x and f <= 5 and f_in <= 64     # wider inputs: the MFMA GEMM is the faster stream
                and w3[0].stride(0) == w3[1].stride(0) == w3[2].stride(0))
    fb = ctx.fb = _chan_block(f)                  # column distance of the two gathered channels
    # Row pitch of Z: for narrow layers the gathered block [Z_L | Z_H] (2F floats) must be
    # one aligned vector fetch, so rows are padded to a multiple of that block.
    ldz = _z_pitch(f, fb)
    pre = call.link.take_pre(x, w3, cfg.relu_before) if (use_proj and call.link is not None) else None
    if pre is None and not sparse_x:              # this layer projects x itself: a hidden activation left unwritten is written first
        ensure_hidden_written(call, x)
    drop_spec = _drop_spec(ctx.in_drop, ops.row_offset) if ctx.in_drop is not None else None
    # [Z_L | Z_H] as a compact table of its own (what a narrow gather / the k-hop chain walks: 16-byte-block rows at
    # their own pitch instead of [Z_L | Z_H | Z_I | pad] rows), Z_I next to it
    two_tables = (use_proj or f in (2, 4, 8) or hops > 1) and not sparse_x
    # four channels of two columns: [Z_L | Z_H] and the gathered struc_low rows share 32-byte rows (_narrow_tables)
    pack4 = four and f == 2 and fb == 2 and two_tables and not ops.sharded and not getattr(ops, "general", False)
    done3 = False
    if pre is None and not sparse_x:
        # tall dense inputs of 32..128 features: the three weight matrices in place on the split-bf16 kernel (no cat)
        if two_tables:
            zlh, _ = _narrow_tables(n, fb, f, dev, pack4)
            zi = torch.empty(n, f, dtype=_F32, device=dev)
            done3 = proj3(x, w3, fb, zlh, zi, relu=cfg.relu_before, x_drop=drop_spec)
        else:
            z = torch.empty(n, ldz, dtype=_F32, device=dev)[:, : 2 * fb + f]
            done3 = proj3(x, w3, fb, z, relu=cfg.relu_before, x_drop=drop_spec)
            zlh, zi = z[:, : 2 * fb], z[:, 2 * fb:]
        if done3:
            ctx.in_drop_used = drop_spec is not None
    if (not done3 and drop_spec is not None
            and (pre is not None or use_proj or two_tables or sparse_x or not gemm_drop_supported(n, f_in, 2 * fb + f))):
        # the caller left its input dropout to this layer (in_drop) but the projection about to run cannot draw
        # the mask in its operand load (the two-table / k-hop GEMM, the narrow streaming projection, shapes outside
        # acm_gemm_drop): apply it here, same counter-based mask, and save the DROPPED input for the backward
        if sparse_x:
            raise NotImplementedError("in_drop with CSR features: the caller applies the dropout to the values")
        x, pre = _drop_now(x, drop_spec), None
        drop_spec = None
    if done3:
        pass                                       # [Z_L | Z_H], Z_I are written
    elif pre is not None:
        zlh, zi = pre                              # computed in the preceding layer's epilogue
    elif use_proj:
        zlh, _ = _narrow_tables(n, fb, f, dev, pack4)
        zi = torch.empty(n, f, dtype=_F32, device=dev)
        proj_fwd(x, w3, zlh, zi, relu=cfg.relu_before, h_col=fb)
    else:
        if fb != f:                        # [W_L 0 | W_H 0 | W_I]: the product lands in channel blocks of fb columns
            zpad = w3[0].new_zeros(w3[0].shape[0], fb - f)
            wcat = torch.cat((w3[0], zpad, w3[1], zpad, w3[2]), dim=1).contiguous()
        else:
            wcat = torch.cat(w3, dim=1).contiguous()                            # [F_in, 3F]
        if two_tables:                            # one GEMM with a two-matrix output
            zlh, _ = _narrow_tables(n, fb, f, dev, pack4)
            zi = torch.empty(n, f, dtype=_F32, device=dev)
            gemm_split(x, wcat, zlh, zi, relu=cfg.relu_before)
        else:
            z = torch.empty(n, ldz, dtype=_F32, device=dev)[:, : 2 * fb + f]
            if sparse_x:                              # Z = X_csr Wcat: nnz(X) * 3F FMAs
                spmm_v(x.csr, x.values, wcat, relu=cfg.relu_before, out=z)
            else:
                gemm(x, wcat, relu=cfg.relu_before, out=z, a_drop=drop_spec)        # [n, 3F] view
                ctx.in_drop_used = drop_spec is not None
            zlh, zi = z[:, : 2 * fb], z[:, 2 * fb:]
    return x, zlh, zi, _hop_chain(ops, zlh, f, fb, hops)


def _hop_chain(ops, zlh, f, fb, hops):
    """The table the layer's gather walks: [Z_L | Z_H] itself, or (the k-hop chain) [A_low^(k-1) Z_L | Z_H]; all-gathered
    when row-sharded."""
    n, dev = zlh.shape[0], zlh.device
    if hops > 2:
        # [A_low^(k-1) Z_L | Z_H] in place: the last of the k - 1 >= 2 products reads a hop buffer and writes over
        # Z_L (which nothing reads again: no ReLU mask in the k-hop layer) -- no copy of Z_H into a second table
        t = zlh[:, :f]
        for hop in range(hops - 1):
            t = _low_product(ops, t, out=zlh[:, :f] if hop == hops - 2 else None)
        zg = _pkg._gather_rows(ops, zlh) if ops.sharded else zlh
    elif hops > 1:
        zc = torch.empty(n, 2 * fb, dtype=_F32, device=dev)              # [A_low Z_L | Z_H]
        _low_product(ops, zlh[:, :f], out=zc[:, :f])
        zc[:, fb:fb + f] = zlh[:, fb:fb + f]
        zg = _pkg._gather_rows(ops, zc)
    else:
        zg = _pkg._gather_rows(ops, zlh) if ops.sharded else zlh                 # gathered [Z_L|Z_H]
    return zg


class _AcmLiteral(torch.autograd.Function):
    """out, att = ACM layer in the reference's order, project then gather (arguments as _AcmAggFirst).

    forward : K1 acm_gemm / acm_proj3 / acm_proj_fwd (X [W_L|W_H|W_I]) [-> the k-hop chain] -> K2 acm_conv_fwd
              (or, for an output layer a training loop asked for it, acm_conv_fwd_tail: K2 + loss + K3 in one row pass)
    backward: K3 acm_conv_bwd_local -> K4 acm_conv_bwd_spmm -> K5 acm_gemm (X^T dZ, dZ Wcat^T)"""

    @staticmethod
    def forward(ctx, x, w_low, w_high, w_mlp, v_low, v_high, v_mlp, v_struc, struc_low, att_mix, lnw_low, lnw_high, lnw_mlp,
                lnw_struc, lnb_low, lnb_high, lnb_mlp, lnb_struc, ops, cfg, post_relu, post_scale, post_drop, call, tail_layer,
                agg_holder, in_drop, pregathered):
        # a block input (functional.blocks): ``x`` is its projection Z, whose Function takes dZ from this layer's backward
        blocks_z = ctx.blocks_z = pregathered is PROJECTED
        x = _conv_prologue(ctx, x, w_low, ops, post_relu, post_scale, post_drop, call, in_drop, projected=blocks_z)
        call, post_scale = ctx.call, ctx.post_scale
        sparse_x = isinstance(x, SparseFeatures)
        dev, n = x.device, x.shape[0]
        f_in, f = w_low.shape
        k = cfg.n_channels
        four = k == 4
        general = bool(getattr(ops, "general", False))
        # k-hop low-pass channel (ACM-SGC, ACM-Pytorch/utils.py:631-637 materialises the dense A_low^k): here the
        # chain A_low (A_low (... Z_L)) with the 1-hop operator, adj_high stays 1-hop like the reference's
        hops = ctx.hops = int(getattr(ops, "hops", 1))
        if hops > 1 and (cfg.relu_before or cfg.relu_after or four or general):
            raise NotImplementedError("hops > 1 is the ACM-SGC chain: model_type 'acmsgc' only")
        if general and ops.sharded:
            raise NotImplementedError("general operator pairs are not row-sharded")
        zero_padded = x.shape[1] != f_in and not blocks_z
        if zero_padded:
            x = x[:, :f_in].contiguous()
        w3 = tuple(_as_f32c(t, "weight") for t in (w_low, w_high, w_mlp))
        x, zlh, zi, zg = _literal_project(ctx, x, w3, ops, cfg)
        fb = ctx.fb
        if four and general:
            if ops.un is None:
                raise RuntimeError("structure_info=1 needs adj_low_unnormalized")
            s_local = _as_f32c(struc_low, "struc_low")
        elif four:
            s_local, s_gath = _struc_rows(ops, struc_low, n)
        vecs, lnw, lnb, mix = _head_params(cfg, (v_low, v_high, v_mlp, v_struc), att_mix, (lnw_low, lnw_high, lnw_mlp, lnw_struc),
                                           (lnb_low, lnb_high, lnb_mlp, lnb_struc))
        out = torch.empty(n, f, dtype=_F32, device=dev)
        att = torch.empty(n, 4, dtype=_F32, device=dev)
        pre = torch.empty(n, (k - 1) * f, dtype=_F32, device=dev)
        p = _lib.ConvFwd()
        p.f_out, p.row_offset = f, ops.row_offset
        _set_head(p, cfg, vecs, lnw, lnb, mix)
        if ops.implicit:
            p.row_scale = ops.row_scale.data_ptr()
        graph = ops.low
        if general:
            # every channel through its own operator, then the fused kernel over the identity operator as a
            # row-local epilogue: pre_L = 1*PL, pre_H = PH - 1*0, pre_S = 1*(1*PS) - 0
            pl = spmm(ops.low, zlh[:, :f])
            ph = spmm(ops.high, zlh[:, fb:fb + f])
            zero = ops.zeros(n, f)
            graph = ops.eye
            p.g_low, p.ld_g_low = pl.data_ptr(), pl.stride(0)
            p.g_high, p.ld_g_high = zero.data_ptr(), zero.stride(0)
            p.s_high, p.ld_s_high = ph.data_ptr(), ph.stride(0)
            if four:
                ps = spmm(ops.un, s_local)
                ones = ops.zeros(n, 1).new_ones(n)
                p.g_struc, p.ld_g_struc = ps.data_ptr(), ps.stride(0)
                p.s_struc, p.ld_s_struc = zero.data_ptr(), zero.stride(0)
                p.deg = ones.data_ptr()
            keep_alive = (pl, ph, zero) + ((ps, ones) if four else ())      # noqa: F841  (until the launch below)
        else:
            if cfg.gather_bf16 and 8 < f <= 64 and f % 2 == 0:
                # bf16 copy of the gathered operand(s): half the gather bytes, fp32 accumulation; the self rows
                # (s_high / s_mlp / s_struc) stay fp32
                zb = cast_bf16(zg[:, : 2 * f])
                p.gather_bf16 = 1
                p.g_low, p.ld_g_low = zb.data_ptr(), zb.stride(0)
                p.g_high, p.ld_g_high = zb.data_ptr() + 2 * f, zb.stride(0)
                if four:
                    sb = cast_bf16(s_gath)
                    p.g_struc, p.ld_g_struc = sb.data_ptr(), sb.stride(0)
            else:
                p.g_low, p.ld_g_low = zg.data_ptr(), zg.stride(0)
                p.g_high, p.ld_g_high = zg.data_ptr() + 4 * fb, zg.stride(0)
                if four:
                    p.g_struc, p.ld_g_struc = s_gath.data_ptr(), s_gath.stride(0)
                    if (f == 2 and fb == 2 and zg is zlh and zlh.stride(0) == 8 and zlh.data_ptr() % 32 == 0 and s_gath is s_local
                            and zlh.untyped_storage().nbytes() - zlh.storage_offset() * 4 >= n * 32):
                        # packed rows (this call's _narrow_tables, or the producing layer's epilogue): the parameter's rows
                        # are copied beside [Z_L | Z_H] -- one small launch for half the lines of the gather
                        torch.as_strided(zlh, (n, 2), (8, 1), zlh.storage_offset() + 4).copy_(s_local)
                        p.g_struc, p.ld_g_struc = zlh.data_ptr() + 16, 8
            p.s_high, p.ld_s_high = zlh.data_ptr() + 4 * fb, zlh.stride(0)
            if four:
                p.s_struc, p.ld_s_struc = s_local.data_ptr(), s_local.stride(0)
                p.deg = ops.deg.data_ptr()
        p.s_mlp, p.ld_s_mlp = zi.data_ptr(), zi.stride(0)
        p.out, p.ld_out = out.data_ptr(), out.stride(0)
        p.pre, p.ld_pre = pre.data_ptr(), pre.stride(0)
        p.att = att.data_ptr()
        _set_post(p, ctx.post_relu, post_scale, ctx.post_drop, ops.row_offset)
        ws = graph.workspace((k - 1) * f)
        # output layer + loss + K3 in one row pass (acm_conv_fwd_tail) when a training loop asked for it
        tail_req = call.tail
        ctx.tail = None
        st = None
        if (tail_req is not None and tail_req.out is None and tail_layer and not general and k == 3 and f <= 8
                and not cfg.gather_bf16 and not post_relu and post_scale is None and post_drop is None
                and any(ctx.needs_input_grad) and tail_req.labels.numel() == n
                and (graph.n_long_rows == 0 or 12.0 < graph.nnz / max(graph.n_rows, 1) <= 160.0)):
            st = _fwd_tail(ctx, ops, cfg, graph, p, ws, tail_req, w3, pre, zi, vecs, lnw, lnb, mix, out)
        if st != 0:
            launch("acm_conv_fwd", f"conv_fwd/F{f}k{k}", dev, graph.handle, C.byref(p), _vp(ws), ws.numel() * 4)
        ctx.ops, ctx.cfg = ops, cfg
        ctx.sparse_x = x if sparse_x else None
        # Lazy input gradient: when the input IS the output of an aggregate-first layer of the same model call and the model
        # vouches that nothing else consumes it (the call's HiddenLink), this layer's backward may hand dX = dZ Wcat^T and
        # dW = X^T dZ to that layer's backward kernel (acm_conv_agg_bwd_t.proj_*) instead of running acm_proj_bwd: the [n, F]
        # gradient then never exists in memory.  The ctx keeps the link only where ``x`` is its activation.
        link = None if sparse_x else call.link
        lazy = (link is not None and link.carries_gradient_of(x) and not zero_padded
                and lazy_hidden_why_not(call.defer, hops) is None)
        if lazy:
            link.lazy_agreed = True
        # left unwritten: only the lazy backward does without its bytes -- a layer that will not go lazy writes it now (the
        # backward's acm_proj_bwd / acm_gemm reads x); one that means to keeps the link, to write it should its backward take
        # another branch after all (call.grad_enabled: a forward under no_grad has no backward to read x)
        unwritten = link is not None and link.unwritten(x)
        if unwritten and not lazy and any(ctx.needs_input_grad) and call.grad_enabled:
            link.ensure_written(x)
        ctx.link = link if (lazy or unwritten) else None
        ctx.save_for_backward(w3[0] if sparse_x else x, *w3, zlh, zi, pre, *_pack_head(vecs, lnw, lnb, mix))
        ctx.mark_non_differentiable(att)
        return out, att

    @staticmethod
    def backward(ctx, grad_out, _grad_att):
        if grad_out is None:
            return _NO_GRADS
        return _literal_backward(ctx, grad_out)


def _fwd_tail(ctx, ops, cfg, graph, p, ws, tail_req, w3, pre, zi, vecs, lnw, lnb, mix, out):
    """acm_conv_fwd_tail: the output layer's K2, the loss the training loop asked for (call.tail) and K3 in one row pass;
    returns its status (None: no workspace for it; 4 = ACM_EUNSUPPORTED: the layer does not qualify, three calls then)."""
    call = ctx.call
    (n, f), k, dev = out.shape, cfg.n_channels, out.device
    dlog = torch.empty(n, f, dtype=_F32, device=dev)
    st3 = _k3_setup(cfg, ops, k, f, n, dev, 0 if ctx.blocks_z else w3[0].shape[0], pre, zi, vecs, lnw, lnb, mix, dlog, False, None, None,
                    fb=ctx.fb)
    loss = torch.empty((), dtype=_F32, device=dev)
    lo = _lib.Loss()
    lo.n_classes = f
    y = tail_req.labels.to(torch.int64).contiguous().reshape(-1)
    w_row = _as_f32c(tail_req.row_weight, "row_weight")
    lo.labels, lo.row_weight = y.data_ptr(), w_row.data_ptr()
    lo.loss, lo.dlogits, lo.ld_dlogits = loss.data_ptr(), dlog.data_ptr(), dlog.stride(0)
    q = st3["q"]
    q.defer = call.defer_ptr()
    nbytes = _workspace_bytes("acm_conv_fwd_tail_workspace_bytes", n, f, k, or_none=True)
    if nbytes is None:
        return None
    wt = torch.empty(max(nbytes // 4, 1), dtype=_F32, device=dev)
    # over the operators' loss-row attachment where the request carries one (rows of weight 0 are then neither gathered nor
    # finished: acm_conv_fwd_tail_rows); ACM_EUNSUPPORTED, a library without the symbol or stale weights: the full call
    ctx.loss_rows = None
    st, lr = EUNSUPPORTED, getattr(tail_req, "loss_rows", None)
    if (lr is not None and f <= 4 and graph is ops.low and not ops.sharded and lr.current_for(tail_req.row_weight)
            and getattr(_lib.load(), "acm_conv_fwd_tail_rows", None) is not None):
        need = lr.fwd["slots"] * (k - 1) * f
        wsr = ws if ws.numel() >= need else torch.empty(need, dtype=_F32, device=dev)     # (the list numbers its own partial slots)
        st = launch("acm_conv_fwd_tail_rows", f"conv_fwd_tail/F{f}k{k}", dev, graph.handle, C.byref(p), C.byref(lo), C.byref(q), _vp(wsr),
                    wsr.numel() * 4, _vp(wt), nbytes, unsupported_ok=True)
        if st == 0:
            ctx.loss_rows = lr
            tail_req.used_loss_rows = True
    if st == EUNSUPPORTED:
        st = launch("acm_conv_fwd_tail", f"conv_fwd_tail/F{f}k{k}", dev, graph.handle, C.byref(p), C.byref(lo), C.byref(q), _vp(ws),
                    ws.numel() * 4, _vp(wt), nbytes, unsupported_ok=True)
    if st == 0:
        st3["keep"] = (y, w_row, wt)
        ctx.tail = st3
        tail_req.loss, tail_req.dz, tail_req.out = loss, dlog, out
        if call.defer is not None:
            call.defer.hold(wt, [loss, st3["d_mix"], *st3["d_vec"], *st3["d_lnw"], *st3["d_lnb"]], keep=[loss, st3["flat"]])
    return st


def _ensure_x_written(ctx, x):
    """The backward is about to read x: a hidden activation its layer left unwritten (ctx.link) is written first."""
    if getattr(ctx, "link", None) is not None:
        ctx.link.ensure_written(x)


def _k3_backward(ctx, grad_out):
    """First stage of the backward of the literal layout (_AcmLiteral, and _AcmAcmii's): its saved tensors, and K3
    (acm_conv_bwd_local) into the G tables, dZ and the flat buffer of the replicated-parameter gradients -- unless
    acm_conv_fwd_tail already ran it with exactly this gradient.  Returns (x, w3, zlh, st3): st3 as _k3_setup's, holding
    this call's own gradient views."""
    ops, cfg, defer = ctx.ops, ctx.cfg, ctx.call.defer
    k = cfg.n_channels
    saved = ctx.saved_tensors
    x, wl, wh, wm, zlh, zi, pre = saved[:7]
    vecs, lnw, lnb, mix = _unpack_head(saved, cfg, 7)
    dev = zlh.device
    n, f = zlh.shape[0], wl.shape[1]
    grad_out = _as_f32c(grad_out, "grad_out")
    tail = ctx.tail
    done = tail is not None and grad_out.data_ptr() == tail["grad_out"].data_ptr()
    # (a block input: the weight gradients belong to the projection's own Function -- no room for them in this layer's buffer)
    f_in_w = 0 if getattr(ctx, "blocks_z", False) else wl.shape[0]
    st3 = tail if done else _k3_setup(cfg, ops, k, f, n, dev, f_in_w, pre, zi, vecs, lnw, lnb, mix, grad_out,
                                      ctx.post_relu, ctx.post_scale, ctx.post_drop, fb=ctx.fb)
    if done:
        ctx.tail = None
    elif getattr(ctx, "mask_table", None) is not None:
        st3["q"].g_scale = None              # the mask form's backward scales by 1 / d_i itself: G_L, G_H as they are
    d_vec, d_lnw, d_lnb, d_mix = _flat_views(st3["flat"], st3["nw"], k, f, cfg.layernorm)    # this call's own view objects
    st3.update(d_vec=d_vec, d_lnw=d_lnw, d_lnb=d_lnb, d_mix=d_mix)
    if not done:                 # else: acm_conv_fwd_tail already ran K3 with exactly this gradient
        ws = _workspace(dev, "acm_conv_bwd_local_workspace_bytes", n, f, k)
        q = st3["q"]
        q.defer = defer.pointer() if defer is not None else None
        launch("acm_conv_bwd_local", f"conv_bwd_local/F{f}k{k}", dev, n, C.byref(q), _vp(ws), ws.numel() * 4)
        if defer is not None:
            defer.hold(ws, [d_mix, *d_vec, *d_lnw, *d_lnb], keep=[st3["flat"]])
    return x, (wl, wh, wm), zlh, st3


def _literal_backward(ctx, grad_out):
    """Backward of the literal layout: K3 (_k3_backward) -> K4 acm_conv_bwd_spmm (the transposed products; ACMII: with the
    ReLU masks of the projected features) [-> the k-hop chain's remaining transposed hops] -> K5 (dWcat = X^T dZ, dX)."""
    x, w3, zlh, s = _k3_backward(ctx, grad_out)
    ops, cfg, defer = ctx.ops, ctx.cfg, ctx.call.defer
    g, dz, gs, flat, nw, ones = s["g"], s["dz"], s["gs"], s["flat"], s["nw"], s["ones"]
    k, fb, dev = cfg.n_channels, ctx.fb, dz.device
    four = k == 4
    n, (f_in_w, f) = dz.shape[0], w3[0].shape
    d_struc = torch.empty(n, f, dtype=_F32, device=dev) if four else None
    r = _lib.ConvBwdSpmm()
    r.f_out, r.row_offset = f, ops.row_offset
    if s["general"]:
        # transposed products channel by channel, then the fused kernel over the identity operator applies the
        # ACMII masks: dZ_L = m*(1*T_L), dZ_H = m*(T_H - 1*0), dS = 1*T_S - 0
        t_l = spmm(ops.low.transpose(), g[:, :f])
        t_h = spmm(ops.high.transpose(), g[:, fb:fb + f])
        zero = ops.zeros(n, f)
        low_t = ops.eye
        r.g_low, r.ld_g_low = t_l.data_ptr(), t_l.stride(0)
        r.g_high, r.ld_g_high = zero.data_ptr(), zero.stride(0)
        r.s_high, r.ld_s_high = t_h.data_ptr(), t_h.stride(0)
        if four:
            t_s = spmm(ops.un.transpose(), gs)
            r.g_struc, r.ld_g_struc = t_s.data_ptr(), t_s.stride(0)
            r.s_struc, r.ld_s_struc = zero.data_ptr(), zero.stride(0)
            r.inv_deg = ones.data_ptr()
            r.d_struc, r.ld_d_struc = d_struc.data_ptr(), d_struc.stride(0)
    else:
        gg = _pkg._gather_rows(ops, g)
        gsg = _pkg._gather_rows(ops, gs) if four else None
        low_t = ops.low_t
        if cfg.gather_bf16 and 8 < f <= 64 and f % 2 == 0 and fb == f:
            # bf16 copies of the gathered gradient tables: half the bytes of the fabric-bound transposed products (the
            # self terms and every sum stay fp32); opt-in, BASELINE config 3's tolerance
            gb = cast_bf16(gg[:, : 2 * f])
            r.gather_bf16 = 1
            r.g_low, r.ld_g_low = gb.data_ptr(), gb.stride(0)
            r.g_high, r.ld_g_high = gb.data_ptr() + 2 * f, gb.stride(0)
            if four:
                gsg = cast_bf16(gsg)
        else:
            r.g_low, r.ld_g_low = gg.data_ptr(), gg.stride(0)
            r.g_high, r.ld_g_high = gg.data_ptr() + 4 * fb, gg.stride(0)
        r.s_high, r.ld_s_high = g.data_ptr() + 4 * fb, g.stride(0)
        if four:
            r.g_struc, r.ld_g_struc = gsg.data_ptr(), gsg.stride(0)
            r.s_struc, r.ld_s_struc = gs.data_ptr(), gs.stride(0)
            r.inv_deg = None if ops.implicit else ops.inv_deg.data_ptr()
            r.d_struc, r.ld_d_struc = d_struc.data_ptr(), d_struc.stride(0)
        if ops.implicit:
            r.self_scale = ops.self_scale.data_ptr()
    if cfg.relu_before:                       # ACMII: ReLU mask of the projected features
        r.mask_low, r.ld_mask_low = zlh.data_ptr(), zlh.stride(0)
        r.mask_high, r.ld_mask_high = zlh.data_ptr() + 4 * fb, zlh.stride(0)
    r.dz_low, r.ld_dz_low = dz.data_ptr(), dz.stride(0)
    r.dz_high, r.ld_dz_high = dz.data_ptr() + 4 * f, dz.stride(0)
    ws2 = low_t.workspace((k - 1) * f)
    launch("acm_conv_bwd_spmm", f"conv_bwd_spmm/F{f}k{k}", dev, low_t.handle, C.byref(r), _vp(ws2), ws2.numel() * 4)
    if ctx.hops > 2 and ops.implicit:
        # the remaining k - 1 >= 2 transposed hops of the low channel with a pattern-only operator:
        # (P D^-1)^(k-1) t = P [D^-1 P]^(k-2) (D^-1 t) -- ONE input scaling, then k - 2 row-scaled products (the forward's
        # form) and a final plain one written over dZ_L (it reads a hop buffer), instead of a scaling pass per hop
        sc = _hop_buffer(dz, f)
        torch.mul(dz[:, :f], ops.row_scale[:, None], out=sc)
        for hop in range(ctx.hops - 2):
            sc = spmm(ops.low_t, _pkg._gather_rows(ops, sc), out=_hop_buffer(dz, f), row_scale=ops.row_scale)
        spmm(ops.low_t, _pkg._gather_rows(ops, sc), out=dz[:, :f])
    elif ctx.hops > 1:                                # the remaining k-1 transposed hops of the low channel
        t = dz[:, :f]
        last = ctx.hops - 2
        for hop in range(ctx.hops - 1):               # the last hop writes dZ_L in place unless it reads it
            t = _low_product(ops, t, transpose=True, out=dz[:, :f] if (hop == last and hop > 0) else None)
        if last == 0:
            dz[:, :f] = t

    if getattr(ctx, "blocks_z", False):
        # a block input: dZ (masked above for ACMII) goes to the projection's backward (functional.blocks._ProjectBlocks), in Z's
        # layout -- channel blocks of fb columns; no gemm / proj_bwd here, and no weight gradient from this Function
        if fb == f:
            d_z = dz
        else:
            d_z = dz.new_zeros(n, 2 * fb + f)
            for c in range(3):
                d_z[:, c * fb:c * fb + f] = dz[:, c * f:(c + 1) * f]
        _reduce_replicated(flat, ops, defer)
        return _grads(d_z, (None, None, None), s["d_vec"], d_struc, s["d_mix"], s["d_lnw"], s["d_lnb"])
    if ctx.sparse_x is not None:                                          # dWcat = X_csr^T dZ
        xs = ctx.sparse_x
        xt = xs.csr_t
        d_wcat = spmm_v(xt, xs.values.index_select(0, xt.src_pos), dz, out=flat[:nw].view(f_in_w, 3 * f))
        d_x = None
    elif (ctx.needs_input_grad[0] and proj_bwd_supported(3 * f)
          and w3[0].stride(0) == w3[1].stride(0) == w3[2].stride(0)):
        d_wcat = flat[:nw].view(3, f_in_w, f)                             # narrow output layer: dX and dW in one
        link = getattr(ctx, "link", None)
        if (link is not None and link.awaits_lazy() and f <= 2 and f_in_w == 64 and x.shape[1] == 64
                and all(w.stride(0) == f and w.is_contiguous() for w in w3)):
            # ... left to the producing layer's backward kernel: the placeholder is what autograd carries there
            d_x = torch.empty(n, x.shape[1], dtype=_F32, device=dev)
            link.lazy = LazyGrad(dz, w3, d_wcat, x, d_x)
        else:
            _ensure_x_written(ctx, x)
            d_x = proj_bwd(x, dz, w3, d_wcat, defer=defer)                # pass over x (acm_proj_bwd)
    else:
        _ensure_x_written(ctx, x)
        d_wcat = gemm(x, dz, trans_a=True, col_blocks=3,
                      out=flat[:nw].view(3, f_in_w, f),                   # contiguous per weight
                      a_drop=_drop_spec(ctx.in_drop, ops.row_offset) if getattr(ctx, "in_drop_used", False) else None)
        d_x = gemm(dz, torch.cat(w3, dim=1), trans_b=True) if ctx.needs_input_grad[0] else None
    if d_x is not None and d_x.shape[1] != ctx.x_width:
        d_x = torch.nn.functional.pad(d_x, (0, ctx.x_width - d_x.shape[1]))
    _reduce_replicated(flat, ops, defer)
    if d_wcat.dim() == 3:
        d_w3 = (d_wcat[0], d_wcat[1], d_wcat[2])
    else:
        d_w3 = tuple(d_wcat[:, i * f:(i + 1) * f] for i in range(3))
    return _grads(d_x, d_w3, s["d_vec"], d_struc, s["d_mix"], s["d_lnw"], s["d_lnb"])


class _AcmAcmii(torch.autograd.Function):
    """out, att = ACMII layer that recomputes relu(x_j [W_L | W_H]) per edge from the gathered narrow input rows
    (_acmii_shape; arguments as _AcmAggFirst).

    forward : the mask form (pattern-only operator, input without gradient): acm_acmii_table -> acm_conv_acmii_v_fwd; else (or
              ACM_EUNSUPPORTED) the fp32 acm_conv_acmii_fwd, which leaves the literal form's saved layout
    backward: mask form: acm_conv_bwd_local -> acm_conv_acmii_v_bwd (all three weight gradients) [-> spmm_sub];
              else the literal backward (_literal_backward)"""

    @staticmethod
    def forward(ctx, x, w_low, w_high, w_mlp, v_low, v_high, v_mlp, v_struc, struc_low, att_mix, lnw_low, lnw_high, lnw_mlp,
                lnw_struc, lnb_low, lnb_high, lnb_mlp, lnb_struc, ops, cfg, post_relu, post_scale, post_drop, call, tail_layer,
                agg_holder, in_drop, pregathered):
        x = _conv_prologue(ctx, x, w_low, ops, post_relu, post_scale, post_drop, call, in_drop)
        dev, n = x.device, x.shape[0]
        f_in, f = w_low.shape
        k = cfg.n_channels
        four = k == 4
        fp = 8
        zero_padded = x.shape[1] != f_in
        x, xpad, xg, _, _ = _gathered_input(ctx, x, ops, f_in, f, fp, agg_holder, pregathered, False)
        w3 = wl, wh, wm = tuple(_as_f32c(t, "weight") for t in (w_low, w_high, w_mlp))
        x = x[:, :f_in].contiguous() if zero_padded else x      # saved for K5 (dWcat = X^T dZ)
        if four:
            s_local, s_gath = _struc_rows(ops, struc_low, n)
        vecs, lnw, lnb, mix = _head_params(cfg, (v_low, v_high, v_mlp, v_struc), att_mix, (lnw_low, lnw_high, lnw_mlp, lnw_struc),
                                           (lnb_low, lnb_high, lnb_mlp, lnb_struc))
        out = torch.empty(n, f, dtype=_F32, device=dev)
        att = torch.empty(n, 4, dtype=_F32, device=dev)
        zlh = torch.empty(n, 2 * f, dtype=_F32, device=dev)
        zi = torch.empty(n, f, dtype=_F32, device=dev)
        pre = torch.empty(n, (k - 1) * f, dtype=_F32, device=dev)
        p = _lib.ConvAcmiiFwd()
        p.f_in, p.f_pad, p.f_out = f_in, fp, f
        _set_head(p, cfg, vecs, lnw, lnb, mix)
        if four:                                  # ps = A_low S: one F-wide single-channel gather of the parameter
            ps = spmm(ops.low, s_gath, row_scale=ops.row_scale if ops.implicit else None, bf16=cfg.gather_bf16)
            p.ps, p.ld_ps = ps.data_ptr(), ps.stride(0)
            p.ss, p.ld_ss = s_local.data_ptr(), s_local.stride(0)
            p.deg = ops.deg.data_ptr()
        p.xg, p.ld_xg = xg.data_ptr(), xg.stride(0)
        p.xs, p.ld_xs = xpad.data_ptr(), xpad.stride(0)
        p.w_low, p.w_high, p.w_mlp, p.ld_w = wl.data_ptr(), wh.data_ptr(), wm.data_ptr(), f
        p.out, p.ld_out = out.data_ptr(), out.stride(0)
        p.pre, p.ld_pre = pre.data_ptr(), pre.stride(0)
        p.att = att.data_ptr()
        p.zlh, p.ld_zlh = zlh.data_ptr(), zlh.stride(0)
        p.zi, p.ld_zi = zi.data_ptr(), zi.stride(0)
        if ops.implicit:
            p.row_scale = ops.row_scale.data_ptr()
        _set_post(p, ctx.post_relu, ctx.post_scale, ctx.post_drop, ops.row_offset)
        ws = _workspace(dev, "acm_conv_acmii_fwd_workspace_bytes", ops.low.handle)
        # The mask form (acm_conv_acmii_v.hip): relu(x_j W) = m_j * (x_j W), so the aggregate is W contracted with
        # V_i = sum_j m_j (x) x_j -- a product over the neighbour index on the bf16 matrix pipe, exact operands -- and the
        # weight gradients are the same V contracted with dH: no transposed product for them (the structure channel's
        # parameter keeps its one F-wide transposed product).  A pattern-only operator over this process's own rows, no
        # gradient into x.
        ctx.mask_table = None
        if (ops.implicit and not ctx.needs_input_grad[0] and n > 0 and xg.shape[0] == ops.low.n_cols
                and (tuning.HOST.rewrites & tuning.REWRITE_ACMII_MASK) != 0
                and (getattr(ops.low, "item_stream_waves", 0) > 0         # one-off per operator (synchronises: never
                     or (not _capturing(dev) and ops.low.build_item_streams()))):     # inside a capture, whose warm-up built them)
            # the table covers every column of the operator: this process's rows, or (row-sharded) the all-gathered input --
            # each rank evaluates the masks of its halo itself, and its backward then needs NO all-gather of gradients
            ng = xg.shape[0]
            tb = _workspace_bytes("acm_acmii_table_bytes", ng)
            table = torch.empty(tb // 4, dtype=torch.int32, device=dev)
            st = launch("acm_acmii_table", f"acmii_table/{ng}x{f_in}", dev, ng, f_in, xg.data_ptr(), xg.stride(0), wl.data_ptr(), wh.data_ptr(),
                        f, table.data_ptr(), tb, unsupported_ok=True)
            if st == 0:
                if ops.low.n_long_rows == 0:          # only the fix-up of long rows reads zlh (its high-pass half)
                    p.zlh, p.ld_zlh = None, 0
                st = launch("acm_conv_acmii_v_fwd", f"conv_acmii_v_fwd/F{f}i{f_in}", dev, ops.low.handle, C.byref(p), table.data_ptr(), _vp(ws),
                            ws.numel() * 4, unsupported_ok=True)
                if st == 0:
                    ctx.mask_table, ctx.mask_x = table, xpad
                    ctx.mask_self_offset = 0
                    if ops.sharded:                   # this rank's rows inside the gathered numbering (_gather_rows)
                        import torch.distributed as dist
                        ctx.mask_self_offset = dist.get_rank(ops.group) * (ops.n_gathered // dist.get_world_size(ops.group))
                else:                                 # refused (ACM_EUNSUPPORTED): the fp32 kernel below
                    p.zlh, p.ld_zlh = zlh.data_ptr(), zlh.stride(0)
        if ctx.mask_table is None:
            launch("acm_conv_acmii_fwd", f"conv_acmii_fwd/F{f}i{f_in}", dev, ops.low.handle, C.byref(p), _vp(ws), ws.numel() * 4)
        ctx.ops, ctx.cfg = ops, cfg
        ctx.tail, ctx.sparse_x, ctx.hops, ctx.fb = None, None, 1, f        # (what _literal_backward reads)
        ctx.save_for_backward(x, *w3, zlh, zi, pre, *_pack_head(vecs, lnw, lnb, mix))
        ctx.mark_non_differentiable(att)
        return out, att

    @staticmethod
    def backward(ctx, grad_out, _grad_att):
        if grad_out is None:
            return _NO_GRADS
        if ctx.mask_table is None:
            return _literal_backward(ctx, grad_out)
        # the mask form's backward: dW_L, dW_H straight from dH_L, dH_H (K3's g) over the FORWARD operator and the
        # forward's table, and the row-local dW_I = X^T dZ_I in the same launch
        ops, defer = ctx.ops, ctx.call.defer
        _, w3, _, s = _k3_backward(ctx, grad_out)
        g, dz, flat = s["g"], s["dz"], s["flat"]
        f_in, f = w3[0].shape
        d_wcat = flat[:s["nw"]].view(3, f_in, f)
        xt = ctx.mask_x
        b = _lib.ConvAcmiiBwd()
        b.f_in, b.table = f_in, ctx.mask_table.data_ptr()
        b.g_low, b.ld_g_low = g.data_ptr(), g.stride(0)
        b.g_high, b.ld_g_high = g.data_ptr() + 4 * ctx.fb, g.stride(0)
        b.g_mlp, b.ld_g_mlp = dz.data_ptr() + 8 * f, dz.stride(0)
        b.x, b.ld_x = xt.data_ptr(), xt.stride(0)
        b.self_offset = ctx.mask_self_offset
        b.row_scale = ops.row_scale.data_ptr()
        b.d_w_low, b.d_w_high, b.d_w_mlp, b.ld_dw = d_wcat[0].data_ptr(), d_wcat[1].data_ptr(), d_wcat[2].data_ptr(), f
        b.defer = defer.pointer() if defer is not None else None
        wsb = _workspace(dz.device, "acm_conv_acmii_v_bwd_workspace_bytes", ops.low.handle)
        launch("acm_conv_acmii_v_bwd", f"conv_acmii_v_bwd/F{f}i{f_in}", dz.device, ops.low.handle, C.byref(b), _vp(wsb), wsb.numel() * 4)
        if defer is not None:
            defer.hold(wsb, [d_wcat[0], d_wcat[1], d_wcat[2]], keep=[flat, ctx.mask_table, g, dz, xt])
        # (pattern-only: K3 left G_S unscaled)
        d_struc = _struc_grad(ops, ctx.cfg, s["gs"]) if ctx.cfg.n_channels == 4 else None
        _reduce_replicated(flat, ops, defer)
        return _grads(None, (d_wcat[0], d_wcat[1], d_wcat[2]), s["d_vec"], d_struc, s["d_mix"], s["d_lnw"], s["d_lnb"])
