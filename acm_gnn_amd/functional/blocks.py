"""The projection of a layer input given as COLUMN BLOCKS [x | h_0 | ... | h_{k-1}] -- ACM-Snowball's layers
(ACM-Geometric/models.py:57-64) -- without the concatenation:

    [x | h_0 | ...] [W_L | W_H | W_I] = x W[0 : nfeat] + sum_j h_j W[r_j : r_j + w_j]

The feature block's term is a product the library has (acm_spmm_v for SparseFeatures, acm_gemm for a dense block), the dense
blocks' terms are acm_proj_blocks_fwd; the backward (acm_proj_blocks_bwd) writes dH_j and the weight-gradient rows of every
dense block, the feature block's weight rows come from the transposed CSR product -- no [n, nfeat + k nhid] tensor and no
full-width input gradient exist.  ``project_blocks`` is the public operator; the literal layer adopts its result
(conv_literal._literal_project) and hands its dZ to this Function's backward."""
import ctypes as C

import torch

from .. import _lib
from ..graph import SparseFeatures
from ._context import _call_or_ambient, _run
from ._conv_shared import _chan_block, _z_pitch
from ._launch import EUNSUPPORTED, _F32, _as_f32_rows, _as_f32c, _vp, _workspace_bytes, launch
from .gcn import mask_bwd
from .ops import gemm, spmm_v

MAX_BLOCKS = _lib.PROJ_BLOCKS_MAX


def check_blocks(blocks, in_features=None, device=None, n_rows=None):
    """The blocks of a block input: ``blocks[0]`` a SparseFeatures or a dense [n, w] tensor, the rest dense fp32 [n, w_j] on the
    same device.  A bad width, dtype, device or row count raises ValueError naming the block; returns the widths."""
    if not isinstance(blocks, (list, tuple)) or len(blocks) == 0:
        raise ValueError("a block input is a non-empty list or tuple of column blocks")
    widths = []
    for j, b in enumerate(blocks):
        if isinstance(b, SparseFeatures):
            if j != 0:
                raise ValueError(f"block {j}: only the first block may be SparseFeatures")
            dev = b.values.device
        elif isinstance(b, torch.Tensor):
            if b.layout != torch.strided or b.dim() != 2:
                raise ValueError(f"block {j}: a dense 2-D tensor is required (got {tuple(b.shape)}, {b.layout})")
            if b.dtype != _F32:
                raise ValueError(f"block {j}: dtype {b.dtype}, float32 is required")
            dev = b.device
        else:
            raise ValueError(f"block {j}: {type(b).__name__} is neither a tensor nor SparseFeatures")
        if device is None:
            device = dev
        if dev != device:
            raise ValueError(f"block {j}: on {dev}, the layer's weights are on {device}")
        if n_rows is None:
            n_rows = b.shape[0]
        if b.shape[0] != n_rows:
            raise ValueError(f"block {j}: {b.shape[0]} rows, the other blocks / the operator have {n_rows}")
        if b.shape[1] < 1:
            raise ValueError(f"block {j}: no columns")
        widths.append(int(b.shape[1]))
    if in_features is not None and sum(widths) != in_features:
        raise ValueError(f"the blocks are {widths} columns wide ({sum(widths)} in all) but the layer has in_features = {in_features}: "
                         f"block {len(widths) - 1} ends at the wrong column")
    return widths


def _packed_rows(w3, r0, r1, f, fb):
    """[W_L 0 | W_H 0 | W_I][r0 : r1]: the rows of the packed weights a product into Z's layout multiplies with."""
    parts = [w[r0:r1] for w in w3]
    if fb != f:
        zpad = w3[0].new_zeros(r1 - r0, fb - f)
        parts = [parts[0], zpad, parts[1], zpad, parts[2]]
    return torch.cat(parts, dim=1)


def _compact(g, f, fb):
    """[n, 3F] from a table in Z's layout (channel blocks of fb columns); the table itself where fb == F."""
    return g if fb == f else torch.cat([g[:, c * fb:c * fb + f] for c in range(3)], dim=1)


def _kernel_block(b):
    """Whether acm_proj_blocks_* take this dense block (else: the composed form)."""
    return b.shape[1] % 4 == 0 and 4 <= b.shape[1] <= 64


def _struct(w3, f, fb, blocks, rows0):
    p = _lib.ProjBlocks()
    p.n_blocks, p.f, p.f_block, p.f_in = len(blocks), f, fb, w3[0].shape[0]
    p.w_low, p.w_high, p.w_mlp, p.ldw = w3[0].data_ptr(), w3[1].data_ptr(), w3[2].data_ptr(), w3[0].stride(0)
    for j, (b, r0) in enumerate(zip(blocks, rows0)):
        p.h[j], p.ld_h[j], p.width[j], p.row0[j] = b.data_ptr(), b.stride(0), b.shape[1], r0
    return p


class _ProjectBlocks(torch.autograd.Function):
    """Z = act([first | dense_0 | ...] [W_L | W_H | W_I]) in the literal layer's Z layout (channel blocks of _chan_block(F)
    columns), arguments (relu, mask_grad, call, W_L, W_H, W_I, first, *dense).

    forward : acm_spmm_v / acm_gemm (the feature block) -> acm_proj_blocks_fwd (the dense blocks, + ReLU)
    backward: [acm_bias_act_bwd: the ReLU mask, ``mask_grad`` -- the literal layer hands dZ over masked] -> acm_proj_blocks_bwd
              (dH_j, dW rows of the dense blocks) -> acm_spmm_v on the transposed features / acm_gemm (dW rows of the feature block).
    No gradient for the feature block.  Outside the kernels' envelope (a width that is no multiple of 4 or above 64, more than
    eight blocks): the same result from acm_gemm, one call per block and direction."""

    @staticmethod
    def forward(ctx, relu, mask_grad, call, w_low, w_high, w_mlp, first, *dense):
        ctx.call = _call_or_ambient(call)
        w3 = tuple(_as_f32c(t, "weight") for t in (w_low, w_high, w_mlp))
        sparse = isinstance(first, SparseFeatures)
        dev = w3[0].device
        first = first if sparse else _as_f32_rows(first, "block 0")
        dense = tuple(_as_f32_rows(h, f"block {j + 1}") for j, h in enumerate(dense))
        n, (f_in, f) = first.shape[0], w3[0].shape
        fb = _chan_block(f)
        width = 2 * fb + f
        z = torch.empty(n, _z_pitch(f, fb), dtype=_F32, device=dev)[:, :width]
        nfeat = first.shape[1]
        rows0, r = [], nfeat
        for h in dense:
            rows0.append(r)
            r += h.shape[1]
        # the feature block: a dense one the kernel takes rides with the others (without a gradient of its own)
        kernel_first = not sparse and _kernel_block(first)
        blocks, brows, have = list(dense), list(rows0), False
        if kernel_first:
            blocks, brows = [first] + blocks, [0] + brows
        elif sparse:
            if first.csr.nnz > 0 and n > 0:
                spmm_v(first.csr, first.values, _packed_rows(w3, 0, nfeat, f, fb), relu=relu and not blocks, out=z)
                have = True
        else:
            gemm(first, _packed_rows(w3, 0, nfeat, f, fb), relu=relu and not blocks, out=z)
            have = True
        composed = len(blocks) > MAX_BLOCKS or not all(_kernel_block(b) for b in blocks)
        if blocks and not composed:
            p = _struct(w3, f, fb, blocks, brows)
            st = launch("acm_proj_blocks_fwd", f"proj_blocks_fwd/{n}x{3 * f}b{len(blocks)}", dev, n, C.byref(p), _vp(z), z.stride(0),
                        int(have), int(relu), unsupported_ok=True)
            composed = st == EUNSUPPORTED
        if blocks and composed:                   # outside the envelope: one acm_gemm per block, summed, then the ReLU
            for b, r0 in zip(blocks, brows):
                t = gemm(b, _packed_rows(w3, r0, r0 + b.shape[1], f, fb))
                if have:
                    z.add_(t)
                else:
                    z.copy_(t)
                    have = True
            if relu:
                z.clamp_(min=0)
        if not have and not blocks:               # (an empty CSR matrix and nothing else)
            z.zero_()
        ctx.relu, ctx.mask_grad, ctx.sparse = bool(relu), bool(mask_grad), first if sparse else None
        ctx.kernel_first, ctx.composed, ctx.rows0, ctx.fb, ctx.nfeat = kernel_first, composed, rows0, fb, nfeat
        ctx.save_for_backward(*w3, z if (relu and mask_grad) else w3[0], *(() if sparse else (first,)), *dense)
        return z

    @staticmethod
    def backward(ctx, g):
        if g is None:
            return (None,) * (7 + len(ctx.rows0))
        saved = ctx.saved_tensors
        w3, z = saved[:3], saved[3]
        sparse = ctx.sparse
        first = sparse if sparse is not None else saved[4]
        dense = saved[4 if sparse is not None else 5:]
        defer = ctx.call.defer
        f_in, f = w3[0].shape
        fb, nfeat, n, dev = ctx.fb, ctx.nfeat, g.shape[0], g.device
        g = _as_f32_rows(g, "grad")
        if ctx.relu and ctx.mask_grad:
            g = mask_bwd(z, g, 1.0, True)
        needs = ctx.needs_input_grad[7:]
        d_h = [torch.empty(n, h.shape[1], dtype=_F32, device=dev) if need else None for h, need in zip(dense, needs)]
        # CSR features: the transposed product writes [nfeat, 3F] rows, so the whole gradient is kept [f_in, 3F]; else the three
        # weights' gradients are contiguous matrices of their own ([3, f_in, F], acm_gemm_blocks' layout)
        by_cols = sparse is not None
        flat = torch.empty(3 * f_in * f, dtype=_F32, device=dev)
        d_w = flat.view(f_in, 3 * f) if by_cols else flat.view(3, f_in, f)
        layout = (3 * f, 0, 0) if by_cols else (f, f, f_in * f)          # lddw, dw_col_block, dw_block_stride
        blocks, brows, grads = list(dense), list(ctx.rows0), list(d_h)
        if ctx.kernel_first:
            blocks, brows, grads = [first] + blocks, [0] + brows, [None] + grads
        if blocks and not ctx.composed:
            p = _struct(w3, f, fb, blocks, brows)
            for j, t in enumerate(grads):
                if t is not None:
                    p.d_h[j], p.ld_dh[j] = t.data_ptr(), t.stride(0)
            nbytes = _workspace_bytes("acm_proj_blocks_bwd_workspace_bytes", n, C.byref(p))
            ws = torch.empty(max(nbytes // 4, 1), dtype=_F32, device=dev)
            # (deferred only where autograd adopts the gradients as they are: contiguous per-weight matrices)
            use_defer = defer if not by_cols else None
            launch("acm_proj_blocks_bwd", f"proj_blocks_bwd/{n}x{3 * f}b{len(blocks)}", dev, n, C.byref(p), _vp(g), g.stride(0),
                   _vp(flat), *layout, _vp(ws), nbytes, use_defer.pointer() if use_defer is not None else None)
            if use_defer is not None:
                use_defer.hold(ws, [d_w[0], d_w[1], d_w[2]], keep=[flat, g, *blocks, *[t for t in grads if t is not None]])
        elif blocks:                              # composed: per block dH_j = dZ W[r_j ...]^T, dW rows = H_j^T dZ
            gc = _compact(g, f, fb)
            for b, r0, t in zip(blocks, brows, grads):
                r1 = r0 + b.shape[1]
                if t is not None:
                    gemm(gc, torch.cat([w[r0:r1] for w in w3], dim=1), trans_b=True, out=t)
                rows = gemm(b, gc, trans_a=True)                            # [w_j, 3F]
                if by_cols:
                    d_w[r0:r1] = rows
                else:
                    for c in range(3):
                        d_w[c, r0:r1] = rows[:, c * f:(c + 1) * f]
        if sparse is not None:                    # dW[0 : nfeat] = X_csr^T dZ (dZ's channel blocks compacted where they are padded)
            if sparse.csr.nnz > 0 and n > 0:
                xt = sparse.csr_t
                vals_t = sparse.values.index_select(0, xt.src_pos)
                spmm_v(xt, vals_t, _compact(g, f, fb), out=d_w[:nfeat])
            else:
                d_w[:nfeat].zero_()
        elif not ctx.kernel_first:                # a dense feature block outside the kernel's widths
            gc = _compact(g, f, fb)
            rows = gemm(first, gc, trans_a=True)
            for c in range(3):
                d_w[c, :nfeat] = rows[:, c * f:(c + 1) * f]
        if by_cols:
            d_w3 = tuple(d_w[:, c * f:(c + 1) * f] for c in range(3))
        else:
            d_w3 = (d_w[0], d_w[1], d_w[2])
        return (None, None, None, *d_w3, None, *d_h)


def project_blocks(blocks, w3, relu=False, call=None, mask_grad=True):
    """Z = act([blocks[0] | blocks[1] | ...] [W_L | W_H | W_I]) without the concatenation.  ``blocks[0]``: SparseFeatures or a
    dense tensor (the features: no gradient), the rest dense [n, w_j]; ``w3``: the three weights, sum(widths) rows each;
    ``relu``: the ACMII form's ReLU over the complete sum.  Returns Z as the literal layer keeps it: [n, 2 fb + F] with
    fb = the channel block (F, or 4 / 8 for F in {3, 5, 6, 7}), channel c at column c * fb, the pad columns zero.
    ``mask_grad=False``: the caller hands the backward a gradient that is masked already (the literal layer's K4 / K3)."""
    w3 = tuple(w3)
    if len(w3) != 3 or any(w.shape != w3[0].shape or w.dim() != 2 for w in w3):
        raise ValueError("project_blocks: w3 holds the three [f_in, F] weights")
    check_blocks(blocks, in_features=w3[0].shape[0], device=w3[0].device)
    if isinstance(blocks[0], torch.Tensor) and blocks[0].requires_grad:
        raise NotImplementedError("project_blocks: the feature block (blocks[0]) takes no gradient")
    return _run(_ProjectBlocks, bool(relu), bool(mask_grad), call, *w3, blocks[0], *blocks[1:])
