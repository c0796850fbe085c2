"""What the four routes of the fused ACM layer share: the layer's static description (AcmConfig), its gathered tables and
flat gradient buffer, the post-op and head fields of the kernels' structs, the head parameters as saved tensors, the setup of
the row-local backward (K3) and the forwards' common prologue."""
import ctypes as C

import torch

from .. import _lib
from .. import functional as _pkg            # (_gather_rows is called through the package, where tests replace it)
from ..graph import SparseFeatures
from ._context import _call_or_ambient, _sum_over_ranks
from ._launch import _F32, _Timed, _as_f32_rows, _as_f32c, _vp, launch
from .ops import _drop_now, _drop_spec, cast_bf16, spmm


class AcmConfig:
    """Static description of one layer variant (what the reference selects with
    model_type / variant / structure_info, ACM-Geometric/layers.py:78-116)."""

    __slots__ = ("n_channels", "relu_before", "relu_after", "relu_mlp", "layernorm", "scale", "gather_bf16")

    def __init__(self, model_type, variant, structure_info, attn_layernorm, gather_dtype="fp32"):
        if gather_dtype not in ("fp32", "bf16"):
            raise ValueError("gather_dtype must be 'fp32' or 'bf16'")
        self.gather_bf16 = gather_dtype == "bf16"
        plus = model_type in ("acmgcnp", "acmgcnpp", "acmgcn+", "acmgcn++")
        if model_type == "acmsgc":
            self.n_channels, self.relu_before, self.relu_after, self.relu_mlp = 3, False, False, False
            self.layernorm = False
        elif model_type == "acmsnowball":                 # the layer's generic branch: three channels, no LayerNorm, the
            self.n_channels = 3                           # structure channel never (layers.py:59,106-108)
            self.relu_before, self.relu_after, self.relu_mlp = bool(variant), not bool(variant), True
            self.layernorm = False
        else:
            self.n_channels = 4 if (plus and structure_info) else 3
            self.relu_before = bool(variant)          # ACMII: ReLU between projection and filter
            self.relu_after = not bool(variant)       # ACM: ReLU after the filter
            self.relu_mlp = True
            self.layernorm = bool(attn_layernorm) and plus
        self.scale = 1.0 if self.n_channels == 4 else 3.0


def _ptr_array(tensors):
    n = len(tensors)
    return _VP4(*[tensors[i].data_ptr() if i < n and tensors[i] is not None else None for i in range(4)])


_VP4 = C.c_void_p * 4


def _gather_rows(ops, local):
    """All-gather row blocks of a row-sharded dense matrix (halo exchange) into the layout the local operators'
    column ids refer to: rank r's rows start at r * n_max, shorter blocks are zero-padded (distributed.ShardPlan).
    Single process: identity."""
    if not ops.sharded:
        return local
    import torch.distributed as dist
    world = dist.get_world_size(ops.group)
    n_max = ops.n_gathered // world
    local = local.contiguous()
    if local.shape[0] != n_max:                       # work-balanced blocks differ in length
        buf = local.new_zeros(n_max, local.shape[1])
        buf[: local.shape[0]] = local
        local = buf
    full = torch.empty(world * n_max, local.shape[1], dtype=local.dtype, device=local.device)
    with _Timed(f"all_gather/{n_max}x{local.shape[1]}", local.numel() * local.element_size()):
        dist.all_gather_into_tensor(full, local, group=ops.group)
    return full


def _hop_buffer(t_like, width):
    """[n, width] view of a buffer whose rows are padded to the next of 4 / 8 columns: the narrow gather fetches such rows
    as aligned 16-byte blocks (see _chan_block)."""
    pitch = width if width > 8 else (8 if width > 4 else (4 if width > 2 else width))
    return torch.empty(t_like.shape[0], pitch, dtype=_F32, device=t_like.device)[:, :width]


def _low_product(ops, t_local, transpose=False, out=None):
    """A_low @ t (or A_low^T @ t) for a row-local t [n_local, w]: one hop of the ACM-SGC k-hop chain, with the
    halo all-gather when row-sharded.  Pattern-only operators: D^-1 (P t) and P (D^-1 t).  ``out``: where the product
    goes (default: a row-padded buffer, _hop_buffer)."""
    if out is None:
        out = _hop_buffer(t_local, t_local.shape[1])
    if transpose:
        if ops.implicit:
            scaled = _hop_buffer(t_local, t_local.shape[1])
            torch.mul(t_local, ops.row_scale[:, None], out=scaled)
            return spmm(ops.low_t, _pkg._gather_rows(ops, scaled), out=out)
        return spmm(ops.low_t, _pkg._gather_rows(ops, t_local), out=out)
    return spmm(ops.low, _pkg._gather_rows(ops, t_local), out=out, row_scale=ops.row_scale if ops.implicit else None)


def _flat_views(flat, nw, k, f, layernorm):
    """The head-parameter gradients as views of the layer's flat gradient buffer (fresh tensor objects on every call:
    autograd adopts a returned gradient only while nobody else holds that tensor object)."""
    # (one split call: 3 k + 1 views; slicing them one by one costs a layer 30 us of host time)
    if layernorm:
        parts = flat[nw:].split([f] * (3 * k) + [k * k])
        d_vec = [t.view(f, 1) for t in parts[:k]]
        d_lnw, d_lnb = list(parts[k:2 * k]), list(parts[2 * k:3 * k])
    else:
        parts = flat[nw:].split([f] * k + [k * k])
        d_vec, d_lnw, d_lnb = [t.view(f, 1) for t in parts[:k]], [], []
    d_mix = parts[-1].view(k, k)
    return d_vec, d_lnw, d_lnb, d_mix


def _chan_block(f):
    """Column distance of the two gathered channels inside [Z_L | Z_H] / [G_L | G_H].  F in {3, 5, 6, 7} pads each channel
    to a block of 4 / 8 columns: the narrow gather then fetches a neighbour's row with aligned 16-byte loads (the
    merged path of acm_spmm.hip's spmm_narrow_kernel) instead of 2 F scalar ones -- on the arXiv-year-shaped graph (5 classes) the
    output layer's gathers are 3-4x faster.  The pad columns are never read into a result."""
    if f in (3, 5, 6, 7):
        return 4 if f == 3 else 8
    return f


def _z_pitch(f, fb):
    """Row pitch of the one-table Z = [Z_L | Z_H | Z_I]: for narrow layers the gathered block [Z_L | Z_H] (2F floats) must be one
    aligned vector fetch, so rows are padded to a multiple of that block."""
    if f in (2, 4, 8):
        return -(-3 * f // (2 * f)) * (2 * f)
    if fb != f:
        return -(-(2 * fb + f) // 4) * 4
    return 3 * f


def _narrow_tables(n, fb, f, dev, packed):
    """The gathered tables of a narrow layer: ([c0 | c1] block rows, third-channel rows or None).  ``packed`` (four channels
    of two columns: the output layer of a two-class model with structure_info): views of ONE table of 32-byte rows
    [c0 c0 c1 c1 | c2 c2 - -], which the pair-lane gather (acm_gather_device.h: spmm_narrow_pair3_kernel) walks with one line per
    neighbour instead of two."""
    if packed:
        base = torch.empty(n, 8, dtype=_F32, device=dev)
        return base[:, :4], base[:, 4:6]
    return torch.empty(n, 2 * fb, dtype=_F32, device=dev), None


def _set_post(st, post_relu, post_scale, post_drop, row_offset):
    """The fused post-op fields of a kernel's struct: relu(out) * post_scale, or the counter-based dropout ``post_drop``."""
    st.post_relu = int(post_relu)
    if post_scale is not None:
        st.post_scale, st.ld_post_scale = post_scale.data_ptr(), post_scale.stride(0)
    spec = _drop_spec(post_drop, row_offset)
    if spec is not None:
        st.post_drop = spec


def _set_head(st, cfg, vecs, lnw, lnb, mix):
    """The head fields of a kernel's struct: the LayerNorm switch, scale, channel count and the head's parameters -- and the two
    ReLU switches on the structs that declare them (the ACMII forward's does not: its ReLUs are fixed)."""
    st.layernorm, st.scale, st.n_channels = int(cfg.layernorm), cfg.scale, cfg.n_channels
    if hasattr(st, "relu_after"):
        st.relu_after, st.relu_mlp = int(cfg.relu_after), int(cfg.relu_mlp)
    st.att_vec, st.ln_weight, st.ln_bias = _ptr_array(vecs), _ptr_array(lnw), _ptr_array(lnb)
    st.att_mix = mix.data_ptr()


def _head_params(cfg, vecs, att_mix, lnw, lnb):
    """The head's parameters of a layer of cfg.n_channels = k channels: (att_vec list, LayerNorm weights, LayerNorm biases,
    the k x k att_mix), each float32 and contiguous; ``vecs`` / ``lnw`` / ``lnb`` list the four channels' tensors."""
    k = cfg.n_channels
    vecs = [_as_f32c(t, "att_vec") for t in vecs[:k]]
    lnw = [_as_f32c(t, "ln") for t in lnw[:k]] if cfg.layernorm else []
    lnb = [_as_f32c(t, "ln") for t in lnb[:k]] if cfg.layernorm else []
    mix = _as_f32c(att_mix, "att_vec")
    if tuple(mix.shape) != (k, k):
        raise RuntimeError(f"att_vec is {tuple(mix.shape)} but the layer mixes {k} channels "
                           "(structure_info is only valid with acmgcnp/acmgcnpp)")
    return vecs, lnw, lnb, mix


def _pack_head(vecs, lnw, lnb, mix):
    """The head's parameters as they sit in a layer Function's saved tensors: the mix, the k att_vec, then (LayerNorm) the k
    weights and the k biases."""
    return (mix, *vecs, *lnw, *lnb)


def _unpack_head(saved, cfg, at):
    """(vecs, lnw, lnb, mix) back from ``saved[at:]`` (_pack_head's order)."""
    k = cfg.n_channels
    nln = k if cfg.layernorm else 0
    v, w, b = at + 1, at + 1 + k, at + 1 + k + nln
    return list(saved[v:w]), list(saved[w:b]), list(saved[b:b + nln]), saved[at]


def _reduce_replicated(flat, ops, defer):
    """Row-sharded: sum the row-shard partials of the replicated parameters' gradients, ONE all-reduce of the layer's flat
    gradient buffer."""
    if ops.sharded:
        _sum_over_ranks(flat, ops.group, defer)


def _struc_grad(ops, cfg, gs):
    """d struc_low = A_low^T (D G_S) - G_S (pattern-only: P G_S - G_S, G_S unscaled) from the row-local backward's G_S: one
    F-wide transposed product that subtracts the self term in its epilogue, after the all-gather of G_S when row-sharded."""
    n, f = gs.shape
    gsg = _pkg._gather_rows(ops, gs)
    low_t = ops.low_t
    d_struc = torch.empty(n, f, dtype=_F32, device=gs.device)
    ws = low_t.workspace(f)
    o = _lib.SpmmOpts()
    o.sub, o.ld_sub = gs.data_ptr(), gs.stride(0)
    o.sub_scale = None if ops.implicit else ops.inv_deg.data_ptr()
    if cfg.gather_bf16 and 8 < f <= 64 and f % 2 == 0:       # bf16 gathered operand (the self term stays fp32)
        gsg = cast_bf16(gsg)
        o.g_bf16 = 1
    launch("acm_spmm_ex", f"spmm_sub/{f}", gs.device, low_t.handle, _vp(gsg), gsg.stride(0), f, _vp(d_struc), d_struc.stride(0), C.byref(o),
           _vp(ws), ws.numel() * 4)
    return d_struc


_NONE4 = (None,) * 4
PROJECTED = object()              # in the layer Functions' ``pregathered`` slot: ``x`` is the projection Z of a block input
_NO_GRADS = (None,) * 28          # one per argument of the layer Functions (see acm_conv)


def _grads(d_x, d_w3, d_vec, d_struc, d_mix, d_lnw, d_lnb):
    """The gradient tuple of the layer Functions' argument list; ``d_vec`` / ``d_lnw`` / ``d_lnb`` hold the k channels' (no
    LayerNorm: empty).  The gradients must be view objects of THIS call (_flat_views)."""
    pad = (None,) * (4 - len(d_vec))
    return (d_x, *d_w3, *d_vec, *pad, d_struc, d_mix, *((*d_lnw, *pad) if d_lnw else _NONE4),
            *((*d_lnb, *pad) if d_lnb else _NONE4), *_NO_GRADS[:10])


def _k3_setup(cfg, ops, k, f, n, dev, f_in_w, pre, zi, vecs, lnw, lnb, mix, grad_out, post_relu, post_scale, post_drop,
              fb=None):
    """Buffers and acm_conv_bwd_local_t of the row-local backward of one layer: G tables, dZ, the flat buffer every
    replicated-parameter gradient is a view of."""
    four = k == 4
    fb = f if fb is None else fb
    g, gs = _narrow_tables(n, fb, f, dev, packed=four and f == 2 and fb == 2)      # [G_L | G_H] (channel blocks of fb columns)
    dz = torch.empty(n, 3 * f, dtype=_F32, device=dev)           # [dZ_L | dZ_H | dZ_I]
    if four and gs is None:
        gs = torch.empty(n, f, dtype=_F32, device=dev)
    # every replicated-parameter gradient is a view of one flat buffer: a row-sharded run sums the partials
    # with a single all-reduce and no pack / unpack launches
    nw, nln = 3 * f_in_w * f, (k * f if cfg.layernorm else 0)
    flat = torch.empty(nw + k * f + 2 * nln + k * k, dtype=_F32, device=dev)
    d_vec, d_lnw, d_lnb, d_mix = _flat_views(flat, nw, k, f, cfg.layernorm)

    q = _lib.ConvBwdLocal()
    q.f_out = f
    _set_head(q, cfg, vecs, lnw, lnb, mix)
    q.grad_out, q.ld_grad_out = grad_out.data_ptr(), grad_out.stride(0)
    q.pre, q.ld_pre = pre.data_ptr(), pre.stride(0)
    q.s_mlp, q.ld_s_mlp = zi.data_ptr(), zi.stride(0)
    general = bool(getattr(ops, "general", False))
    ones = ops.zeros(n, 1).new_ones(n) if (four and general) else None
    # pattern-only backward: A_low^T G = P (D^-1 G), so G_L / G_H are written pre-scaled and G_S unscaled
    # (A_low^T (D G_S) = P G_S)
    q.deg = None if (not four or ops.implicit) else (ones if general else ops.deg).data_ptr()
    if ops.implicit:
        q.g_scale = ops.row_scale.data_ptr()
    q.g_low, q.ld_g_low = g.data_ptr(), g.stride(0)
    q.g_high, q.ld_g_high = g.data_ptr() + 4 * fb, g.stride(0)
    q.g_mlp, q.ld_g_mlp = dz.data_ptr() + 8 * f, dz.stride(0)
    if four:
        q.g_struc, q.ld_g_struc = gs.data_ptr(), gs.stride(0)
    q.d_att_vec, q.d_ln_weight, q.d_ln_bias = _ptr_array(d_vec), _ptr_array(d_lnw), _ptr_array(d_lnb)
    q.d_att_mix = d_mix.data_ptr()
    _set_post(q, post_relu, post_scale, post_drop, ops.row_offset)
    return dict(q=q, g=g, dz=dz, gs=gs, flat=flat, nw=nw, d_vec=d_vec, d_lnw=d_lnw, d_lnb=d_lnb, d_mix=d_mix,
                general=general, ones=ones, grad_out=grad_out)


def _conv_prologue(ctx, x, w_low, ops, post_relu, post_scale, post_drop, call, in_drop, projected=False):
    """What the narrow forms (aggregate-first, ACMII, literal) check and record first; returns the input as float32.
    ``projected``: ``x`` is the projection Z of a block input (functional.blocks), not the layer's input: no width check.

    ``call``: the model call's context (deferral list, loss-tail request, input pipeline, projection hand-off);
    ``in_drop = (p, tag, DropoutState)``: the caller's INPUT dropout (models.py:54), left to this layer -- the forms that gather
    X apply it first, the literal one inside the dense projection (acm_gemm_drop) where it can, forward and backward."""
    ctx.set_materialize_grads(False)          # no zero-filled gradient for the (non-differentiable) att output
    ctx.call = _call_or_ambient(call)
    ctx.in_drop = in_drop if (in_drop is not None and in_drop[0] > 0) else None
    sparse_x = isinstance(x, SparseFeatures)
    if not sparse_x:
        x = _as_f32_rows(x, "input") if projected else _as_f32c(x, "input")      # (Z keeps its row pitch)
    n, f = x.shape[0], w_low.shape[1]
    if post_scale is not None:
        post_scale = _as_f32c(post_scale, "post_scale")
        if tuple(post_scale.shape) != (n, f):
            raise ValueError(f"post_scale must be [{n}, {f}]")
    ctx.post_relu, ctx.post_scale = bool(post_relu), post_scale
    ctx.post_drop = post_drop if (post_drop is not None and post_drop[0] > 0) else None
    if n != ops.n_local:
        raise ValueError(f"input has {n} rows but the graph operator has {ops.n_local}")
    ctx.x_width = x.shape[1]
    if not projected and x.shape[1] != w_low.shape[0] and (sparse_x or x.shape[1] < w_low.shape[0]):   # (dropout(..., pad_to=...): zero columns)
        raise ValueError(f"input has {x.shape[1]} columns but the weights have {w_low.shape[0]} rows")
    return x


def _gathered_input(ctx, x, ops, f_in, f, fp, agg_holder, pregathered, agg_first):
    """The input of the two forms that gather X itself (aggregate-first, ACMII recompute): the caller's input dropout applied,
    X zero-padded to ``fp`` columns, P = A_low X when it is at hand already and the gathered rows.  Returns
    (x, xpad, xg, agg_given, agg_holder); sets ctx.pipe.

    ``agg_holder``: layers.GraphConvolution's {"agg": P-or-None} of a pass over a static input; ``pregathered``: every node's
    (dropped) input from the caller (models.GCN, row-sharded); a training step's InputPipeline (call.pipe) hands an
    aggregate-first layer the P that the previous step's backward gathered."""
    n, call = x.shape[0], ctx.call
    if ctx.in_drop is not None:               # these forms gather the input itself: they need the dropped rows
        x = _drop_now(x, _drop_spec(ctx.in_drop, ops.row_offset))
    # (the pipeline's table is refilled in place through raw pointers -- no version bump: never through the holder;
    #  ACMII recomputes per edge from the gathered rows: there is no P to keep)
    if agg_holder is not None and (ops.sharded or call.pipe is not None or not agg_first or ctx.in_drop is not None):
        agg_holder = None
    if x.shape[1] == fp:
        xpad = x
    else:                                     # the zero-padded copy of a static input is kept with its P
        xpad = agg_holder.get("xpad") if agg_holder is not None else None
        if xpad is None or tuple(xpad.shape) != (n, fp):
            xpad = torch.nn.functional.pad(x[:, :f_in], (0, fp - f_in))
            if agg_holder is not None:
                agg_holder["xpad"] = xpad
    agg_given = agg_holder.get("agg") if agg_holder is not None else None
    if agg_given is not None and tuple(agg_given.shape) != (n, fp):
        agg_given = None
    # a training loop's input pipeline (InputPipeline): P for this step came out of the previous step's backward
    pipe = call.pipe
    ctx.pipe = None
    if (pipe is not None and pipe.primed and agg_first and fp == 8 and f == 64 and ops is pipe.ops
            and xpad.data_ptr() == pipe.local_table().data_ptr() and agg_holder is None):   # (only a training step carries a pipe)
        agg_given = pipe.agg()
        ctx.pipe = pipe
        pipe.adopted = True               # the loop may refill the table: this forward leaves its copies in ``saved``
    if agg_given is not None:
        xg = xpad                             # not read: P = A_low X comes from the holder
    elif (pregathered is not None and pregathered[0].data_ptr() == xpad.data_ptr()
            and pregathered[1].shape[1] == fp and pregathered[1].shape[0] == ops.n_gathered):
        xg = pregathered[1]                   # the caller already holds every node's (dropped) input
    else:
        xg = _pkg._gather_rows(ops, xpad)
    return x, xpad, xg, agg_given, agg_holder


def _struc_rows(ops, struc_low, n):
    """The structure channel's parameter rows of this process, and of every node (all-gathered when row-sharded)."""
    if ops.deg is None:
        raise RuntimeError("structure_info=1 needs adj_low_unnormalized")
    s_local = _as_f32c(struc_low, "struc_low")
    if s_local.shape[0] != n:
        raise ValueError("struc_low rows != local nodes")
    return s_local, _pkg._gather_rows(ops, s_local)
