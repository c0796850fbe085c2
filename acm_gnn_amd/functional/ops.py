"""The single-kernel operators: the gemm family, the narrow projections, spmm, the bf16 cast, the masked NLL and BCE, the evaluation
metrics (accuracy / NLL, ROC-AUC) and the counter-based dropout -- raw launches and, where a model differentiates through them, their autograd
Functions."""
import ctypes as C

import torch

from .. import _lib, tuning
from ._context import _ambient, _run
from ._launch import EUNSUPPORTED, _F32, _as_f32_rows, _as_f32c, _check_device, _ref, _vp, _workspace, _workspace_bytes, _workspace_sized, launch


# ---- dense and sparse products ----
def gemm_drop_supported(n_rows, f_in, n_out):
    """Whether BOTH products of a dense projection -- Z = drop(X) W (NN) and dW = drop(X)^T dZ (TN) -- can take the input
    dropout in their tile loads (acm_gemm_drop: the row-panel kernels of acm_gemm_rows.hip)."""
    return (n_rows >= 8192 and 16 <= f_in <= 128 and 1 <= n_out <= 192
            and (tuning.gemm_forms() & (tuning.GEMM_ROWS | tuning.GEMM_ROWS_ALWAYS)) != 0)


def gemm(a, b, trans_a=False, trans_b=False, relu=False, out=None, col_blocks=0, a_drop=None, b_shift=None):
    """out = op(a) @ op(b) on the fp32 MFMA pipe (acm_gemm).  ``col_blocks=j`` returns the product as a
    contiguous [j, m, n / j] tensor of column blocks (acm_gemm_blocks).  ``a_drop``: an acm_dropout_t applied to the stored
    matrix ``a`` while its tiles are staged (acm_gemm_drop; see gemm_drop_supported).  ``b_shift``: one float per column of the
    stored ``b``, subtracted while ITS tiles are staged (acm_gemm_shift: a^T (b - 1 shift^T) only)."""
    a, b = _as_f32_rows(a, "a"), _as_f32_rows(b, "b")          # column slices of wider matrices: (pointer, ld), no copy
    m, k = (a.shape[1], a.shape[0]) if trans_a else (a.shape[0], a.shape[1])
    k2, n = (b.shape[1], b.shape[0]) if trans_b else (b.shape[0], b.shape[1])
    if k != k2:
        raise ValueError(f"gemm: inner dimensions differ ({k} vs {k2})")
    shape = (m, n)
    if col_blocks:
        if n % col_blocks:
            raise ValueError("gemm: col_blocks needs n divisible by the block count")
        nb = n // col_blocks
        shape = (col_blocks, m, nb)
        if out is not None and (tuple(out.shape) != shape or not out.is_contiguous() or out.dtype != _F32):
            raise ValueError("gemm: out must be a contiguous fp32 [col_blocks, m, n / col_blocks] tensor")
    if out is None:
        out = torch.empty(shape, dtype=_F32, device=a.device)
    ld = (nb, nb, m * nb) if col_blocks else (out.stride(0), 0, 0)          # ldc, block width, block stride
    ws, nbytes = _gemm_workspace(a.device, trans_a, trans_b, m, n, k)
    label = f"gemm_{'T' if trans_a else 'N'}{'T' if trans_b else 'N'}/{m}x{n}x{k}"
    head = (int(trans_a), int(trans_b), m, n, k, _vp(a), a.stride(0), _vp(b), b.stride(0), _vp(out))
    if b_shift is not None:
        if a_drop is not None or col_blocks or relu:
            raise ValueError("gemm: b_shift goes with a plain product only")
        b_shift = _as_f32c(b_shift, "b_shift")
        if b_shift.numel() != b.shape[1]:
            raise ValueError(f"gemm: b_shift has {b_shift.numel()} entries for {b.shape[1]} columns")
        launch("acm_gemm_shift", label, a.device, *head[:9], _vp(b_shift), _vp(out), ld[0], _vp(ws), nbytes)
    elif a_drop is not None:
        launch("acm_gemm_drop", label, a.device, *head, *ld, int(relu), C.byref(a_drop), _vp(ws), nbytes)
    elif col_blocks:
        launch("acm_gemm_blocks", label, a.device, *head, *ld, int(relu), _vp(ws), nbytes)
    else:
        launch("acm_gemm", label, a.device, *head, ld[0], int(relu), _vp(ws), nbytes)
    return out


def _gemm_workspace(dev, trans_a, trans_b, m, n, k):
    """(workspace, byte count as the library answered it) of the acm_gemm family; no buffer -- a null pointer -- for zero."""
    nbytes = _workspace_bytes("acm_gemm_workspace_bytes", int(trans_a), int(trans_b), m, n, k)
    return (torch.empty(max(nbytes // 4, 1), dtype=_F32, device=dev) if nbytes else None), nbytes


def gemm_split(a, b, out1, out2, relu=False):
    """[out1 | out2] = a @ b: the first out1.shape[1] columns go to out1, the rest to out2 (acm_gemm_split)."""
    a, b = _as_f32c(a, "a"), _as_f32c(b, "b")
    m, k = a.shape
    n = b.shape[1]
    split = out1.shape[1]
    if b.shape[0] != k or out2.shape[1] != n - split or out1.shape[0] != m or out2.shape[0] != m:
        raise ValueError("gemm_split: shape mismatch")
    ws, nbytes = _gemm_workspace(a.device, 0, 0, m, n, k)
    launch("acm_gemm_split", f"gemm_NN/{m}x{n}x{k}", a.device, 0, 0, m, n, k, _vp(a), a.stride(0), _vp(b), b.stride(0), _vp(out1), out1.stride(0),
           split, _vp(out2), out2.stride(0), int(relu), _vp(ws), nbytes)


def proj3(x, weights, f_block, out, out2=None, relu=False, x_drop=None):
    """[Z_L 0 | Z_H 0 | Z_I] = relu?(drop?(x) @ [W_L 0 | W_H 0 | W_I]) with the three weight matrices read in place
    (acm_proj3: no packed copy of the weights, the input dropout drawn in the operand load): the first two channels in
    blocks of ``f_block`` columns; all 2 f_block + F columns go to ``out``, or the first out.shape[1] to ``out`` and the rest
    to ``out2``.  Returns False -- nothing launched -- outside the kernel's envelope (tall dense x of 32..128 features)."""
    if not isinstance(x, torch.Tensor) or x.dtype != _F32 or x.dim() != 2 or not (tuning.gemm_forms() & tuning.GEMM_BX3):
        return False
    n, k = x.shape
    ws3 = list(weights)
    f = ws3[0].shape[1]
    ncols = 2 * int(f_block) + f
    if (n < 8192 or not 32 <= k <= 128 or k % 4 or x.stride(1) != 1 or x.stride(0) % 4 or x.data_ptr() % 16 or ncols > 192
            or any(w.dtype != _F32 or tuple(w.shape) != (k, f) or w.stride(1) != 1 or w.stride(0) != ws3[0].stride(0)
                   or w.device != x.device for w in ws3)):
        return False
    split = 0 if out2 is None else out.shape[1]
    if out.shape[0] != n or (out2 is None and out.shape[1] != ncols) or (out2 is not None and tuple(out2.shape) != (n, ncols - split)):
        raise ValueError("proj3: shape mismatch")
    st = launch("acm_proj3", f"proj3/{n}x{ncols}x{k}", x.device, n, k, _vp(x), x.stride(0), _vp(ws3[0]), _vp(ws3[1]), _vp(ws3[2]),
                ws3[0].stride(0), f, int(f_block), _vp(out), out.stride(0), split, _vp(out2), out2.stride(0) if out2 is not None else 0,
                int(relu), _ref(x_drop), unsupported_ok=True)
    return st != EUNSUPPORTED                     # (unsupported after all: nothing launched)


def proj_fwd(x, weights, out_lh, out_i, relu=False, h_col=None):
    """[out_lh | out_i] = relu?(x @ [W_L | W_H | W_I]) for a narrow layer (F <= 8), straight from the three weight
    matrices (acm_proj_fwd): out_lh [n, 2F] is the gathered block, out_i [n, F].  ``h_col`` (acm_proj_fwd_at): Z_H starts
    at that column of out_lh ([n, h_col + F] at least) instead of column F -- channel blocks of 4 / 8 columns."""
    x = _as_f32c(x, "x")
    ws3 = [_as_f32c(w, "weight") for w in weights]
    n, f_in = x.shape
    f = ws3[0].shape[1]
    h_col = f if h_col is None else int(h_col)
    if (any(tuple(w.shape) != (f_in, f) for w in ws3) or out_lh.shape[0] != n or out_lh.shape[1] < h_col + f or h_col < f
            or out_i.shape != (n, f)):
        raise ValueError("proj_fwd: shape mismatch")
    launch("acm_proj_fwd_at", f"proj_fwd/{n}x{f_in}x{3 * f}", x.device, n, f_in, f, _vp(x), x.stride(0), _vp(ws3[0]), _vp(ws3[1]), _vp(ws3[2]),
           ws3[0].stride(0), int(relu), _vp(out_lh), out_lh.stride(0), h_col, _vp(out_i), out_i.stride(0))


def proj_bwd(x, dz, weights, d_w_out, defer=None, dx_out=None):
    """Backward of the skinny projection Z = x @ [W_L | W_H | W_I] in one pass over x (acm_proj_bwd): returns
    dX = dz @ Wcat.T and fills ``d_w_out`` ([3, f_in, F], contiguous) with x.T @ dz.  ``weights``: the three
    [f_in, F] matrices.  ``defer``: a DeferredReductions the second phase is appended to (default: the thread's)."""
    if defer is None:
        defer = _ambient().defer
    x, dz = _as_f32c(x, "x"), _as_f32c(dz, "dz")
    ws3 = [_as_f32c(w, "weight") for w in weights]
    n, f_in = x.shape
    q = 3 * ws3[0].shape[1]
    blocks = d_w_out.shape[0]
    nb = q // blocks
    if (tuple(d_w_out.shape) != (blocks, f_in, nb) or not d_w_out.is_contiguous() or dz.shape != (n, q)
            or any(tuple(w.shape) != (f_in, q // 3) or w.stride(0) != ws3[0].stride(0) for w in ws3)):
        raise ValueError("proj_bwd: shape mismatch")
    dx = torch.empty(n, f_in, dtype=_F32, device=x.device) if dx_out is None else dx_out[:, :f_in]
    ws, nbytes = _workspace_sized(x.device, "acm_proj_bwd_workspace_bytes", n, f_in, q)
    launch("acm_proj_bwd", f"proj_bwd/{n}x{f_in}x{q}", x.device, n, f_in, q, _vp(x), x.stride(0), _vp(dz), dz.stride(0), _vp(ws3[0]), _vp(ws3[1]),
           _vp(ws3[2]), ws3[0].stride(0), _vp(dx), dx.stride(0), _vp(d_w_out), nb, nb, f_in * nb, _vp(ws), nbytes,
           defer.pointer() if defer is not None else None)
    if defer is not None:
        defer.hold(ws, [d_w_out])
    return dx


def proj_bwd_supported(q):
    return q in (3, 6, 9, 12, 15)


def spmm(graph, dense, out=None, row_scale=None, bf16=False):
    """out = A @ dense for a CsrGraph A (acm_spmm); with ``row_scale``: diag(row_scale) (A @ dense) (acm_spmm_ex).
    ``bf16``: gather a bf16 copy of ``dense`` (even 8 < width <= 64; fp32 sums)."""
    dense = _as_f32_rows(dense, "dense")
    if dense.shape[0] != graph.n_cols:
        raise ValueError(f"spmm: dense has {dense.shape[0]} rows, operator has {graph.n_cols} columns")
    width = dense.shape[1]
    if out is None:
        out = torch.empty(graph.n_rows, width, dtype=_F32, device=dense.device)
    if width == 0 or graph.n_rows == 0:
        return out
    ws = graph.workspace(min(width, 256))
    bf16 = bool(bf16) and 8 < width <= 64 and width % 2 == 0
    if bf16:
        dense = cast_bf16(dense)
    label, io = f"spmm/W{width}{'b' if bf16 else ''}", (graph.handle, _vp(dense), dense.stride(0), width, _vp(out), out.stride(0))
    if row_scale is None and not bf16:
        launch("acm_spmm", label, dense.device, *io, _vp(ws), ws.numel() * 4)
    else:
        o = _lib.SpmmOpts()
        o.g_bf16 = int(bf16)
        o.row_scale = _as_f32c(row_scale, "row_scale").data_ptr() if row_scale is not None else None
        launch("acm_spmm_ex", label, dense.device, *io, C.byref(o), _vp(ws), ws.numel() * 4)
    return out


def spmm_v(graph, vals, dense, relu=False, out=None):
    """out = A(vals) @ dense: the operator's structure with per-call values (acm_spmm_v)."""
    dense = _as_f32c(dense, "dense")
    vals = _as_f32c(vals, "vals")
    if dense.shape[0] != graph.n_cols or vals.numel() != graph.nnz:
        raise ValueError("spmm_v: shape mismatch")
    width = dense.shape[1]
    if out is None:
        out = torch.empty(graph.n_rows, width, dtype=_F32, device=dense.device)
    if width == 0 or graph.n_rows == 0:
        return out
    ws = graph.workspace(min(width, 256))
    launch("acm_spmm_v", f"spmm_v/{graph.n_rows}x{graph.n_cols}W{width}", dense.device, graph.handle, _vp(vals), _vp(dense), dense.stride(0),
           width, _vp(out), out.stride(0), int(relu), _vp(ws), ws.numel() * 4)
    return out


def cast_bf16(src):
    """fp32 [n, c] (any row pitch) -> new contiguous bf16 [n, c] (acm_cast_bf16, round to nearest even)."""
    _check_device(src, "src")
    n, c = src.shape
    dst = torch.empty(n, c, dtype=torch.bfloat16, device=src.device)
    if n == 0 or c == 0:                          # (an empty tensor has no address to hand to the library)
        return dst
    launch("acm_cast_bf16", f"cast_bf16/{n}x{c}", src.device, n, c, _vp(src), src.stride(0), _vp(dst), dst.stride(0))
    return dst


class _Mm(torch.autograd.Function):
    """Differentiable dense product on acm_gemm (used by the trivial layer branches)."""

    @staticmethod
    def forward(ctx, a, b):
        ctx.save_for_backward(a, b)
        return gemm(a, b)

    @staticmethod
    def backward(ctx, g):
        a, b = ctx.saved_tensors
        g = g.contiguous()
        ga = gemm(g, b, trans_b=True) if ctx.needs_input_grad[0] else None
        gb = gemm(a, g, trans_a=True) if ctx.needs_input_grad[1] else None
        return ga, gb


def mm(a, b):
    return _run(_Mm, a, b)


# ---- the masked NLL and the evaluation metrics ----
class _MaskedNll(torch.autograd.Function):
    """loss = sum_i w_i * (logsumexp(z_i) - z_i[y_i]) with its gradient from the same pass
    (acm_nll_loss)."""

    @staticmethod
    def forward(ctx, logits, labels, row_weight, defer=None):
        z = _as_f32c(logits, "logits")
        w = _as_f32c(row_weight, "row_weight")
        _check_device(labels, "labels")
        y = labels.to(torch.int64).contiguous().reshape(-1)
        n, c = z.shape
        if y.numel() != n or w.numel() != n:
            raise ValueError("masked_nll: labels / row_weight must have one entry per row")
        loss = torch.empty((), dtype=_F32, device=z.device)
        dz = torch.empty_like(z)
        ws = _workspace(z.device, "acm_nll_loss_workspace_bytes", n)
        launch("acm_nll_loss", f"nll_loss/{n}x{c}", z.device, n, c, _vp(z), z.stride(0), _vp(y), _vp(w), _vp(loss), _vp(dz), dz.stride(0),
               _vp(ws), ws.numel() * 4, defer.pointer() if defer is not None else None)
        if defer is not None:
            defer.hold(ws, [loss])
        ctx.save_for_backward(dz)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        (dz,) = ctx.saved_tensors
        return dz * grad_loss, None, None, None


def nll_loss_and_grad(logits, labels, row_weight, defer=None):
    """(loss, dloss/dlogits) of the masked NLL in one launch, outside autograd: a training loop can call
    ``logits.backward(gradient=dz)`` directly instead of ``loss.backward()`` (which costs a ones-fill and a
    scalar multiply of dz on top).  ``defer``: see proj_bwd."""
    if defer is None:
        defer = _ambient().defer
    with torch.no_grad():
        ctx = _NoCtx()
        loss = _MaskedNll.forward(ctx, logits.detach(), labels, row_weight, defer)
    return loss, ctx.saved[0]


class _NoCtx:
    def save_for_backward(self, *t):
        self.saved = t


def masked_nll(logits, labels, row_weight):
    """Fused log-softmax + NLL over the rows with non-zero weight (weights = 1/|train| on the
    training rows reproduces F.log_softmax + NLLLoss(out[train_idx], y[train_idx]),
    ACM-Geometric/train.py:133-134)."""
    return _run(_MaskedNll, logits, labels, row_weight, _ambient().defer)


def eval_metrics_buffers(n_rows, n_sets, device):
    """(result [n_sets + 1], workspace) for :func:`eval_metrics`; the workspace is zeroed ONCE (its arrival counter resets
    itself after every launch)."""
    nbytes = _workspace_bytes("acm_eval_metrics_workspace_bytes", int(n_rows), int(n_sets))
    return (torch.empty(n_sets + 1, dtype=_F32, device=device),
            torch.zeros(max(nbytes // 4, 1), dtype=_F32, device=device))


def eval_metrics(logits, labels, weights, loss_set, buffers=None):
    """Accuracy on every index set and the NLL on set ``loss_set`` from eval-mode logits, as one launch (acm_eval_metrics:
    the evaluation of ACM-Geometric/train.py:138-140 + data_utils.py:153-168 and ACM-Pytorch/train.py:112-139).
    ``weights`` [k, n]: 1 / |set| on the set's rows, 0 elsewhere (rows of weight 0 may carry the label -1).  Returns the
    fp32 tensor [acc_0 .. acc_{k-1}, nll]."""
    _check_device(logits, "logits")
    n, c = logits.shape
    k = weights.shape[0]
    if weights.shape[1] != n or weights.dtype != _F32 or weights.stride(1) != 1 or labels.shape[0] != n:
        raise ValueError("eval_metrics: weights must be fp32 [k, n] with contiguous rows, labels [n]")
    res, ws = buffers if buffers is not None else eval_metrics_buffers(n, k, logits.device)
    launch("acm_eval_metrics", f"eval_metrics/{n}x{c}k{k}", logits.device, n, c, _vp(logits), logits.stride(0), _vp(labels), _vp(weights),
           weights.stride(0), k, int(loss_set), _vp(res), _vp(ws), ws.numel() * 4)
    return res


# ---- the second protocol: masked BCE-with-logits on one-hot labels, ROC-AUC (ACM-Geometric/train.py:86-92, 123-131) ----
def _check_rows(who, logits, labels, n_classes_min=1):
    """The public entry points below take their operands as they are -- fp32 logits [n, C] with unit column stride, int64
    labels [n], contiguous, on the logits' device -- and say so instead of converting or reading something else."""
    _check_device(logits, "logits")
    _check_device(labels, "labels")
    if logits.dim() != 2 or logits.dtype != _F32 or logits.shape[1] < n_classes_min or logits.stride(1) != 1 \
            or (logits.shape[0] > 1 and logits.stride(0) < logits.shape[1]):
        raise ValueError(f"{who}: logits must be fp32 [n, C >= {n_classes_min}] with stride(1) == 1")
    if logits.shape[1] > 64:
        raise ValueError(f"{who}: {logits.shape[1]} classes > 64")
    if labels.dtype != torch.int64 or labels.dim() != 1 or labels.shape[0] != logits.shape[0] or not labels.is_contiguous():
        raise ValueError(f"{who}: labels must be a contiguous int64 [n] tensor")
    if labels.device != logits.device:
        raise ValueError(f"{who}: labels are on {labels.device}, logits on {logits.device}")


def _check_weights(who, weights, shape, dev):
    _check_device(weights, "weights")
    if weights.dtype != _F32 or tuple(weights.shape) != tuple(shape) or weights.stride(-1) != 1 or weights.device != dev \
            or (weights.dim() == 2 and weights.shape[0] > 1 and weights.stride(0) < weights.shape[1]):
        raise ValueError(f"{who}: weights must be fp32 {list(shape)} with contiguous rows on {dev}")


def _bce_launch(z, y, w, defer, dz):
    """acm_bce_loss on checked operands; ``dz`` None = loss only.  Returns the loss scalar."""
    n, c = z.shape
    loss = torch.empty((), dtype=_F32, device=z.device)
    ws = _workspace(z.device, "acm_bce_loss_workspace_bytes", n)
    launch("acm_bce_loss", f"bce_loss/{n}x{c}", z.device, n, c, _vp(z), z.stride(0), _vp(y), _vp(w), _vp(loss), _vp(dz),
           dz.stride(0) if dz is not None else 0, _vp(ws), ws.numel() * 4, defer.pointer() if defer is not None else None)
    if defer is not None:
        defer.hold(ws, [loss])
    return loss


class _MaskedBce(torch.autograd.Function):
    """loss = sum_i w_i / C * sum_c bce(z_ic, [c == y_i]) with its gradient from the same pass (acm_bce_loss)."""

    @staticmethod
    def forward(ctx, logits, labels, row_weight, defer=None, out=None):
        _check_rows("masked_bce", logits, labels)
        _check_weights("masked_bce", row_weight, (logits.shape[0],), logits.device)
        if out is None:
            dz = torch.empty(logits.shape, dtype=_F32, device=logits.device)
        else:
            dz = out
            if dz.dtype != _F32 or dz.shape != logits.shape or dz.stride(1) != 1 or dz.device != logits.device \
                    or (dz.shape[0] > 1 and dz.stride(0) < dz.shape[1]):
                raise ValueError("masked_bce: out must be fp32 with the logits' shape, stride(1) == 1, on their device")
        loss = _bce_launch(logits, labels, row_weight, defer, dz)
        ctx.save_for_backward(dz)
        return loss

    @staticmethod
    def backward(ctx, grad_loss):
        (dz,) = ctx.saved_tensors
        return dz * grad_loss, None, None, None, None


def masked_bce(logits, labels, row_weight):
    """nn.BCEWithLogitsLoss() against the one-hot of ``labels`` over the rows with non-zero weight (weights = 1/|train| on
    the training rows -- train.row_weights -- reproduce ``criterion(out[train_idx], F.one_hot(label)[train_idx].float())``,
    ACM-Geometric/train.py:86-92, 123-131).  Rows of weight 0 may carry the label -1."""
    return _run(_MaskedBce, logits, labels, row_weight, _ambient().defer, None)


def bce_loss_and_grad(logits, labels, row_weight, defer=None, out=None):
    """(loss, dloss/dlogits) of the masked BCE in one launch, outside autograd (see nll_loss_and_grad).  ``out``: an fp32
    buffer for the gradient (any row pitch).  ``defer``: see proj_bwd."""
    if defer is None:
        defer = _ambient().defer
    with torch.no_grad():
        ctx = _NoCtx()
        loss = _MaskedBce.forward(ctx, logits.detach(), labels, row_weight, defer, out)
    return loss, ctx.saved[0]


def bce_loss(logits, labels, row_weight):
    """The masked BCE alone (acm_bce_loss with a NULL gradient): the validation loss of an evaluation pass."""
    _check_rows("bce_loss", logits, labels)
    _check_weights("bce_loss", row_weight, (logits.shape[0],), logits.device)
    return _bce_launch(logits.detach(), labels, row_weight, None, None)


def rocauc_buffers(n_rows, n_sets, device):
    """(scores fp32 [n], counts int64 [k, 3], auc float64 [k], workspace) for :func:`eval_rocauc`: made once by a caller whose
    pass is captured (the addresses are baked in).  Nothing needs initialising."""
    nbytes = _workspace_bytes("acm_rocauc_workspace_bytes", int(n_rows), int(n_sets))
    return (torch.empty(int(n_rows), dtype=_F32, device=device), torch.empty(int(n_sets), 3, dtype=torch.int64, device=device),
            torch.empty(int(n_sets), dtype=torch.float64, device=device),
            torch.empty(nbytes // 8 + 1, dtype=torch.int64, device=device))


def eval_rocauc(logits, labels, weights, buffers=None, return_counts=False):
    """ROC-AUC of softmax(logits)[:, 1] against ``labels`` on every index set, on the device (data_utils.eval_rocauc for
    single-column labels, ACM-Geometric/data_utils.py:128-151, without its three copies to the host): acm_rocauc_scores, ONE
    ``torch.sort`` of the n scores for all sets, acm_rocauc.  ``weights`` [k, n]: non-zero on a set's rows (k <= 8); of those
    the rows labelled 0 / 1 are the set's negatives / positives, any other label is skipped.  Returns the float64 device
    tensor [k] of AUCs -- NaN where a set lacks a class -- and with ``return_counts`` also the exact int64 [k, 3] triples
    (U2, npos, nneg), AUC = U2 / (2 npos nneg).  Both are views of ``buffers`` when given."""
    _check_rows("eval_rocauc", logits, labels, n_classes_min=2)
    n, c = logits.shape
    if weights.dim() != 2 or not 1 <= weights.shape[0] <= 8:
        raise ValueError("eval_rocauc: weights must be [k, n] with 1 <= k <= 8 index sets")
    k = weights.shape[0]
    _check_weights("eval_rocauc", weights, (k, n), logits.device)
    scores, counts, auc, ws = buffers if buffers is not None else rocauc_buffers(n, k, logits.device)
    if scores.shape[0] != n or counts.shape[0] != k:
        raise ValueError("eval_rocauc: buffers were made for another shape (rocauc_buffers(n_rows, n_sets, device))")
    launch("acm_rocauc_scores", f"rocauc_scores/{n}x{c}", logits.device, n, c, _vp(logits), logits.stride(0), _vp(scores))
    ranked, order = torch.sort(scores)                  # the one device primitive of the pass that is not this library's
    launch("acm_rocauc", f"rocauc/{n}k{k}", logits.device, n, _vp(ranked), _vp(order), _vp(labels), _vp(weights), weights.stride(0), k,
           _vp(counts), _vp(auc), _vp(ws), ws.numel() * 8)
    return (auc, counts) if return_counts else auc


# ---- counter-based dropout (acm_dropout_t) ----
class DropoutState:
    """Seed + device step counter of the counter-based dropout.  The mask of element (row, col) is a pure
    function of (seed, step, tag, row, col), so forward and backward kernels regenerate it instead of storing
    it.  ``advance()`` (or FusedAdam's ``also_advance`` hook) must run once per optimizer step; every forward /
    backward between two advances sees the same masks (distinguished by ``tag``)."""

    def __init__(self, device, seed=None):
        self.seed = int(torch.initial_seed() if seed is None else seed) & 0xFFFFFFFFFFFFFFFF
        self.step = torch.zeros(1, dtype=torch.int64, device=device)
        self.host_steps = 0          # host-side count of advances (whoever advances `step` on the device bumps it too):
                                     # lets a consumer that works ahead (InputPipeline) notice that someone else stepped

    def advance(self):
        self.step.add_(1)
        self.host_steps += 1

    def spec(self, p, tag, row_offset=0):
        d = _lib.Dropout()
        d.p, d.tag, d.seed, d.step, d.row_offset = float(p), int(tag), self.seed, self.step.data_ptr(), int(row_offset)
        return d


def _drop_spec(post_drop, row_offset):
    if post_drop is None:
        return None
    p, tag, state = post_drop
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout probability must be in [0, 1)")
    return state.spec(p, tag, row_offset) if p > 0 else None


class _FusedDropout(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, p, tag, state, pad_to, row_offset):
        x = _as_f32c(x, "input")
        n, c = x.shape
        width = max(c, int(pad_to or 0))
        buf = torch.empty(n, width, dtype=_F32, device=x.device)
        d = state.spec(p, tag, row_offset)
        launch("acm_dropout", f"dropout/{n}x{c}", x.device, n, c, _vp(x), x.stride(0), _vp(buf), buf.stride(0), width, C.byref(d))
        ctx.args = (p, tag, state, row_offset, c)
        return buf

    @staticmethod
    def backward(ctx, g):
        p, tag, state, row_offset, c = ctx.args
        g = _as_f32c(g, "grad")                   # [n, width]; the pad columns carry no gradient
        out = torch.empty(g.shape[0], c, dtype=_F32, device=g.device)
        d = state.spec(p, tag, row_offset)
        launch("acm_dropout", None, g.device, g.shape[0], c, _vp(g), g.stride(0), _vp(out), out.stride(0), c, C.byref(d))
        return out, None, None, None, None, None


def _drop_now(x, spec):
    """x * keep / (1 - p) for an acm_dropout_t ``spec`` (non-differentiable launch; same mask as the fused forms)."""
    n, c = x.shape
    buf = torch.empty(n, c, dtype=_F32, device=x.device)
    launch("acm_dropout", f"dropout/{n}x{c}", x.device, n, c, _vp(x), x.stride(0), _vp(buf), buf.stride(0), c, C.byref(spec))
    return buf


def dropout(x, p, state, tag=0, pad_to=None, row_offset=0):
    """x * keep / (1 - p) with the counter-based mask (acm_dropout).  ``pad_to`` > x.shape[1] returns an
    [n, pad_to] tensor whose extra columns are zero -- the row layout the aggregate-first gather wants (pass
    it to the layer with ``input_zero_padded=True``), saving the pad fill + copy."""
    if p <= 0 and not (pad_to and pad_to > x.shape[1]):
        return x
    return _run(_FusedDropout, x, float(p), int(tag), state, pad_to, int(row_offset))


def agg_pad_width(f_in):
    """Row length (floats) of the gathered operand of the aggregate-first path, or f_in when it does not apply."""
    return 4 if f_in <= 4 else (8 if f_in <= 8 else (16 if f_in <= 16 else f_in))
