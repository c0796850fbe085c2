"""The synthetic study's model family (synthetic-experiments/baseline_models/{layers,models}.py) on CSR operators:
``mlp``, ``gcn``, ``sgc`` -- the baselines the study draws ACM-GCN and ACM-SGC against -- and, through the same constructor,
``acmgcn`` / ``acmsgc``.

    from acm_gnn_amd import baselines, synthetic as S, train as T
    g = S.generate_graph("regular", 5, 400, degree_intra=2, edge_homo=0.3)
    model = baselines.GCN(nfeat, 32, 5, dropout=0.5, model_type="gcn")
    T.fit(model, opt, x, g.operators(), g.labels, *S.disassortative_splits(g.labels, 5, seed=0), epochs=..., rule="min_val_loss")

The reference's layer multiplies a DENSE ``adj_low`` with ``torch.mm`` (layers.py:123); here ``adj_low`` is a FilterOperators
(implicit or explicit-valued, possibly relabelled) or the reference's torch sparse tensor (``operators_for``).  What differs from
the two-layer ``models.GCN``, as in the study's code: no input dropout for the three baselines, no ``nnodes`` / structure
channel / LayerNorm, ``sgc`` is ONE layer nfeat -> nclass (``ops.hops = k`` makes it A_low^k X W).

Execution forms: the baselines have no input dropout, so for a dense ``x`` that takes no gradient
P = A_low^k x is constant over a training run -- computed once, kept under the rule of ``layers.GraphConvolution._eval_agg_holder``
(same tensor object and version, same operators) and the first graph layer becomes a dense product on P (acm_gemm_act: ReLU and the
counter-based dropout in its epilogue), with no gather in its backward either.  CSR features, or an ``x`` that needs a gradient,
project first and gather afterwards (acm_gcn_fwd).

``acmgcn`` / ``acmsgc`` build the package's ``models.GCN`` (``attn_layernorm=False``, ``structure_info=0``: the study's ACM layer is
the ACM-Pytorch dialect) and need the ``nnodes`` keyword the study's constructor does not take -- the factory ``GCN(...)`` then
returns that model, so its parameter names and initial draws are the package's (a reference ``state_dict`` loads by name: the names it
shares are the layer's weights and attention vectors)."""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F
from torch.nn.parameter import Parameter

from . import functional as AF
from .graph import FilterOperators, SparseFeatures, operators_for
from .layers import _default_device

BASELINES = ("mlp", "gcn", "sgc")
ACM = ("acmgcn", "acmsgc")


class GraphConvolution(nn.Module):
    """One layer of ``mlp`` / ``gcn`` / ``sgc`` with the parameter set of baseline_models/layers.py:15-70 (names, shapes and the
    draw order of ``reset_parameters``, layers.py:82-95).  ``low_param`` / ``high_param`` / ``mlp_param``, which the reference never
    initialises, are zero-filled (the ``fea_param`` convention of models.GCN).  Only ``weight_mlp`` (mlp) or ``weight_low`` (gcn,
    sgc) takes part in a forward; the other parameters receive no gradient."""

    def __init__(self, in_features, out_features, model_type, output_layer=0):
        super().__init__()
        if model_type not in BASELINES:
            raise ValueError(f"baselines.GraphConvolution: model_type {model_type!r} ({' | '.join(BASELINES)})")
        self.in_features, self.out_features = in_features, out_features
        self.output_layer, self.model_type = output_layer, model_type
        self.att_low, self.att_high, self.att_mlp = 0, 0, 0
        self.eval_agg_cache = True                     # see layers.GraphConvolution
        dev = _default_device()

        def new(*shape):
            return Parameter(torch.empty(*shape, dtype=torch.float32, device=dev))

        self.weight_low, self.weight_high, self.weight_mlp = (new(in_features, out_features) for _ in range(3))
        self.att_vec_low, self.att_vec_high, self.att_vec_mlp = (new(out_features, 1) for _ in range(3))
        self.low_param, self.high_param, self.mlp_param = (Parameter(torch.zeros(1, 1, device=dev)) for _ in range(3))
        self.attention_param = new(3 * out_features, 3)
        self.att_vec = new(3, 3)
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.weight_mlp.size(1))
        std_att = 1.0 / math.sqrt(self.att_vec_mlp.size(1))
        std_att_vec = 1.0 / math.sqrt(self.att_vec.size(1))
        for p in (self.weight_low, self.weight_high, self.weight_mlp):
            p.data.uniform_(-stdv, stdv)
        for p in (self.att_vec_high, self.att_vec_low, self.att_vec_mlp):
            p.data.uniform_(-std_att, std_att)
        self.att_vec.data.uniform_(-std_att_vec, std_att_vec)
        self.attention_param.data.uniform_(-std_att_vec, std_att_vec)

    @property
    def weight(self):
        """The one weight matrix this layer's forward reads."""
        return self.weight_mlp if self.model_type == "mlp" else self.weight_low

    def aggregated(self, x, ops, hops, permute=False):
        """P = A_low^hops x of a dense input that takes no gradient, computed once per (tensor object, version, operators,
        hops) and role -- the rule and the entry layout of layers.GraphConvolution._eval_agg_holder, so that train.TrainStep /
        EvalStep hold what a captured pass read -- or None where the input does not qualify.  ``permute``: x is in the caller's
        numbering and the operators are relabelled (P is formed, and returned, in theirs)."""
        if (not isinstance(x, torch.Tensor) or x.layout != torch.strided or x.dim() != 2 or x.requires_grad or x.grad_fn is not None
                or not self.eval_agg_cache):
            return None
        key = (x.data_ptr(), x._version, tuple(x.shape), tuple(x.stride()), int(hops), bool(permute))
        role = "train" if (self.training and torch.is_grad_enabled()) else "eval"
        slots = self.__dict__.setdefault("_eval_agg", {})
        cached = slots.get(role)
        if cached is None or cached[0] != key or cached[3] is not ops:
            other = slots.get("eval" if role == "train" else "train")
            if other is not None and other[0] == key and other[3] is ops and other[1] is x:
                cached = other                         # the same operand in the other role: one P serves both
            else:
                with torch.no_grad():
                    xin = x.index_select(0, ops.perm) if permute else x
                    p = AF.aggregate(xin, ops, hops)
                cached = (key, x, {"agg": p}, ops)
            slots[role] = cached
        return cached[2]["agg"]

    def held_entries(self):
        return list(self.__dict__.get("_eval_agg", {}).values())

    def forward(self, input, adj_low=None, adj_high=None):
        """The reference's layer call (layers.py:118-124) on rows in the operator's own numbering: ``input @ weight_mlp`` for
        mlp, ``A_low^hops (input @ weight_low)`` otherwise."""
        if self.model_type == "mlp":
            return AF.sparse_mm(input, self.weight_mlp) if isinstance(input, SparseFeatures) else AF.mm(input, self.weight_mlp)
        ops = _operators(adj_low)
        z = AF.sparse_mm(input, self.weight_low) if isinstance(input, SparseFeatures) else AF.mm(input, self.weight_low)
        return AF.aggregate(z, ops, ops.hops if self.model_type == "sgc" else 1)

    def __repr__(self):
        return f"{self.__class__.__name__} ({self.in_features} -> {self.out_features})"


def _operators(adj_low):
    if adj_low is None:
        raise ValueError("baselines: adj_low is required for the graph layers")
    ops = adj_low if isinstance(adj_low, FilterOperators) else operators_for(adj_low)
    if ops.sharded:
        raise NotImplementedError("baselines: row-sharded operators are not supported (the one-channel layers gather every node's "
                                  "row and have no halo exchange)")
    return ops


def GCN(nfeat, nhid, nclass, dropout, model_type, nnodes=None):
    """The study's constructor (baseline_models/models.py:6-23) plus ``nnodes``: a :class:`BaselineGCN` for mlp / gcn / sgc, the
    package's ``models.GCN`` (``attn_layernorm=False``, ``structure_info=0``) for acmgcn / acmsgc, which need ``nnodes``."""
    if model_type in ACM:
        if nnodes is None:
            raise ValueError(f"baselines.GCN: model_type {model_type!r} needs nnodes= (the package's ACM layer registers "
                             "the per-node structure parameter the study's constructor leaves out)")
        from .models import GCN as AcmGCN
        return AcmGCN(nfeat, nhid, nclass, 2, nnodes, dropout, model_type, 0, variant=False, attn_layernorm=False)
    if model_type not in BASELINES:
        raise ValueError(f"baselines.GCN: unsupported model_type {model_type!r} ({' | '.join(BASELINES + ACM)})")
    return BaselineGCN(nfeat, nhid, nclass, dropout, model_type, nnodes)


class BaselineGCN(nn.Module):
    """baseline_models/models.py:6-39 for the three baselines.

    mlp   relu -> dropout between two ``x @ weight_mlp`` products
    gcn   A_low (dropout(relu(A_low (x W1))) W2)
    sgc   the single layer A_low^k (x W), k = ``ops.hops``

    ``fused_dropout`` / ``dropout_state`` as in models.GCN: off by default (F.dropout between the layers); a loop that advances the
    counter once per optimizer step (train.TrainStep) switches it on and the hidden mask (tag 1) is drawn inside the kernels.
    ``fused``: True = the fused graph kernels where they measured faster (functional.gcn.FUSE_MAX_ITEMS), the composed arm
    beyond; False = every graph product composed from the entry points that predate acm_gcn_*; "always" = fused at any size."""
    structure_info = 0

    def __init__(self, nfeat, nhid, nclass, dropout, model_type, nnodes=None):
        super().__init__()
        if model_type not in BASELINES:
            raise ValueError(f"baselines.BaselineGCN: model_type {model_type!r} ({' | '.join(BASELINES)})")
        self.model_type, self.dropout, self.nnodes = model_type, dropout, nnodes
        self.gcns = nn.ModuleList()
        if model_type == "sgc":
            self.gcns.append(GraphConvolution(nfeat, nclass, model_type=model_type))
        else:
            if nhid > AF.gcn.MASK_MAX:
                raise NotImplementedError(f"baselines.GCN: nhid = {nhid} (the hidden layer's backward masks at most {AF.gcn.MASK_MAX} columns)")
            self.gcns.append(GraphConvolution(nfeat, nhid, model_type=model_type))
            self.gcns.append(GraphConvolution(nhid, nclass, model_type=model_type, output_layer=1))
        self.fused_dropout = False
        self.dropout_state = None
        self.fused = True

    def forward(self, x, adj_low, adj_high=None, adj_low_unnormalized=None, call=None, rows_permuted=False):
        """Reference signature plus ``call`` / ``rows_permuted`` as models.GCN.forward: with relabelled operators the rows are
        translated once here unless the caller (train.TrainStep) already works in the operator's numbering."""
        call = AF.CallContext.from_ambient() if call is None else call
        if isinstance(x, torch.Tensor) and x.layout != torch.strided:
            x = SparseFeatures.from_torch(x)
        if self.model_type == "mlp":
            return self._forward(x, None, call, None)            # row-local: any numbering
        ops = _operators(adj_low)
        translate = ops.perm is not None and not rows_permuted
        raw = x if translate else None                       # (the cached P is keyed by the tensor the caller handed over)
        if translate:
            x = x.permute_rows(ops.perm) if isinstance(x, SparseFeatures) else x.index_select(0, ops.perm)
        out = self._forward(x, ops, call, raw)
        return out.index_select(0, ops.inv_perm) if translate else out

    def _cached(self, x, raw, ops, hops):
        """P = A_low^hops x in the operator's numbering, from the first layer's holder, or None.  ``raw``: the tensor the caller
        handed over when it was translated here (the holder's key; P is formed from its permuted rows)."""
        if raw is not None:
            return self.gcns[0].aggregated(raw, ops, hops, permute=True)
        return self.gcns[0].aggregated(x, ops, hops)

    def _forward(self, x, ops, call, raw):
        mt, p = self.model_type, self.dropout
        training = self.training and p > 0
        fused_drop = training and self.fused_dropout
        if fused_drop and self.dropout_state is None:
            self.dropout_state = AF.DropoutState(x.values.device if isinstance(x, SparseFeatures) else x.device)
        off = ops.row_offset if ops is not None else 0
        drop = (p, 1, self.dropout_state, off) if fused_drop else None       # tag 1: the hidden site, as in models.GCN
        l0 = self.gcns[0]
        if mt == "sgc":
            pagg = self._cached(x, raw, ops, ops.hops)
            if pagg is not None:
                return AF.mm(pagg, l0.weight_low)
            z = AF.sparse_mm(x, l0.weight_low) if isinstance(x, SparseFeatures) else AF.mm(x, l0.weight_low)
            return AF.aggregate(z, ops, ops.hops, self.fused)
        l1 = self.gcns[1]
        if mt == "mlp":
            h = AF.dense_act(x, l0.weight_mlp, relu=True, drop=drop)
            if training and not fused_drop:
                h = F.dropout(h, p, training=True)
            return AF.mm(h, l1.weight_mlp)
        pagg = self._cached(x, raw, ops, 1)
        if not training or fused_drop:
            if pagg is not None:
                return AF.gcn_two_layer(pagg, l0.weight_low, l1.weight_low, ops, cached=True, drop=drop, fused=self.fused, call=call)
            return AF.gcn_two_layer(x, l0.weight_low, l1.weight_low, ops, cached=False, drop=drop, fused=self.fused, call=call)
        # F.dropout between the layers (a mask torch draws): layer by layer
        if pagg is not None:
            h = AF.dense_act(pagg, l0.weight_low, relu=True)
        else:
            z = AF.sparse_mm(x, l0.weight_low) if isinstance(x, SparseFeatures) else AF.mm(x, l0.weight_low)
            h = F.relu(AF.aggregate(z, ops, 1, self.fused))
        h = F.dropout(h, p, training=True)
        return AF.aggregate(AF.mm(h, l1.weight_low), ops, 1, self.fused)
