"""The training step / evaluation pass of the two-layer ACM model on a SMALL graph as six (three) launches -- seven (four)
for ACM-GCN++, whose residual branch adds a prologue launch -- behind ONE C-ABI call (``acm_small_step``, include/acm_hip.h; kernels: csrc/acm_small.hip).

Caller side of ACM-Pytorch/train.py:95-139 + utils.py:547-574 (and ACM-Geometric/train.py:119-140 on small data sets):
``train.TrainStep`` / ``train.EvalStep`` build a :class:`SmallPlan` when :func:`SmallPlan.why_not` finds nothing against it
-- Cora, Chameleon, Squirrel, Film ... with bag-of-words features (CSR) -- and then run a step as one ctypes call: no
autograd graph, no per-kernel Python dispatch, parameters updated in place by the kernels that finish their gradients
(the optimizer's own ``state`` tensors are used, so ``state_dict`` / checkpoints / a later switch to the general path see
exactly what ``optimizer.step()`` would have left).

Envelope: ``GCN`` of model_type acmgcn | acmgcnp | acmgcnpp (the last with ``init_layers_X = 1``: one Linear with bias of the
hidden width as the residual branch; deeper ``mlpX`` stacks stay on the general path, and so do acmgcnpp runs in the batched
forms below), two layers, hidden width 32 or 64, <= 8 classes, <= 16384 nodes, pattern-only
operators on one device, CSR features (``graph.SparseFeatures``, or dense features the model's ``auto_csr`` turns into one),
counter-based dropout (or none), this package's FusedAdam / FusedAdamW with one parameter group.  Anything else stays on
the general path (``why_not`` says why).
"""
import ctypes as C

import torch

from . import _lib, tuning
from .graph import FilterOperators, SparseFeatures, _device_ctx, _stream

_F32 = torch.float32
_ON_DEVICE = lambda t: t.is_cuda          # noqa: E731  (the CPU test double of the library lifts this guard)
MAX_ROWS = 16384
HIDDEN = (32, 64)                         # the widths acm_small.hip instantiates
MAX_CLASSES = 8


def hidden_widths(lib=None):
    """The hidden widths the loaded library's small step runs.  The real library always has ``acm_small_step_has_hidden``
    (``_lib`` requires every declared symbol); the object without it is the CPU test double (tests/fake_lib.py), whose small
    step has 64 written in and ignores the struct's ``hidden`` field, so only 64 is offered to it."""
    probe = getattr(lib if lib is not None else _lib.load(), "acm_small_step_has_hidden", None)
    if probe is None:
        return (64,)
    return tuple(w for w in HIDDEN if probe(w))

def has_residual(lib=None):
    """Whether the loaded library's small step runs the ACM-GCN++ residual branch (``acm_small_step_has_residual``).  The CPU
    test double (tests/fake_lib.py) lacks the symbol and is never offered an acmgcnpp plan."""
    probe = getattr(lib if lib is not None else _lib.load(), "acm_small_step_has_residual", None)
    return bool(probe is not None and probe())


# the residual branch's two tensors: acm_small_step_t.res[k], and the names their gradients go by in plan.grads
_RES_NAMES = ("weight", "bias")


def _res_params(model):
    lin = model.mlpX.lins[0]
    return lin.weight, lin.bias


_ROLE_NAMES = {
    _lib.SR_W_LOW: "weight_low", _lib.SR_W_HIGH: "weight_high", _lib.SR_W_MLP: "weight_mlp",
    _lib.SR_V_LOW: "att_vec_low", _lib.SR_V_HIGH: "att_vec_high", _lib.SR_V_MLP: "att_vec_mlp", _lib.SR_V_STRUC: "att_struc_low",
    _lib.SR_LNW_LOW: "layer_norm_low.weight", _lib.SR_LNW_HIGH: "layer_norm_high.weight", _lib.SR_LNW_MLP: "layer_norm_mlp.weight",
    _lib.SR_LNW_STRUC: "layer_norm_struc_low.weight",
    _lib.SR_LNB_LOW: "layer_norm_low.bias", _lib.SR_LNB_HIGH: "layer_norm_high.bias", _lib.SR_LNB_MLP: "layer_norm_mlp.bias",
    _lib.SR_LNB_STRUC: "layer_norm_struc_low.bias",
    _lib.SR_MIX: "att_vec", _lib.SR_STRUC: "struc_low",
}


def _roles(cfg):
    """The roles of a layer that take part in the forward (and so take a gradient) under ``cfg``."""
    four = cfg.n_channels == 4
    roles = [_lib.SR_W_LOW, _lib.SR_W_HIGH, _lib.SR_W_MLP, _lib.SR_V_LOW, _lib.SR_V_HIGH, _lib.SR_V_MLP, _lib.SR_MIX]
    if four:
        roles += [_lib.SR_V_STRUC, _lib.SR_STRUC]
    if cfg.layernorm:
        roles += [_lib.SR_LNW_LOW, _lib.SR_LNW_HIGH, _lib.SR_LNW_MLP, _lib.SR_LNB_LOW, _lib.SR_LNB_HIGH, _lib.SR_LNB_MLP]
        if four:
            roles += [_lib.SR_LNW_STRUC, _lib.SR_LNB_STRUC]
    return roles


def _param(layer, role):
    obj = layer
    for part in _ROLE_NAMES[role].split("."):
        obj = getattr(obj, part)
    return obj


def _has_hooks(model, optimizer=None):
    """Forward / backward hooks on any module, gradient hooks on any parameter, step hooks on the optimizer."""
    for m in model.modules():
        if m._forward_hooks or m._forward_pre_hooks or m._backward_hooks or getattr(m, "_backward_pre_hooks", None):
            return True
    for p in model.parameters():
        if getattr(p, "_backward_hooks", None) or getattr(p, "_post_accumulate_grad_hooks", None):
            return True
    if optimizer is not None:
        if getattr(optimizer, "_optimizer_step_pre_hooks", None) or getattr(optimizer, "_optimizer_step_post_hooks", None):
            return True
    return False


class SmallPlan:
    """Everything ``acm_small_step`` needs, bound once to (model, optimizer, features, operators, labels, row weights).

    What a caller of TrainStep / EvalStep does NOT get on this path (by construction: the step is six kernels, not a forward,
    a backward and an optimizer call): ``p.grad`` stays None (``keep_grads=True`` writes the gradients to ``plan.grads``
    instead), ``model.forward`` and ``optimizer.step`` are not called -- hooks would not fire, so ``why_not`` refuses a
    hooked model / parameter / optimizer -- and hyper-parameters are read on every call (eager) or baked in at capture
    (``use_graph``: like the general path, re-capture after a scheduler changed ``lr``).  Parameters and the optimizer's
    own state tensors are updated in place: ``state_dict()`` of both is what a stock loop would have left."""

    @staticmethod
    def why_not(model, x, ops, optimizer=None, need_dropout_state=True):
        """None if the fused small-graph step applies, else the first reason it does not (a string)."""
        from .optim import _FusedAdamBase
        if tuning.HOST.small_step <= 0:
            return "switched off (tuning small_step=0)"
        if getattr(model, "model_type", None) not in ("acmgcn", "acmgcnp", "acmgcnpp"):
            return f"model_type {getattr(model, 'model_type', None)!r} (acmgcn | acmgcnp | acmgcnpp)"
        gcns = getattr(model, "gcns", None)
        if gcns is None or len(gcns) != 2:
            return "not a two-layer model"
        l0, l1 = gcns
        residual = model.model_type == "acmgcnpp"
        if residual:
            if not has_residual():
                return "model_type 'acmgcnpp' (acmgcn | acmgcnp): library without the residual step"
            lins = getattr(getattr(model, "mlpX", None), "lins", None)
            if lins is None or len(lins) != 1:
                return f"mlpX with {len(lins) if lins is not None else 0} Linears (init_layers_X = 1 only)"
            lin = lins[0]
            if lin.bias is None:
                return "mlpX Linear without bias"
            if lin.in_features != l0.in_features or lin.out_features != l0.out_features:
                return (f"mlpX Linear {lin.in_features} -> {lin.out_features} (the first layer is "
                        f"{l0.in_features} -> {l0.out_features})")
        widths = hidden_widths()
        if l0.out_features not in widths or l1.in_features != l0.out_features:
            return f"hidden width {l0.out_features} ({' | '.join(map(str, widths))})"
        if not 1 <= l1.out_features <= MAX_CLASSES:
            return f"{l1.out_features} classes (<= {MAX_CLASSES})"
        c0, c1 = l0._config(), l1._config()
        if (c0.n_channels, c0.relu_before, c0.layernorm, c0.gather_bf16) != (c1.n_channels, c1.relu_before, c1.layernorm, c1.gather_bf16):
            return "the two layers are configured differently"
        if c0.gather_bf16:
            return "bf16 gather tables"
        if not isinstance(ops, FilterOperators) or ops.sharded or getattr(ops, "general", False) or not ops.implicit:
            return "operators: one device, pattern-only form"
        if ops.perm is not None or int(getattr(ops, "hops", 1)) != 1:
            return "relabelled / k-hop operators"
        n = ops.low.n_rows
        if not 1 <= n <= min(MAX_ROWS, tuning.HOST.small_step) or ops.low.n_cols != n:
            return f"{n} rows (<= {min(MAX_ROWS, tuning.HOST.small_step)})"
        if c0.n_channels == 4 and ops.deg is None:
            return "structure channel without degrees"
        if not isinstance(x, SparseFeatures):
            return "dense features (CSR features only)"
        if x.shape != (n, l0.in_features) or x.values.dtype != _F32 or not _ON_DEVICE(x.values):
            return "feature matrix shape / dtype / device"
        dev = x.values.device
        if any(p.device != dev or p.dtype != _F32 or not p.is_contiguous() for p in model.parameters()):
            return "parameters: contiguous fp32 on the features' device"
        if l0.struc_low.shape[0] != n and c0.n_channels == 4:
            return "struc_low rows"
        p_drop = float(getattr(model, "dropout", 0.0))
        if p_drop > 0 and need_dropout_state and not getattr(model, "fused_dropout", False):
            return "F.dropout masks (counter-based dropout only)"
        if _has_hooks(model, optimizer):
            # the fused step never calls model.forward, never materialises a .grad and never calls optimizer.step():
            # nothing a hook is attached to happens, so a hooked model / parameter / optimizer keeps the path
            # on which its hooks fire
            return "hooks registered on the model, a parameter or the optimizer"
        if optimizer is not None:
            if not isinstance(optimizer, _FusedAdamBase) or len(optimizer.param_groups) != 1:
                return "optimizer: FusedAdam / FusedAdamW with one parameter group"
            have = {id(p) for p in optimizer.param_groups[0]["params"]}
            for layer, cfg in ((l0, c0), (l1, c1)):
                if any(id(_param(layer, r)) not in have for r in _roles(cfg)):
                    return "a parameter of the model is not in the optimizer's group"
            if residual and any(id(t) not in have for t in _res_params(model)):
                return "a parameter of mlpX is not in the optimizer's group"
        return None

    def __init__(self, model, x, ops, labels=None, weights=None, optimizer=None, update=True, keep_grads=False):
        """``optimizer`` None: an evaluation plan (forward only).  ``update=False``: the step stops at the gradients
        (``self.grads[(layer, role name)]``; nothing is updated, no optimizer state is touched); ``keep_grads``: an
        updating plan that ALSO writes every gradient there (tests; the kernels store them on the way)."""
        lib = _lib.load()
        self.model, self.x, self.ops, self.opt = model, x, ops, optimizer
        l0, l1 = model.gcns
        cfg = l0._config()
        self.cfg = cfg
        n, dev = ops.low.n_rows, x.values.device
        self.n, self.C, self.hidden = n, l1.out_features, l0.out_features
        self.train = labels is not None                 # labels + row weights: a training plan; neither: evaluation
        self.residual = model.model_type == "acmgcnpp"  # (why_not has asked the library: has_residual)
        self._xt = x.csr_t if self.train else None
        self.low = self._operator(ops)
        nbytes = C.c_size_t()
        xt_handle = self._xt.handle if self._xt is not None else None
        if self.residual:
            # the residual's buffers lie behind the blocks every plan has: sized by the entry that takes the shape
            shape = _lib.SmallStep()
            shape.residual, shape.f_in, shape.hidden = 1, l0.in_features, l0.out_features
            _lib.check(lib.acm_small_step_workspace_bytes_for(self.low.handle, x.csr.handle, xt_handle, C.byref(shape), C.byref(nbytes)),
                       "acm_small_step_workspace_bytes_for")
        else:
            _lib.check(lib.acm_small_step_workspace_bytes(self.low.handle, x.csr.handle, xt_handle, C.byref(nbytes)),
                       "acm_small_step_workspace_bytes")
        self.workspace = torch.zeros(nbytes.value // 4, dtype=_F32, device=dev)     # zero once: counters, pad columns
        self.logits = torch.empty(n, self.C, dtype=_F32, device=dev)
        self.att1 = torch.zeros(n, 4, dtype=_F32, device=dev)
        self.att2 = torch.zeros(n, 4, dtype=_F32, device=dev)
        self.loss = torch.zeros((), dtype=_F32, device=dev)
        self.arrive = torch.zeros(1, dtype=torch.int32, device=dev)
        self.labels = labels.to(torch.int64).contiguous() if labels is not None else None
        self.weights = weights.to(_F32).contiguous() if weights is not None else None
        self._keep = []
        p = self.p = _lib.SmallStep()
        p.n_classes, p.n_channels, p.relu_before, p.layernorm = self.C, cfg.n_channels, int(cfg.relu_before), int(cfg.layernorm)
        # every width-dependent buffer of a plan is either the model's own (parameters, `grads` as zeros_like of them, the
        # optimizer's state) or sized for the widest width by the library (the workspace): the width is this one field
        p.hidden = self.hidden
        p.residual = int(self.residual)
        self.update = bool(update) and self.train and optimizer is not None
        self.grads = {}
        if self.train and (keep_grads or not self.update):
            for li, layer in enumerate(model.gcns):
                for role in _roles(cfg):
                    self.grads[(li, _ROLE_NAMES[role])] = torch.zeros_like(_param(layer, role))
            if self.residual:
                for name, t in zip(_RES_NAMES, _res_params(model)):
                    self.grads[("mlpX", name)] = torch.zeros_like(t)
        p.scale, p.train, p.update = cfg.scale, int(self.train), int(self.update)
        p.f_in = l0.in_features
        p.x_vals = x.values.data_ptr()
        if self._xt is not None:
            p.xt_src_pos = self._xt._src_pos_ptr
            # the (static) values in the transposed order: made once per feature object and shared by its plans (the slots of
            # a SmallBatch must name the same buffer), remade when the values were replaced or edited in place
            key = (x.values.data_ptr(), x.values._version)
            held = x.__dict__.get("_small_xt_vals")
            if held is None or held[0] != key:
                held = x.__dict__["_small_xt_vals"] = (key, x.values.index_select(0, self._xt.src_pos))
            self.xt_vals = held[1]
            p.xt_vals = self.xt_vals.data_ptr()
        p.row_scale = ops.row_scale.data_ptr()
        p.logits, p.att1, p.att2, p.loss = self.logits.data_ptr(), self.att1.data_ptr(), self.att2.data_ptr(), self.loss.data_ptr()
        p.arrive = self.arrive.data_ptr()
        p.workspace, p.workspace_bytes = self.workspace.data_ptr(), self.workspace.numel() * 4
        if self.train:
            p.labels, p.row_weight = self.labels.data_ptr(), self.weights.data_ptr()
        self._bind_parameters()
        self.refresh_hyper()

    @staticmethod
    def _operator(ops):
        """The operator handle the six launches walk: ops.low itself, or a copy of its pattern cut into work items of the
        length that suits one-item-per-wave kernels (made once per operator set, kept on it).  Measured (captured ms per step,
        chunk 128 / 256 / 512): Squirrel 0.192 / 0.168 / 0.179, Chameleon 0.102 / 0.114 / 0.130, Cora (longest row 168) 0.086 /
        0.079 / 0.078 -- short rows want no pieces at all, long rows on a dense graph want pieces of ~3 x the mean degree."""
        low = ops.low
        n, nnz = low.n_rows, low.nnz
        if low.max_degree <= 256:
            want = 128 if low.max_degree <= 128 else 256
        else:
            want = 128 if nnz < 48 * n else 256
        if int(low.chunk) == want or low.n_long_rows == 0 and low.max_degree <= want:
            return low
        cache = ops.__dict__.setdefault("_small_low", {})
        if want not in cache:
            from .graph import CsrGraph
            ip, ix, _ = low.arrays()
            cache[want] = CsrGraph.from_csr(ip, ix, None, low.n_cols, chunk=want)
        return cache[want]

    def _tensors(self):
        """(the struct's entry, the parameter, its key in ``grads``) of every tensor the step reads: the roles of the two
        layers, then -- ACM-GCN++ -- the residual branch's weight and bias."""
        p = self.p
        for li, layer in enumerate(self.model.gcns):
            for role in _roles(self.cfg):
                yield p.t[li][role], _param(layer, role), (li, _ROLE_NAMES[role])
        if self.residual:
            for k, t in enumerate(_res_params(self.model)):
                yield p.res[k], t, ("mlpX", _RES_NAMES[k])

    def _bind_parameters(self):
        for e, t, name in self._tensors():
            e.param, e.numel = t.data_ptr(), t.numel()
            g = self.grads.get(name)
            e.grad = g.data_ptr() if g is not None else None
            if self.update:
                st = self.opt.state[t]
                if len(st) == 0:
                    st["step"] = torch.zeros((), dtype=_F32, device=t.device)
                    st["exp_avg"] = torch.zeros_like(t, memory_format=torch.preserve_format)
                    st["exp_avg_sq"] = torch.zeros_like(t, memory_format=torch.preserve_format)
                else:
                    self.opt._normalize_state(t, st)
                e.exp_avg, e.exp_avg_sq, e.step = st["exp_avg"].data_ptr(), st["exp_avg_sq"].data_ptr(), st["step"].data_ptr()
        self._bound = self._binding_key()

    def _binding_key(self):
        key = []
        for _, t, _name in self._tensors():
            st = self.opt.state.get(t, {}) if self.update else {}
            key.append((t.data_ptr(), st["exp_avg"].data_ptr() if st else 0, st["step"].data_ptr() if st else 0))
        return tuple(key)

    def refresh_hyper(self):
        """Hyper-parameters and dropout state as they are NOW (a scheduler may have changed lr; a loop sets the dropout
        state after constructing the model)."""
        p, model = self.p, self.model
        if self.update:
            g = self.opt.param_groups[0]
            p.lr, p.beta1, p.beta2, p.eps = float(g["lr"]), float(g["betas"][0]), float(g["betas"][1]), float(g["eps"])
            p.weight_decay, p.decoupled = float(g["weight_decay"]), int(self.opt._decoupled)
            adv = getattr(self.opt, "also_advance", None)
            p.also_advance = adv.data_ptr() if adv is not None else None
        pd = float(getattr(model, "dropout", 0.0))
        st = getattr(model, "dropout_state", None)
        training = self.train
        if training and pd > 0:
            if st is None:
                raise RuntimeError("SmallPlan: the model has dropout but no dropout_state (counter-based dropout only)")
            p.drop_in, p.drop_hidden = st.spec(pd, 0, 0), st.spec(pd, 1, self.ops.row_offset)
            # (tag 2: the mask the general path draws for the residual branch, models.GCN._forward_fused_dropout)
            p.drop_res = st.spec(pd, 2, self.ops.row_offset) if self.residual else _lib.Dropout()
        else:
            p.drop_in, p.drop_hidden, p.drop_res = _lib.Dropout(), _lib.Dropout(), _lib.Dropout()

    def stale(self):
        """A parameter or an optimizer state tensor was replaced (load_state_dict, .to()): bind again."""
        return self._binding_key() != self._bound

    def run(self):
        """One call = the step (training plan) or the forward (evaluation plan).  Returns the loss tensor / the logits."""
        if self.stale():
            self._bind_parameters()
        self.refresh_hyper()
        from .functional import _Timed
        dev = self.logits.device
        with _device_ctx(dev), _Timed("small_step" if self.train else "small_forward"):
            st = _lib.load().acm_small_step(self.low.handle, self.x.csr.handle, self._xt.handle if self._xt is not None else None,
                                            C.byref(self.p), _stream())
        _lib.check(st, "acm_small_step")
        l0, l1 = self.model.gcns
        for layer, att in ((l0, self.att1), (l1, self.att2)):
            layer._att_raw, layer._att_inv, layer._att_k = att, None, self.cfg.n_channels
        return self.loss if self.train else self.logits


_BATCH_RESIDUAL = "residual plans (acmgcnpp) run as single steps: the batched launches have no residual form"


class SmallBatch:
    """B <= 32 :class:`SmallPlan` s over the SAME feature and operator objects -- all training plans or all evaluation plans --
    whose steps go through ONE set of six (three) launches (``acm_small_batch_step``): grid row k is plan k's single step, bit
    for bit.  The runs of the reference's ten-split loop (ACM-Pytorch/train.py:49-139) and of its hyper-parameter grid
    (hyperparameter_searching.py:51-70) share the graph and the features and nothing else: ``lr``, ``betas``, ``eps``,
    ``weight_decay``, Adam or AdamW, the dropout probability and the dropout state are per slot.

    The per-slot arguments live in a device table this object owns.  ``run()`` is one C call; it binds the table again first
    (``acm_small_batch_bind``) when a plan is ``stale()`` or a plan's hyper-parameters changed -- the ``refresh_hyper`` rule of
    the single plan: read on every eager call, baked at capture.  ``set_slot(i, plan_or_None)`` hands a slot to another run
    (None: an empty slot, which every launch skips); a captured ``run()`` keeps replaying, the table's address is all it
    baked in."""

    @staticmethod
    def why_not(plans):
        """None if the plans can share launches, else the first reason they cannot (a string)."""
        plans = [p for p in plans if p is not None]
        if not plans:
            return "no plan"
        if len(plans) > _lib.SMALL_BATCH_MAX:
            return f"{len(plans)} plans (<= {_lib.SMALL_BATCH_MAX} slots)"
        first = plans[0]
        if any(p.residual for p in plans):
            return _BATCH_RESIDUAL
        for p in plans[1:]:
            if (p.cfg.n_channels, p.cfg.relu_before, p.cfg.layernorm, p.cfg.scale) != \
                    (first.cfg.n_channels, first.cfg.relu_before, first.cfg.layernorm, first.cfg.scale):
                return "the models are configured differently"
            if p.hidden != first.hidden:
                return f"hidden widths {p.hidden} and {first.hidden}: the models are configured differently"
            if p.C != first.C:
                return f"{p.C} and {first.C} classes"
            if p.x is not first.x:
                return "different feature objects"
            if p.ops is not first.ops or p.low is not first.low:
                return "different operator objects"
            if (p.train, p.update) != (first.train, first.update):
                return "training and evaluation plans (or updating and gradient-only plans) mixed"
        return None

    def __init__(self, plans, n_slots=None):
        why = self.why_not(plans)
        if why is not None:
            raise ValueError(f"SmallBatch: {why}")
        lib = _lib.load()
        self.n_slots = int(n_slots) if n_slots is not None else len(plans)
        if not 1 <= self.n_slots <= _lib.SMALL_BATCH_MAX or len(plans) > self.n_slots:
            raise ValueError(f"SmallBatch: {len(plans)} plans in {self.n_slots} slots (1 .. {_lib.SMALL_BATCH_MAX})")
        self.plans = list(plans) + [None] * (self.n_slots - len(plans))
        first = self._first()
        self.low, self.x, self._xt, self.train = first.low, first.x, first._xt, first.train
        nbytes = C.c_size_t()
        _lib.check(lib.acm_small_batch_table_bytes(self.n_slots, C.byref(nbytes)), "acm_small_batch_table_bytes")
        self.table = torch.zeros(nbytes.value, dtype=torch.uint8, device=first.logits.device)     # zero: every slot empty
        self._slots = (C.POINTER(_lib.SmallStep) * self.n_slots)()
        self._bound = None

    def _first(self):
        return next(p for p in self.plans if p is not None)

    def set_slot(self, i, plan):
        """Slot ``i`` belongs to ``plan`` from the next ``run()`` / replay on (None: empty).  Table bytes only: call it when
        nothing that reads the table is in flight (after the synchronising look at the runs' state)."""
        if plan is not None:
            others = [p for k, p in enumerate(self.plans) if k != i and p is not None]
            why = self.why_not(others[:1] + [plan])
            if why is not None:
                raise ValueError(f"SmallBatch.set_slot: {why}")
        self.plans[i] = plan
        if any(p is not None for p in self.plans):
            self.bind()
        else:
            self.table.zero_()
            self._bound = None

    def _state(self):
        return tuple(bytes(p.p) if p is not None else None for p in self.plans)

    def _fill_slots(self):
        """The plans' blocks as they are now into the host array of slot pointers (None: an empty slot)."""
        for i, p in enumerate(self.plans):
            if p is not None:
                if p.stale():
                    p._bind_parameters()
                p.refresh_hyper()
                l0, l1 = p.model.gcns
                for layer, att in ((l0, p.att1), (l1, p.att2)):
                    layer._att_raw, layer._att_inv, layer._att_k = att, None, p.cfg.n_channels
            self._slots[i] = C.pointer(p.p) if p is not None else None

    def bind(self):
        """Write the table from the plans as they are now (not capturable)."""
        self._fill_slots()
        dev = self.table.device
        with _device_ctx(dev):
            st = _lib.load().acm_small_batch_bind(self.low.handle, self.x.csr.handle, self._xt.handle if self._xt is not None else None,
                                                  self.n_slots, self._slots, self.table.data_ptr(), self.table.numel(), _stream())
        _lib.check(st, "acm_small_batch_bind")
        self._bound = self._state()

    def _changed(self):
        for p in self.plans:
            if p is not None:
                if p.stale():
                    return True
                p.refresh_hyper()
        return self._bound is None or self._state() != self._bound

    def run(self):
        """One call = every slot's step (training plans) or forward (evaluation plans).  Results are in the plans' own
        buffers (``plan.loss`` / ``plan.logits``)."""
        capturing = self.table.is_cuda and torch.cuda.is_current_stream_capturing()
        if not capturing and self._changed():
            self.bind()
        if self._bound is None:
            raise RuntimeError("SmallBatch.run: bind() the table before capturing a run")
        from .functional import _Timed
        with _device_ctx(self.table.device), _Timed("small_batch_step" if self.train else "small_batch_forward"):
            st = _lib.load().acm_small_batch_step(self.low.handle, self.x.csr.handle, self._xt.handle if self._xt is not None else None,
                                                  self.n_slots, C.byref(self._first().p), self.table.data_ptr(), _stream())
        _lib.check(st, "acm_small_batch_step")


def _handle_value(h):
    return h.value if isinstance(h, C.c_void_p) else h


class SmallGraphBatch(SmallBatch):
    """B <= 32 :class:`SmallPlan` s on DIFFERENT graphs in ONE set of six (three) launches (``acm_small_batch_step_graphs``):
    the runs of synthetic-experiments/train.py:64-164, which trains on ten generated graphs per edge-homophily level, each
    with its own adjacency, features, labels and split.  The plans must agree in the number of rows, ``f_in``, the class
    count, the model configuration and the hidden width; operator, features, row scale, labels and weights are per slot.
    Grid row k is still plan k's single step, bit for bit: a slot's table entry is made from ITS handles, so it loops with
    its own workgroup counts over its own workspace; the launches are as wide as the widest run and the workgroups past a
    slot's own width return at once.

    ``handles``: ``(operator, features, transposed features or None)`` of EVERY run that will ever hold a slot
    (:meth:`handles_of`), beside those of ``plans``: their launch widths fold into ``self.grids``, the envelope a captured
    ``run()`` bakes in.  ``set_slot`` then hands a slot to a run on another graph by table bytes; a plan whose graph needs a
    wider launch than the envelope is refused with the library's message (and the slot keeps its run)."""

    @staticmethod
    def handles_of(x, ops, train):
        """The handles a :class:`SmallPlan` over (x, ops) walks, without building the plan."""
        return SmallPlan._operator(ops), x.csr, (x.csr_t if train else None)

    @staticmethod
    def why_not(plans):
        """None if the plans can share launches, else the first reason they cannot (a string)."""
        plans = [p for p in plans if p is not None]
        if not plans:
            return "no plan"
        if len(plans) > _lib.SMALL_BATCH_MAX:
            return f"{len(plans)} plans (<= {_lib.SMALL_BATCH_MAX} slots)"
        first = plans[0]
        if any(p.residual for p in plans):
            return _BATCH_RESIDUAL
        for p in plans[1:]:
            if (p.cfg.n_channels, p.cfg.relu_before, p.cfg.layernorm, p.cfg.scale) != \
                    (first.cfg.n_channels, first.cfg.relu_before, first.cfg.layernorm, first.cfg.scale):
                return "the models are configured differently"
            if p.hidden != first.hidden:
                return f"hidden widths {p.hidden} and {first.hidden}: the models are configured differently"
            if p.C != first.C:
                return f"{p.C} and {first.C} classes"
            if p.n != first.n:
                return f"graphs of {p.n} and {first.n} rows (one row count per batch)"
            if p.p.f_in != first.p.f_in:
                return f"{p.p.f_in} and {first.p.f_in} input features"
            if (p.train, p.update) != (first.train, first.update):
                return "training and evaluation plans (or updating and gradient-only plans) mixed"
        return None

    def __init__(self, plans, n_slots=None, handles=None):
        super().__init__(plans, n_slots)
        lib, first = _lib.load(), self._first()
        self.grids = _lib.SmallBatchGrids()
        for low, xc, xt in list(handles or []) + [(p.low, p.x.csr, p._xt) for p in self.plans if p is not None]:
            if low.n_rows != first.n:
                raise ValueError(f"SmallGraphBatch: graphs of {low.n_rows} and {first.n} rows (one row count per batch)")
            _lib.check(lib.acm_small_batch_grids(low.handle, xc.handle, xt.handle if xt is not None else None, C.byref(first.p),
                                                 C.byref(self.grids)), "acm_small_batch_grids")
        self._a, self._x, self._t = ((C.c_void_p * self.n_slots)() for _ in range(3))

    def set_slot(self, i, plan):
        held = self.plans[i]
        try:
            super().set_slot(i, plan)
        except Exception:
            self.plans[i] = held              # (a refused bind wrote nothing: the table still holds the run before)
            raise

    def bind(self):
        """Write the table from the plans as they are now, every slot from its own handles (not capturable)."""
        self._fill_slots()
        for i, p in enumerate(self.plans):
            self._a[i] = _handle_value(p.low.handle) if p is not None else None
            self._x[i] = _handle_value(p.x.csr.handle) if p is not None else None
            self._t[i] = _handle_value(p._xt.handle) if p is not None and p._xt is not None else None
        with _device_ctx(self.table.device):
            st = _lib.load().acm_small_batch_bind_graphs(self.n_slots, self._a, self._x, self._t, self._slots, C.byref(self.grids),
                                                         self.table.data_ptr(), self.table.numel(), _stream())
        _lib.check(st, "acm_small_batch_bind_graphs")
        self._bound = self._state()

    def run(self):
        """One call = every slot's step (training plans) or forward (evaluation plans), each on its own graph."""
        capturing = self.table.is_cuda and torch.cuda.is_current_stream_capturing()
        if not capturing and self._changed():
            self.bind()
        if self._bound is None:
            raise RuntimeError("SmallGraphBatch.run: bind() the table before capturing a run")
        from .functional import _Timed
        with _device_ctx(self.table.device), _Timed("small_batch_step" if self.train else "small_batch_forward"):
            st = _lib.load().acm_small_batch_step_graphs(self.n_slots, C.byref(self._first().p), C.byref(self.grids),
                                                         self.table.data_ptr(), _stream())
        _lib.check(st, "acm_small_batch_step_graphs")
