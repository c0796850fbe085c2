"""Training / evaluation harness around the ACM model: the callers of the hot path
(ACM-Geometric/train.py:107-162, data_utils.py:115-168; ACM-Pytorch/train.py:49-139,
utils.py:547-574), restated so the op can be trained and measured where the reference's Python
cannot run.

* ``TrainStep``      one full-batch step: forward, fused masked NLL (acm_nll_loss) or -- the reference's second
                     protocol, ``criterion="bce"`` -- masked BCE-with-logits on the one-hot labels (acm_bce_loss), backward,
                     optimizer update; optionally captured once in a HIP graph and replayed
                     (every launch of the step is stream-ordered and allocation-free, so the
                     whole step is one graph launch instead of ~60 kernel launches).
* ``evaluate``       eval-mode forward + accuracy (or, ``metric="rocauc"``, ROC-AUC) on index sets, on device (the
                     reference pulls the predictions to the host three times per epoch, data_utils.py:117-118, 132-135).
* ``EvalStep``       the same pass as an object: index sets as averaging weights, one device-to-host copy per pass, optionally
                     a hipGraph replay, optionally ending in the device-resident selection (functional.SelectionState).
* ``fit``            the two model-selection rules of the reference; with ``sync_every`` / ``keep_best`` the selection state
                     stays on the device across epochs (functional.SelectionState) and the selected model is returned.
* ``fit_concurrent`` several runs of ``fit`` on the same graph, ``streams`` at a time, each on a stream of its own.
* ``fit_batched``    several runs on the same small graph, ``batch`` at a time in the same launches (small.SmallBatch).
* ``fit_batched_graphs`` the same for runs on DIFFERENT small graphs of one row count (small.SmallGraphBatch).

Stated once for all of them: the model call (``_call_model``), the capture (``_captured``), the epoch loop (``_drive``) around
``enqueue`` / ``finished`` / ``result`` and the construction of a run (``_new_run``).
"""
import contextlib
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from . import _lib, functional as AF
from . import tuning
from .graph import FilterOperators, SparseFeatures, operators_for

_TORCH_DROPOUT = F.dropout          # to notice a patched F.dropout (mask replay in tests): see TrainStep
CRITERIA = ("nll", "bce")           # log_softmax + NLLLoss | BCEWithLogitsLoss on one-hot labels (ACM-Geometric/train.py:86-92)
METRICS = ("acc", "rocauc")         # eval_acc | eval_rocauc (data_utils.py:115-151)


def _checked(value, allowed, what):
    if value not in allowed:
        raise ValueError(f"{what} must be one of {allowed}, not {value!r}")
    return value


def row_weights(train_idx, n_rows, n_train_total=None, device=None):
    """w_i = 1/|train| on training rows else 0 (mean NLL over the training set)."""
    device = device if device is not None else train_idx.device
    w = torch.zeros(n_rows, dtype=torch.float32, device=device)
    total = n_train_total if n_train_total is not None else train_idx.numel()
    w[train_idx.to(device)] = 1.0 / float(total)
    return w


def _tape_safe(model):
    """models.GCN configurations whose training forward is a chain of this package's Functions only (nothing for a Tape to
    trip over): the two-layer ACM-GCN / ACM-GCN+ and the single-layer ACM-SGC.  ACM-GCN++ adds its residual branch with a
    torch operation unless the fused dropout's one-launch form applies; acmsnowball concatenates blocks."""
    from .models import GCN
    return type(model) is GCN and model.model_type in ("acmgcn", "acmgcnp", "acmsgc")


def _rng_snapshot(device):
    """States of the generators F.dropout draws from: torch's CPU generator and the device's."""
    dev = torch.device(device)
    cuda = torch.cuda.get_rng_state(dev) if (dev.type == "cuda" and not torch.cuda.is_current_stream_capturing()) else None
    return torch.get_rng_state(), cuda, dev


def _rng_restore(snap):
    if snap is None:
        return
    cpu, cuda, dev = snap
    torch.set_rng_state(cpu)
    if cuda is not None:
        torch.cuda.set_rng_state(cuda, dev)


def _buffers_restore(snap):
    """Put the model's buffers back (values cloned before a pass that has to be redone)."""
    if snap:
        with torch.no_grad():
            for b, v in snap:
                b.copy_(v)


def _held_entries(model):
    """What a captured step or pass over ``model`` reads beyond its graph's own pool: the layers' P = A_low X cache entries
    (layers.GraphConvolution._eval_agg_holder: key, input, {"agg": P, "xpad": ...}, operators) as they are right now.  The graph
    bakes in the address of the P its capture read (a dropout-0 step, every evaluation pass); only the layer's cache entry keeps
    that tensor alive, and another forward of the same model on another input object replaces the entry.  Held by the captured
    object, the replay keeps reading valid memory whatever the layers cache afterwards (use-after-free)."""
    held = []
    for m in model.modules():
        entries = getattr(m, "held_entries", None)
        if entries is not None:
            held.extend(entries())
    return held


def _capture_mode():
    """Keyword arguments of torch.cuda.graph for a capture.  With a process group alive, ProcessGroupNCCL's watchdog
    thread polls the events of earlier collectives (hipEventQuery) whenever it wakes up; under the default GLOBAL capture
    mode such a call from another thread while this thread captures is an error that aborts the process
    ("operation not permitted when stream is capturing", seen on a single-rank RCCL run).  Thread-local mode confines the
    restriction to the capturing thread."""
    import torch.distributed as dist
    if dist.is_available() and dist.is_initialized():
        return {"capture_error_mode": "thread_local"}
    return {}


def _operators_and_features(model, x, adj, adj_high, adj_un):
    """(operators, features) a step or pass over ``model`` works on: the reference's adjacency TENSORS become the operator set
    (the structure channel's degrees only for ACM-GCN+ / ++ with ``structure_info``), wide one-hot / bag-of-words features
    handed over dense become their CSR twin (tuning csr_features).  Anything else is handed back as it came."""
    ops = adj
    if not isinstance(adj, FilterOperators) and isinstance(adj, torch.Tensor) and hasattr(model, "structure_info"):
        four = model.structure_info and getattr(model, "model_type", "") in ("acmgcnp", "acmgcnpp")
        ops = operators_for(adj, adj_high, adj_un if four else None)
    if hasattr(model, "auto_csr"):
        x = model.auto_csr(x, ops if isinstance(ops, FilterOperators) else None)
    return ops, x


def _warm_up(fn, times):
    """``times`` eager calls of ``fn`` on a side stream before a capture (lazy handles, allocator pools, optimizer state);
    the device is idle on return."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(times):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()


def _captured(fn):
    """(a new hipGraph with ``fn()`` captured into it, what ``fn`` returned); warm-up, snapshots and resets are the caller's."""
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, **_capture_mode()):
        result = fn()
    return graph, result


def _takes_call(model):
    """Whether ``model.forward`` takes a step's or pass's CallContext as the ``call`` keyword (models.GCN does)."""
    import inspect
    try:
        return "call" in inspect.signature(model.forward).parameters
    except (TypeError, ValueError):
        return False


def _call_model(model, takes_call, inputs, call, tail=None, rows_permuted=False, ambient=True):
    """``model(*inputs)`` (x, adj, adj_high, adj_un) for a training step or an evaluation pass, with what ``call`` carries -- the
    deferral list, the input pipeline -- and the loss-tail request ``tail``: as the ``call`` keyword where ``forward`` takes it,
    otherwise (a wrapper around the model) as the thread's ambient contexts, from which the model derives its own context.
    ``ambient=False`` (EvalStep): a model without the keyword is called plainly -- the one known difference between a step and
    a pass, decided here and nowhere else: a pass has no context of its own to enter, and enters none."""
    kw = {"rows_permuted": True} if rows_permuted else {}
    if takes_call:
        if tail is not None:
            call.tail = tail
        out = model(*inputs, call=call, **kw)
        if tail is not None:
            call.tail = None
        return out
    if not ambient:
        return model(*inputs, **kw)
    with AF.deferred_reductions_as(call.defer), AF.input_pipeline(call.pipe), tail if tail is not None else contextlib.nullcontext():
        return model(*inputs, **kw)


def _note_elision(step, call):
    """``step.hidden_elided`` / ``hidden_elided_refused`` (TrainStep, EvalStep) from what the model call's hidden layer reported."""
    done, why = call.elision if call.elision is not None else (False, "no aggregate-first hidden layer ran with this call")
    step.hidden_elided, step.hidden_elided_refused = bool(done), why


class TrainStep:
    def __init__(self, model, optimizer, x, adj, labels, weights, adj_high=None, adj_un=None, use_graph=False,
                 fused_dropout=None, pipeline_input=None, steps_per_graph=1, flush_in_optimizer=True, small_step=None, tape=True,
                 criterion="nll"):
        """``criterion``: "nll" = log_softmax + NLLLoss on the weighted rows (acm_nll_loss, fused into the output layer where it
        qualifies); "bce" = nn.BCEWithLogitsLoss() against the one-hot labels (acm_bce_loss: ACM-Geometric/train.py:86-92,
        123-131 -- genius, twitch-e, yelp-chi, ``--rocauc``), always a launch of its own and never on the fused small-graph step
        (acm_conv_fwd_tail and acm_small_step compute the NLL).  The same row weights serve both.

        ``tape``: eager steps record this package's Functions on a functional.Tape and replay them backwards themselves
        instead of building an autograd graph (no Function.apply, no AccumulateGrad nodes, no engine hand-off: the host side of
        an eager step); a model with torch operations between its layers falls back to autograd on its first step, for good.

        ``small_step``: the fused six-launch step for small graphs (small.SmallPlan / acm_small_step): None = where it
        applies (``self.small`` is the plan, ``self.small_refused`` the reason it does not), False = never.  On that path
        ``p.grad`` stays None and neither ``model.forward`` nor ``optimizer.step`` is called (see small.SmallPlan): a model,
        parameter or optimizer with hooks registered keeps the general path.

        ``flush_in_optimizer``: with this package's FusedAdam / FusedAdamW the step's deferred gradient sums are flushed by
        the optimizer's own launch (acm_adam_config_t.pending) instead of a launch of their own.

        ``loss_rows`` (attribute): with the masked NLL on unsharded FilterOperators, when at least one row in eight has weight 0,
        the step attaches the set of weighted rows to the operators ONCE, here (graph.FilterOperators.loss_rows: host-side
        preprocessing that synchronises the device, so never inside the capture), and the output layer's forward gather and its
        row pass skip the other rows (acm_conv_fwd_tail_rows; tuning key ``loss_rows``).  Loss and
        parameters keep their bits; the logits of zero-weight rows are no longer computed inside the step.  ``loss_rows`` is
        the graph.LossRows in use, or None with the reason in ``loss_rows_refused``.  The NONZERO PATTERN of ``weights`` is
        fixed for the life of a captured step (as the reference fixes the split before its epoch loop, ACM-Geometric/train.py);
        an eager step re-checks ``weights._version`` and re-attaches after an in-place edit.

        ``steps_per_graph`` (with ``use_graph``): capture that many consecutive optimizer steps in ONE hipGraph, so that a
        call runs them all (``steps_per_call``; the loss returned is the last one, ``losses`` holds every one) -- the ~8 us
        between two graph launches is then paid once per call instead of once per step.  Every captured step is a complete
        step (fresh counter-based masks: the step counters live on the device); a loop that looks at the model between two
        steps (train.fit's evaluation pass) keeps the default of one."""
        self.model, self.opt = model, optimizer
        self.criterion = _checked(criterion, CRITERIA, "criterion")
        self.steps_per_call = max(int(steps_per_graph), 1) if use_graph else 1
        self.losses = []
        self.x, self.adj, self.adj_high, self.adj_un = x, adj, adj_high, adj_un
        self.labels, self.weights = labels, weights
        # Relabelled operators (graph.relabel_by_degree; operators_for applies it to large graphs): the static inputs
        # of the step -- features, labels, row weights -- are moved into the operator's numbering ONCE, and the step
        # never leaves it (the loss does not care about the order of the rows).
        self._permuted = False
        # the step keeps the operator set it built (the model's forward would look the same set up again, per call, by
        # the tensors' identity): a caller that hands over the reference's adjacency TENSORS -- the drop-in loop,
        # ACM-Pytorch/train.py:95-139 -- then reaches every plan that asks for FilterOperators, the fused small-graph
        # step first of all (round 5: such a caller silently stayed on the general path)
        ops, x = _operators_and_features(model, x, adj, adj_high, adj_un)
        self.adj, self.x = ops, x
        if isinstance(ops, FilterOperators) and ops.perm is not None and hasattr(model, "_forward"):
            self.x = x.permute_rows(ops.perm) if isinstance(x, SparseFeatures) else x.index_select(0, ops.perm)
            self.labels, self.weights = labels.index_select(0, ops.perm), weights.index_select(0, ops.perm)
            self._permuted = True
        self.graph, self.loss = None, None
        self._held = None                   # what a captured step reads beyond its graph's pool (see _capture)
        # counter-based dropout: this loop owns the step structure (one advance per optimizer step), so the
        # model may draw its masks inside the kernels; the advance rides FusedAdam's step-counter kernel
        # (default: on, unless someone replaced F.dropout -- a mask-replay harness must keep seeing its masks)
        self._manual_advance = False
        self._defer = True
        self._tape = bool(tape)
        self._pass_proven = False           # a pass went through without a redo: the model's buffers need no snapshot any more
        self._tape_proven = False           # a first taped step went through: the model's Functions are all this package's
        if self._tape and F.dropout is not _TORCH_DROPOUT and getattr(model, "dropout", 0) > 0 and not _tape_safe(model):
            # someone replaced F.dropout (a mask-replay harness: it hands out recorded masks by call position) and this model
            # may break the tape (torch operations between its layers): the redo of the step on autograd would draw the NEXT
            # masks of the harness -- its state cannot be put back like a generator's.  Such a step starts on autograd.
            self._tape = False
        from .optim import _FusedAdamBase
        self._opt_flushes = bool(flush_in_optimizer) and isinstance(optimizer, _FusedAdamBase)
        self._unflushed = None
        if fused_dropout is None:
            fused_dropout = F.dropout is _TORCH_DROPOUT
        if fused_dropout and getattr(model, "dropout", 0) > 0 and hasattr(model, "fused_dropout"):
            model.fused_dropout = True
            if model.dropout_state is None:
                model.dropout_state = AF.DropoutState(labels.device)
            if hasattr(optimizer, "also_advance"):
                optimizer.also_advance = model.dropout_state.step
            else:
                self._manual_advance = True
        self._params = list(model.parameters())          # walked every step: module.parameters() costs 0.1 ms of host time
        self._takes_call = _takes_call(model)
        # the first layer's input aggregation one step ahead, inside its own backward (functional.InputPipeline);
        # pipeline_input: None = when the configuration qualifies (InputPipeline.eligible), False = never
        self.pipe = None
        if pipeline_input is not False and not self._manual_advance and getattr(model, "fused_dropout", False) \
                and AF.InputPipeline.eligible(model, self.adj, self.x):
            self.pipe = AF.InputPipeline(self.adj, self.x, model.dropout, model.dropout_state, tag=0)
        # small graphs: the whole step behind one C-ABI call (six launches, updates applied where gradients finish)
        self.small, self.small_refused = None, "not requested"
        if small_step is not False:
            from .small import SmallPlan
            why = 'criterion="bce" (the fused step computes the masked NLL)' if self.criterion != "nll" else \
                "the loop advances the dropout counter by hand" if self._manual_advance else \
                SmallPlan.why_not(model, self.x, self.adj, optimizer)
            if why is None and getattr(model, "dropout", 0) > 0 and not getattr(model, "fused_dropout", False):
                why = "F.dropout masks (counter-based dropout only)"
            self.small_refused = why
            if why is None:
                self.small = SmallPlan(model, self.x, self.adj, self.labels, self.weights, optimizer)
                self.pipe = None
        self.loss_rows, self.loss_rows_refused = None, "not requested"
        if self.small is None:
            self._attach_loss_rows()
        # whether the last forward (the captured one, with use_graph) left the hidden activation unwritten (tuning key
        # ``elide_hidden``; functional.hidden_elision_why_not), and the reason if it did not
        self.hidden_elided, self.hidden_elided_refused = False, "no forward has run"
        if use_graph:
            self._capture()

    # below one zero-weight row in eight the forward gather can lose at most an eighth of its items (measured at one half: 52 ->
    # 41 us, EXPERIMENTS.md) while the row pass pays for its divergent zero stores whatever the share: not worth an attachment
    LOSS_ROWS_MIN_DROPPED = 0.125

    def _attach_loss_rows(self):
        """Build (or rebuild, after an in-place edit of the weights) the operators' loss-row attachment; never under capture."""
        old, self.loss_rows = self.loss_rows, None
        ops, w = self.adj, self.weights
        why = None
        if self.criterion != "nll":
            why = 'criterion="bce"'
        elif not tuning.HOST.loss_rows:
            why = "tuning: loss_rows=0"
        elif not isinstance(ops, FilterOperators) or ops.sharded or ops.general:
            why = "needs unsharded FilterOperators of the (A_low, I - A_low) pair"
        elif not isinstance(w, torch.Tensor) or w.dim() != 1 or w.numel() != ops.low.n_rows:
            why = "row weights of another shape"
        elif w.is_cuda and torch.cuda.is_current_stream_capturing():
            why = "the stream is capturing"
        elif int((w == 0).sum()) < self.LOSS_ROWS_MIN_DROPPED * w.numel():
            why = "fewer than one row in eight has weight 0"
        elif any(getattr(_lib.load(), name, None) is None for name in _lib.LOSS_ROWS_SYMBOLS):
            why = "the library lacks the loss-row entry points"
        else:
            self.loss_rows = ops.loss_rows(w, replaces=old)
            if self.loss_rows is None:
                why = "the operators refused (not square, or attached to another live step's weights)"
        self.loss_rows_refused = why

    def _one_step(self):
        """Forward + loss + backward + update (+ the dropout counter's advance): one step, eager or under capture."""
        if self.small is not None:
            loss = self.small.run()
        else:
            loss = self._forward_backward(for_optimizer=True)
            self._opt_step()
        self._count_advance()
        if self.pipe is not None:
            self.pipe.end_step()
        return loss

    def _forward_backward(self, for_optimizer=False):
        """Forward, fused loss and backward; the loss sum and the parameter-gradient sums of the backward kernels run
        as ONE deferred launch at the end (AF.deferred_reductions: four launches less per step).  That is only sound
        while nothing reads a gradient before the flush, which this method checks on every pass: every ``.grad``
        must be the tensor the backward kernels wrote (autograd adopts it when ``.grad`` is None), not a copy taken
        before the flush -- otherwise deferral is switched off for good and the step is redone.
        ``for_optimizer``: the caller runs ``_opt_step()`` next, which may take the flush into the optimizer's launch; without
        it the gradients and the loss are complete on return."""
        pipe = self.pipe
        if pipe is not None and pipe.stale():
            if self.x.is_cuda and torch.cuda.is_current_stream_capturing():
                self.pipe = pipe = None           # its buffers cannot be refilled inside a capture: the plain step
            else:
                pipe.prime()
        # this step's own context: the deferral list, the loss-tail request and the pipeline travel with the model call
        # (and, captured by the autograd Functions, with its backward) -- nothing is parked in module state
        pending = AF.DeferredReductions() if self._defer else None
        call = AF.CallContext(defer=pending, pipe=pipe)
        # eager steps: the Functions on the step's own tape (a capture keeps autograd: nothing to save in a replayed graph)
        tape = AF.Tape() if (self._tape and not (torch.cuda.is_available() and torch.cuda.is_current_stream_capturing())) else None
        # until a taped step has gone through once, the attempt may have to be redone on autograd: the generators' states are
        # put back first, so that the redo draws the masks (F.dropout) the aborted forward drew -- the step then IS the step an
        # autograd run of the same seeds takes (acmgcnpp trained on other masks with tape=True than with False)
        rng = _rng_snapshot(self.labels.device) if (tape is not None and not self._tape_proven) else None
        # ... and the model's buffers (BatchNorm running statistics and batch counter of a deep mlpX stack: the forward updates
        # them) -- until a pass has gone through without a redo: a redone step must count once
        buffers = None if self._pass_proven else [(b, b.detach().clone()) for b in getattr(self.model, "buffers", lambda: ())()]
        try:
            with AF.on_tape(tape):
                loss, dz, out = self._forward_loss(call)
            if pipe is not None:
                pipe.make_next()              # dropout_{t+1}(x): the operand of the gather the backward carries (only if
                                              # the forward adopted the pipeline's buffers)
            if tape is not None:
                tape.backward(out, dz)
                self._tape_proven = True
            else:
                out.backward(dz)
        except BaseException as err:
            # what abandoning an attempt releases, whatever ended it: the tape's records and the deferral list
            if tape is not None:
                tape.release()
            if pending is not None:
                pending.discard()
            # an in-place torch operation on a taped output fails inside torch ("a leaf Variable that requires grad is being
            # used in an in-place operation") before the tape can notice: the same verdict
            broken = isinstance(err, RuntimeError) and tape is not None and not self._tape_proven \
                and (isinstance(err, AF.TapeBroken) or "leaf Variable" in str(err))
            if not broken:
                raise
            # torch operations between the layers: this model's steps run on autograd from now on; the step is redone
            self._tape = False
            return self._redo(for_optimizer, pipe, buffers, rng)
        if pending is None:
            self._pass_proven = True
            return loss
        adopted = pending.all_adopted([loss] + [p.grad for p in self._params])
        # The optimizer's launch can flush the list itself (acm_adam_config_t.pending: one launch and one grid drain less)
        # when nothing has to come between the flush and the update: no gradient all-reduce, our own optimizer.
        self._unflushed = None
        if for_optimizer and adopted and self._opt_flushes and not pending.collectives_pending:
            self._unflushed = pending
            self._pass_proven = True
            return loss
        pending.flush()
        if not adopted:
            # a gradient was copied before the flush: no deferral from now on; the step is redone.  (No generator snapshot is
            # handed on: this redo draws its F.dropout masks from where the attempt left the generators, as it always has.)
            self._defer = False
            return self._redo(for_optimizer, pipe, buffers)
        self._pass_proven = True
        return loss

    def _redo(self, for_optimizer, pipe, buffers, rng=None):
        """The step again, after an attempt that must not count: what it moved is put back first -- the generators' states
        (where a snapshot is handed on), the model's buffers, the gradients, and the pipeline, whose buffers the attempt has
        already refilled for the NEXT step.  State that a step changes before its backward ends is added HERE."""
        _rng_restore(rng)
        _buffers_restore(buffers)
        self.opt.zero_grad(set_to_none=True)
        if pipe is not None:
            pipe.primed = False
        return self._forward_backward(for_optimizer)

    def _forward_loss(self, call):
        """Forward and loss: (loss, dloss/dlogits, logits).  With the NLL the model's output layer is asked to run its row
        phase, the loss and its own row-local backward as one kernel (AF.fused_loss_tail); where it does not qualify
        (wide output, structure channel, a wrapper around the output) -- and with ``criterion="bce"``, which asks for no tail
        (the fused tail computes the NLL) -- the loss is its own launch."""
        nll = self.criterion == "nll"
        lr = self.loss_rows
        if nll and lr is not None and not lr.current_for(self.weights):
            # the weights were edited in place: re-attach -- or, under a capture (no host-side preprocessing there), the full path
            if self.weights.is_cuda and torch.cuda.is_current_stream_capturing():
                lr = None
            else:
                self._attach_loss_rows()
                lr = self.loss_rows
        tail = AF.fused_loss_tail(self.labels, self.weights, loss_rows=lr) if nll else None
        out = _call_model(self.model, self._takes_call, (self.x, self.adj, self.adj_high, self.adj_un), call, tail, self._permuted)
        _note_elision(self, call)
        if tail is not None and tail.matches(out):
            return tail.loss, tail.dz, out
        # = masked_nll(...).backward() / masked_bce(...).backward(), two launches less
        loss, dz = (AF.nll_loss_and_grad if nll else AF.bce_loss_and_grad)(out, self.labels, self.weights, defer=call.defer)
        return loss, dz, out

    def _eager(self):
        if not self.model.training:
            self.model.train()
        if type(self.opt).zero_grad is torch.optim.Optimizer.zero_grad:
            for group in self.opt.param_groups:      # = the stock zero_grad(set_to_none=True) without its dispatch wrapper (30 us)
                for p in group["params"]:
                    p.grad = None
        else:
            self.opt.zero_grad(set_to_none=True)
        loss = self._one_step()
        return loss                 # never hand out the autograd graph: a live AccumulateGrad node pins its
                                    # stream and breaks a later graph capture

    def _snapshot(self):
        """Values of everything a training step changes: parameters / buffers, optimizer state, dropout counter."""
        model_state = [(t, t.detach().clone()) for t in self.model.state_dict().values() if torch.is_tensor(t)]
        opt_state = [(p, {k: (v.detach().clone() if torch.is_tensor(v) else v) for k, v in st.items()})
                     for p, st in self.opt.state.items()]
        ds = getattr(self.model, "dropout_state", None)
        return model_state, opt_state, ((ds.step.clone(), ds.host_steps) if ds is not None else None)

    def _restore(self, snap):
        """Put the snapshot back IN PLACE (the captured graph and the optimizer's pointer tables keep their addresses);
        optimizer state created since the snapshot is zeroed -- what a fresh optimizer starts from."""
        model_state, opt_state, drop_step = snap
        with torch.no_grad():
            for t, v in model_state:
                t.copy_(v)
            had = {id(p): st for p, st in opt_state}
            for p, st in self.opt.state.items():
                old = had.get(id(p))
                for k, v in st.items():
                    if not torch.is_tensor(v):
                        if old is not None and k in old:
                            st[k] = old[k]
                        continue
                    if old is not None and k in old:
                        v.copy_(old[k])
                    else:
                        v.zero_()
            if drop_step is not None:
                self.model.dropout_state.step.copy_(drop_step[0])
                self.model.dropout_state.host_steps = drop_step[1]
        if getattr(self, "pipe", None) is not None:
            self.pipe.primed = False            # its buffers belong to another counter value now

    def _capture(self):
        # NOTE for callers: no autograd graph of an earlier, un-captured backward through this model may still be alive
        # (e.g. a retained `out` of `out = model(x); loss(out).backward()`): its AccumulateGrad nodes are bound to the
        # stream they were created on, and the captured backward would have to synchronise with that stream --
        # torch aborts the capture (a segmentation fault in capture_end on ROCm).  Drop such references first.
        # The warm-up runs real steps (lazy handles, allocator pools, optimizer state) -- on a snapshot: the model,
        # the optimizer moments / step counts and the dropout counter are put back afterwards, so a captured
        # TrainStep starts from exactly the state an eager one starts from (fit(epochs=N) trains N steps, not N + 3).
        snap = self._snapshot()
        _warm_up(self._eager, 3)
        self._restore(snap)
        if self.pipe is not None:
            self.pipe.prime()                   # for the restored counter, outside the capture
            torch.cuda.synchronize()
        self.model.train()
        self.opt.zero_grad(set_to_none=True)
        self.graph, self.losses = _captured(self._steps_of_a_call)
        self.loss = self.losses[-1]
        self._held = _held_entries(self.model)

    def _steps_of_a_call(self):
        """The ``steps_per_call`` consecutive steps one graph holds: every step's loss scalar."""
        losses = []
        for k in range(self.steps_per_call):
            if k:
                self.opt.zero_grad(set_to_none=True)
            loss = self._one_step()
            if self.small is not None and self.steps_per_call > 1:
                loss = loss.clone()              # the plan's loss scalar is rewritten by the next step of the same graph
            losses.append(loss)
        return losses

    def refresh(self):
        """Re-capture after an in-place edit of the features (or of anything else the captured step read once: a captured
        step assumes ``x`` is static, like EvalStep)."""
        if self.graph is not None:
            self.graph = None
            if self.pipe is not None:
                self.pipe.primed = False
            if self.loss_rows is not None and not self.loss_rows.current_for(self.weights):
                self._attach_loss_rows()        # (the old graph is gone: nothing replays over the attachment it replaces)
            self._capture()

    def _opt_step(self):
        pending, self._unflushed = self._unflushed, None
        if pending is not None:
            self.opt.step(pending=pending)
        else:
            self.opt.step()

    def _count_advance(self):
        """The dropout counter moves once per optimizer step: by hand, or by the optimizer's kernel (the shadow follows)."""
        if self._manual_advance:
            self.model.dropout_state.advance()
        else:
            self._counter_moved(1, by="optimizer")

    def _counter_moved(self, k, by):
        """The dropout counter on the device has moved by ``k`` optimizer steps: its host shadow (``host_steps``) follows.  ``by``:
        "optimizer"  an eager ``optimizer.step()``: FusedAdam's kernel advances the counter where its ``also_advance`` is it
        "replay"     the captured step(s): they advanced it, and refilled this step's pipeline buffers for the new value
        "plan"       launches of fit_batched over this step's SmallPlan: an updating plan advances it"""
        ds = getattr(self.model, "dropout_state", None)
        if ds is None or (by == "optimizer" and getattr(self.opt, "also_advance", None) is not ds.step) \
                or (by == "plan" and not self.small.update):
            return
        ds.host_steps += k
        if by == "replay" and self.pipe is not None:
            self.pipe._host_steps = ds.host_steps

    def __call__(self):
        if self.graph is not None:
            self.graph.replay()
            self._counter_moved(self.steps_per_call, by="replay")
            return self.loss
        return self._eager()


@torch.no_grad()
def evaluate(model, x, adj, labels, index_sets, adj_high=None, adj_un=None, metric="acc"):
    """Eval-mode logits and the accuracy -- ``metric="rocauc"``: the ROC-AUC (AF.eval_rocauc; NaN where a set lacks a class)
    -- on each index set (data_utils.py:153-168)."""
    _checked(metric, METRICS, "metric")
    model.eval()
    out = model(x, adj, adj_high, adj_un)
    if metric == "rocauc":
        return out, AF.eval_rocauc(out, labels, _set_weights(index_sets, labels, mean=False)).tolist()
    pred = out.argmax(dim=1)
    accs = [float((pred[idx] == labels[idx]).float().mean()) for idx in index_sets]
    return out, accs


def _is_sharded(adj):
    return isinstance(adj, FilterOperators) and adj.sharded


def _selection_key(rule, metric_va, val_loss):
    """What ``fit`` maximises.  An undefined validation metric (a NaN ROC-AUC: the split lacks a class) never becomes "best":
    its key is None and the epoch is passed over."""
    key = metric_va if rule == "max_val_acc" else -val_loss
    return None if key != key else key


def _eager_val_loss(out, labels, val_idx, criterion):
    """The validation loss of an un-captured epoch, as the reference forms it (train.py:123-135)."""
    if criterion == "bce":
        target = (labels[val_idx].view(-1, 1) == torch.arange(out.shape[1], device=out.device).view(1, -1)).to(out.dtype)
        return float(F.binary_cross_entropy_with_logits(out[val_idx], target))
    return float(F.nll_loss(F.log_softmax(out, 1)[val_idx], labels[val_idx]))


def _set_weights(index_sets, labels, mean=True):
    """[k, n] fp32 rows: 1 / |set| (``mean``) or 1 on a set's rows, 0 elsewhere.  Index tensors or boolean masks."""
    n, dev = labels.shape[0], labels.device
    w = torch.zeros(len(index_sets), n, dtype=torch.float32, device=dev)
    for k, idx in enumerate(index_sets):
        idx = torch.as_tensor(idx, device=dev)
        idx = idx.nonzero().view(-1) if idx.dtype == torch.bool else idx.long()
        w[k].index_fill_(0, idx, 1.0 / max(int(idx.numel()), 1) if mean else 1.0)
    return w


class EvalStep:
    """The per-epoch evaluation pass of the reference's loops (ACM-Geometric/train.py:138-140 + data_utils.py:153-168,
    ACM-Pytorch/train.py:129-139): eval-mode logits, the accuracy on every index set and the NLL on one of them
    (``loss_set``: the validation set).  Everything stays on the device -- the index sets become [k, n] averaging
    weights, accuracies and loss land in one small tensor -- so a call costs ONE device-to-host copy, and with
    ``use_graph`` the whole pass (the library's forward kernels + a handful of torch reductions) is a hipGraph replay.
    Returns (logits, [accuracy per index set], loss on ``loss_set``).

    Index sets may be index tensors or boolean masks.  Rows outside every set may carry the reference's "unlabeled"
    marker -1 (data_utils.rand_train_test_idx, ignore_negative): they have zero weight and their label is clamped before
    the gather.  A CAPTURED pass bakes in the addresses of what its warm-up left behind -- in particular the first layer's
    P = A_low X of an aggregate-first layer (layers.GraphConvolution._eval_agg) -- so it assumes ``x`` is not modified
    in place afterwards (call :meth:`refresh` if it was) and it keeps those tensors alive itself: another evaluation of
    the same model on other inputs may replace the layers' cache entries, the replay still reads valid memory.

    ``small_step`` (None = where it applies): small graphs run the forward as three launches behind one C-ABI call
    (small.SmallPlan) WITHOUT calling ``model.forward`` -- a model with forward hooks keeps the general path.

    The reference's second protocol (ACM-Geometric/train.py:86-92, data_utils.py:128-151): ``metric="rocauc"`` makes the
    per-set results ROC-AUCs (AF.eval_rocauc: scores, one ``torch.sort``, exact integer statistic; NaN where a set lacks a
    class) and ``criterion="bce"`` makes the loss on ``loss_set`` the BCE-with-logits against the one-hot labels (acm_bce_loss,
    loss only).  Still one synchronising copy per pass (float64 then: the AUCs are exact quotients of integers).  The sort is
    global, so row-sharded operators are refused with ``metric="rocauc"``.

    ``selector`` (a functional.SelectionState) with ``train_loss`` (the training step's fp32 loss scalar; the attribute may
    be re-pointed between un-captured passes): every pass ends by folding its epoch into the selector's device-resident
    state -- acm_select_step on (train_loss, result), then, if the selector keeps snapshots, acm_copy_if.  Needs three index
    sets (train, validation, test) and ``loss_set=1``.  A captured pass holds these launches at the tail of its graph (one
    linear chain: an epoch stays two graph replays); the selector is reset after the capture's warm-up passes, so
    :meth:`refresh` is refused once the run has begun."""

    def __init__(self, model, x, adj, labels, index_sets, adj_high=None, adj_un=None, loss_set=1, use_graph=False,
                 small_step=None, fused_metrics=True, metric="acc", criterion="nll", selector=None, train_loss=None):
        self.model, self.x, self.adj, self.adj_high, self.adj_un = model, x, adj, adj_high, adj_un
        self.metric, self.criterion = _checked(metric, METRICS, "metric"), _checked(criterion, CRITERIA, "criterion")
        if self.metric == "rocauc" and _is_sharded(adj):
            raise NotImplementedError('EvalStep(metric="rocauc"): the ROC-AUC sorts the scores of ALL rows; row-sharded '
                                      "operators are not supported")
        self.fused_metrics, self._metrics = bool(fused_metrics), None
        self._auc = None
        self.labels = labels
        self._labels_safe = labels.clamp_min(0)             # -1 = unlabeled (never in an index set)
        self.w, self.loss_set = _set_weights(index_sets, labels), int(loss_set)
        self.selector, self.train_loss = selector, train_loss
        if selector is not None and (self.w.shape[0] != 3 or self.loss_set != 1):
            raise ValueError("EvalStep(selector=...): needs the three index sets (train, validation, test) and loss_set=1")
        # small graphs: the evaluation forward as one call (small.SmallPlan without an optimizer)
        self.small, self.small_refused = None, "not requested"
        if small_step is not False:
            from .small import SmallPlan
            ops, xs = _operators_and_features(model, x, adj, adj_high, adj_un)
            self.small_refused = SmallPlan.why_not(model, xs, ops, None, need_dropout_state=False)
            if self.small_refused is None:
                self.small = SmallPlan(model, xs, ops)
        self.graph, self.out, self.res = None, None, None
        self._held = None
        self._use_graph = bool(use_graph)
        self._takes_call = _takes_call(model)
        # whether the last pass (the captured one, with use_graph) left the hidden activation unwritten, and why not
        self.hidden_elided, self.hidden_elided_refused = False, "no forward has run"
        if use_graph:
            self._capture()

    def refresh(self):
        """Re-capture after an in-place edit of the features (or of anything else the captured pass read once).

        With a ``selector`` only before the run's first epoch: the capture's warm-up passes fold epochs into the selector's
        state and the capture resets it, which in the middle of a run would wipe the epoch counter, the best key and the stop
        flag.  Refused (RuntimeError) once an epoch has been folded in; asking costs one small synchronising read."""
        if self._use_graph:
            if self.selector is not None and self.selector.poll()[0] > 0:
                raise RuntimeError("EvalStep.refresh(): the selector has folded epochs in; a re-capture would reset its state "
                                   "in the middle of the run")
            self.graph = None
            self._capture()

    @torch.no_grad()
    def _run(self):
        out, res = self._pass()
        if self.selector is not None:
            if self.train_loss is None:
                raise ValueError("EvalStep(selector=...): train_loss is not set")
            self.selector.launch(self.train_loss, res)
        return out, res

    def _pass(self):
        self.model.eval()
        if self.small is not None:
            out = self.small.run()                       # three launches, one C-ABI call (acm_small_step, train = 0)
        else:
            # (the context the model would make itself: here to read what the layers report into it)
            call = AF.CallContext.from_ambient() if self._takes_call else None
            out = _call_model(self.model, self._takes_call, (self.x, self.adj, self.adj_high, self.adj_un), call, ambient=False)
            if call is not None:
                _note_elision(self, call)
        if self.metric == "rocauc" or self.criterion == "bce":
            return out, self._second_protocol(out)
        if self._metrics_ok(out):
            # accuracy on every index set + the NLL on one of them as ONE launch over the logits (acm_eval_metrics, ABI 28)
            # instead of argmax / compare / log_softmax / gather / matmul / sum / cat (eight torch launches)
            return out, AF.eval_metrics(out, self.labels, self.w, self.loss_set, self._metrics_buffers(out))
        correct = (out.argmax(dim=1) == self.labels).to(torch.float32)
        return out, torch.cat([self.w @ correct, self._weighted_nll(out).view(1)])

    def _weighted_nll(self, out):
        """The NLL of the logits averaged over ``loss_set`` (its row of the averaging weights), in torch operations."""
        nll = -F.log_softmax(out, 1).gather(1, self._labels_safe.view(-1, 1)).view(-1)
        return (self.w[self.loss_set] * nll).sum()

    def _second_protocol(self, out):
        """[metric per index set ..., loss on ``loss_set``] in float64 for ``metric="rocauc"`` and / or ``criterion="bce"``:
        the library's launches (+ one torch.sort), no fallback."""
        if self.metric == "rocauc":
            if self._auc is None:
                self._auc = AF.rocauc_buffers(out.shape[0], self.w.shape[0], out.device)
            per_set = AF.eval_rocauc(out, self.labels, self.w, self._auc)
        else:
            per_set = (self.w @ (out.argmax(dim=1) == self.labels).to(torch.float32)).double()
        if self.criterion == "bce":
            loss = AF.bce_loss(out, self.labels, self.w[self.loss_set])
        else:
            loss = self._weighted_nll(out)
        return torch.cat([per_set, loss.double().view(1)])

    def _metrics_ok(self, out):
        return (self.fused_metrics and out.dim() == 2 and out.shape[1] <= 64 and 1 <= self.w.shape[0] <= 8
                and out.dtype == torch.float32 and out.stride(1) == 1 and self.labels.dtype == torch.int64
                and self.labels.dim() == 1 and self.labels.is_contiguous())

    def _metrics_buffers(self, out):
        """(result [k + 1], zero-initialised workspace) of acm_eval_metrics, made once per pass object: a captured pass bakes
        their addresses in."""
        if self._metrics is None:
            self._metrics = AF.eval_metrics_buffers(out.shape[0], self.w.shape[0], out.device)
        return self._metrics

    def _capture(self):
        _warm_up(self._run, 2)
        if self.selector is not None:
            self.selector.reset()               # the warm-up passes folded two epochs in
            torch.cuda.synchronize()
        self.graph, (self.out, self.res) = _captured(self._run)
        self._held = _held_entries(self.model)

    def launch(self):
        """Enqueue the pass on the current stream WITHOUT reading its result (``read()`` does): a loop that trains several
        models side by side (``fit_concurrent``) launches every model's pass before it waits for any."""
        if self.graph is not None:
            self.graph.replay()
            self._pending = (self.out, self.res)
        else:
            self._pending = self._run()

    def read(self):
        out, res = self._pending
        vals = res.tolist()                     # the one synchronising copy of the pass
        return out, vals[:-1], vals[-1]

    def __call__(self):
        self.launch()
        return self.read()


def fit(model, optimizer, x, adj, labels, train_idx, val_idx, test_idx, epochs, rule="max_val_acc",
        early_stopping=0, adj_high=None, adj_un=None, use_graph=False, fused_dropout=None, pipeline_input=None,
        criterion="nll", metric="acc", sync_every=1, keep_best=False):
    """Train and return (selected test accuracy, per-epoch history).

    ``sync_every`` / ``keep_best``: with the defaults (1, False) every epoch ends in a synchronising read of its numbers and
    the selection is done here on the host.  Otherwise the selection state lives on the device (functional.SelectionState:
    acm_select_step at the tail of the captured evaluation pass), up to ``sync_every`` epochs are enqueued back to back, and
    only then the host looks whether the run has stopped -- never more than ``epochs`` in total.  Needs ``use_graph=True``;
    row-sharded operators are refused.  Both returned values equal those of ``sync_every=1`` from the same initial state
    exactly (the window mean is the plain left-to-right float64 sum, ``sum()`` up to CPython 3.11; see DESIGN.md section 4a
    for the compensated ``sum()`` of later interpreters).  After an early stop the MODEL has taken up to ``sync_every - 1`` more optimizer steps than with
    ``sync_every=1``: the device state is frozen from the stopping epoch on, so the results do not see them.
    ``keep_best=True`` snapshots the parameters (and the model's fp32 buffers: BatchNorm running statistics) on the device whenever an epoch is selected (acm_copy_if, predicated on the
    selection: no cost in the other epochs, no extra read) and restores the selected epoch's parameters into ``model`` in
    place before returning -- the values after that epoch's optimizer step, which its evaluation pass saw.

    ``criterion`` / ``metric``: the reference's two protocols (ACM-Geometric/train.py:86-92): "nll" + "acc", or -- genius,
    twitch-e, yelp-chi, ``--rocauc`` -- "bce" + "rocauc".  With "rocauc" the three per-set numbers of a history row and the
    selected value are ROC-AUCs, ``rule="max_val_acc"`` selects on the validation AUC, and an undefined (NaN) AUC is never
    "best".  The validation loss follows the criterion.

    ``pipeline_input``: TrainStep's input pipeline (None = where the configuration qualifies, False = never).  On by
    default since round 3: with the sixteen-rows-per-wave backward kernel carrying the gather, an epoch (training step +
    evaluation pass, both captured) of the twitch-shaped graph takes 0.463 ms with it against 0.483 ms without
    (round 2, with the older kernel: 0.551 against 0.544, so it was off here).

    rule = "max_val_acc":  test accuracy at the best validation accuracy, fixed number of epochs
                           (ACM-Geometric/train.py:139-140, logger.py:17-48)
    rule = "min_val_loss": test accuracy at the lowest validation loss, stop when the validation loss
                           exceeds the mean of the last `early_stopping` epochs
                           (ACM-Pytorch/train.py:129-139)
    """
    resident = _resident_loop(sync_every, keep_best)
    if resident and not use_graph:
        raise ValueError("fit(sync_every > 1 or keep_best=True) needs use_graph=True: the selection launches ride the captured "
                         "evaluation pass")
    if resident and int(epochs) < 1:
        return 0.0, []
    run = _new_run(resident, use_graph, keep_best, model=model, optimizer=optimizer, x=x, adj=adj, labels=labels, train_idx=train_idx,
                   val_idx=val_idx, test_idx=test_idx, epochs=epochs, rule=rule, early_stopping=early_stopping, adj_high=adj_high,
                   adj_un=adj_un, fused_dropout=fused_dropout, pipeline_input=pipeline_input, criterion=criterion, metric=metric)
    # (without a budget the host-selected run has still built, and with use_graph captured, its step by now)
    return _drive(run, sync_every, done=int(epochs) < 1)


def _drive(run, sync_every, done=False):
    """The epoch loop of a ``_HostRun``, a ``_ResidentRun`` or ``_BatchedRuns`` on the current stream."""
    while not done:
        run.enqueue(sync_every)
        done = run.finished()
    return run.result()


def _new_run(resident, use_graph, keep_best, *, model, optimizer, x, adj, labels, train_idx, val_idx, test_idx, epochs, rule,
             early_stopping, adj_high, adj_un, fused_dropout, pipeline_input, criterion, metric):
    """One run of ``fit`` / ``fit_concurrent`` around what both kinds have: the training step and the evaluation pass's arguments
    (its own captured graph when the step is one).  The problem by keyword, every part of it: no call site counts positions."""
    _checked(metric, METRICS, "metric")
    if resident and _is_sharded(adj):
        raise NotImplementedError("fit(sync_every > 1 or keep_best=True): the selection state lives on ONE device; "
                                  "row-sharded operators are not supported")
    step = TrainStep(model, optimizer, x, adj, labels, row_weights(train_idx, x.shape[0], device=labels.device), adj_high, adj_un,
                     use_graph=use_graph or resident, fused_dropout=fused_dropout, pipeline_input=pipeline_input, criterion=criterion)
    eval_args = (model, x, adj, labels, (train_idx, val_idx, test_idx), adj_high, adj_un)         # EvalStep's and evaluate's
    if resident:
        return _ResidentRun(step, eval_args, metric, criterion, epochs, rule, early_stopping, keep_best)
    return _HostRun(step, eval_args, metric, criterion, epochs, rule, early_stopping, use_graph)


def _resident_loop(sync_every, keep_best):
    """Whether fit / fit_concurrent keep the selection state on the device (anything but the defaults)."""
    if int(sync_every) != sync_every or sync_every < 1:
        raise ValueError(f"sync_every must be an integer >= 1, not {sync_every!r}")
    return sync_every != 1 or bool(keep_best)


class _ResidentRun:
    """One run of ``fit`` with its selection state on the device: the captured training step, the captured evaluation pass
    whose graph ends in the selection launches, and how many epochs have been enqueued."""

    def __init__(self, step, eval_args, metric, criterion, epochs, rule, early_stopping, keep_best):
        self.step, self.model, self.epochs, self.enqueued = step, eval_args[0], int(epochs), 0
        model = self.model
        self.select = AF.SelectionState(rule, early_stopping, epochs, eval_args[3].device,
                                        params=list(model.parameters()) if keep_best else None,
                                        # (the running statistics of a deep mlpX stack's BatchNorms: the selected epoch's
                                        #  evaluation pass read them, so the returned model must hold them too)
                                        buffers=[b for b in model.buffers() if b.dtype == torch.float32] if keep_best else None)
        self.ev = EvalStep(*eval_args, loss_set=1, use_graph=True, metric=metric, criterion=criterion, selector=self.select,
                           train_loss=step.loss)

    def enqueue(self, sync_every):
        """Up to ``sync_every`` epochs (step replay + evaluation replay) on the current stream, within the budget."""
        for _ in range(min(int(sync_every), self.epochs - self.enqueued)):
            self.ev.train_loss = self.step()
            self.ev.launch()
            self.enqueued += 1

    def finished(self):
        """Waits for what was enqueued; True once the run has stopped or used its budget up."""
        _, stopped = self.select.poll()
        return stopped or self.enqueued >= self.epochs

    def result(self):
        selected, history, _ = self.select.result()
        if self.select.snapshot is not None:
            self.select.restore(self.model)
        return selected, history


class _HostRun:
    """One run of ``fit`` with the selection on the host, behind the three methods of ``_ResidentRun``: the training step, the
    captured evaluation pass (without ``use_graph`` an epoch is ``evaluate`` + ``_eager_val_loss``), the history and the
    selection.  The host loop's selection and early-stopping rule is stated once, in ``_fold``."""

    def __init__(self, step, eval_args, metric, criterion, epochs, rule, early_stopping, use_graph):
        self.step, self.eval_args, self.metric, self.criterion = step, eval_args, metric, criterion
        self.epochs, self.rule, self.early_stopping = epochs, rule, early_stopping
        self.best_key, self.selected, self.history, self.val_hist = None, 0.0, [], []
        self.ev = EvalStep(*eval_args, loss_set=1, use_graph=True, metric=metric, criterion=criterion) if use_graph else None

    def enqueue(self, sync_every):
        """One epoch (step + evaluation pass) on the current stream: this loop IS ``sync_every = 1``, whatever it is handed."""
        self.loss = self.step()
        if self.ev is not None:
            self.ev.launch()

    def finished(self):
        """The epoch's synchronising read (the pass's numbers, then the loss), folded in; True once the run has stopped or used
        its budget up."""
        if self.ev is not None:
            _, accs, val_loss = self.ev.read()
        else:
            out, accs = evaluate(*self.eval_args, metric=self.metric)
            (_, _, _, labels, (_, val_idx, _), _, _) = self.eval_args
            val_loss = _eager_val_loss(out, labels, val_idx, self.criterion)
        return self._fold(float(self.loss), accs, val_loss)

    def _fold(self, loss, accs, val_loss):
        """Append the epoch's row; "best so far" by ``_selection_key`` (strict ``>``); under "min_val_loss" stop when the
        validation loss exceeds the mean of the ``early_stopping`` epochs before it (``sum(...) / early_stopping``: see ``fit``)."""
        epoch, (acc_tr, acc_va, acc_te) = len(self.history), accs
        self.history.append((loss, acc_tr, acc_va, acc_te, val_loss))
        key = _selection_key(self.rule, acc_va, val_loss)
        if key is not None and (self.best_key is None or key > self.best_key):
            self.best_key, self.selected = key, acc_te
        stop, es = False, self.early_stopping
        if self.rule == "min_val_loss":
            self.val_hist.append(val_loss)
            stop = es > 0 and epoch > es and val_loss > sum(self.val_hist[epoch - es:epoch]) / es
        return stop or epoch + 1 >= self.epochs

    def result(self):
        return self.selected, self.history


def _run_on_streams(start, n_runs, streams, sync_every):
    """``start(k)`` builds run ``k`` (a ``_HostRun`` or a ``_ResidentRun``); at most ``streams`` of the ``n_runs`` are alive at a
    time, each on a stream of its own, and a finished run's stream goes to the next pending one.  Results in the order of k."""
    results, pending = [None] * n_runs, list(range(n_runs))
    slots = [None] * min(int(streams), n_runs)
    pool = [torch.cuda.Stream() for _ in slots]
    while pending or any(sl is not None for sl in slots):
        for i in range(len(slots)):
            if slots[i] is None and pending:
                k = pending.pop(0)
                with torch.cuda.stream(pool[i]):         # built and captured on the stream it will run on
                    slots[i] = k, start(k)
                pool[i].synchronize()
        live = [(i, sl) for i, sl in enumerate(slots) if sl is not None]
        for i, (k, run) in live:                         # every live run's epochs are enqueued before any result is awaited
            with torch.cuda.stream(pool[i]):
                run.enqueue(sync_every)
        for i, (k, run) in live:
            with torch.cuda.stream(pool[i]):
                if run.finished():
                    results[k] = run.result()
                    # keep_best: the restore was enqueued HERE, the caller reads elsewhere.  (A host-selected run's stream is
                    # already drained by its epoch's read: one call that waits for nothing.)
                    pool[i].synchronize()
                    slots[i] = None
    return results


def fit_concurrent(runs, x, adj, labels, epochs, rule="min_val_loss", early_stopping=0, adj_high=None, adj_un=None, streams=2,
                   fused_dropout=None, criterion="nll", metric="acc", sync_every=1, keep_best=False):
    """Several independent training runs on the same graph -- the reference's ten fixed splits, which ACM-Pytorch/train.py:49-139
    trains one after the other, each with a fresh model -- ``streams`` at a time, every run on its own stream with its own
    captured step and evaluation pass: the launches of one run fill the gaps of the other (a small-graph step is a chain of
    six short, latency-bound launches that leaves most of the chip idle).  Measured on the MI355X (scripts/probe_concurrent_splits.py):
    two runs side by side take 0.050 ms per step each on Cora (0.083 alone), 0.117 on Squirrel (0.159); more than two gain nothing.

    ``runs``: a list of ``(model, optimizer, train_idx, val_idx, test_idx)``; every run is exactly ``fit(..., use_graph=True)``
    of its model (same selection rules, same history rows, bit-identical results: the runs share no state but the read-only
    graph and features; ``criterion`` / ``metric`` as in ``fit``).  Returns ``[(selected test accuracy, history)]`` in the order of ``runs``.  Without a GPU stream to
    overlap on (CPU test double) the runs are trained one after the other.

    ``sync_every`` / ``keep_best`` as in ``fit``: a live run enqueues ``sync_every`` epochs on its stream before any run's
    state is looked at, and a run's stream is drained before its result is handed back (with ``keep_best`` the models hold the
    selected parameters on return, whatever stream the caller uses).  These need the captured graphs: the one-after-the-other
    path (``streams <= 1``) then calls ``fit(use_graph=True)``, so unlike the default path it does not run without a GPU
    (the CPU tests stub the capture)."""
    resident = _resident_loop(sync_every, keep_best)
    if resident and int(epochs) < 1:
        return [(0.0, []) for _ in runs]
    on_gpu = labels.is_cuda and torch.cuda.is_available()
    if not on_gpu or streams <= 1:
        return [fit(model, opt, x, adj, labels, tr, va, te, epochs, rule=rule, early_stopping=early_stopping, adj_high=adj_high,
                    adj_un=adj_un, use_graph=on_gpu or resident, fused_dropout=fused_dropout, criterion=criterion, metric=metric,
                    sync_every=sync_every, keep_best=keep_best) for model, opt, tr, va, te in runs]

    shared = dict(x=x, adj=adj, labels=labels, epochs=epochs, rule=rule, early_stopping=early_stopping, adj_high=adj_high,
                  adj_un=adj_un, fused_dropout=fused_dropout, pipeline_input=None, criterion=criterion, metric=metric)

    def start(k):
        model, opt, tr, va, te = runs[k]
        return _new_run(resident, True, keep_best, model=model, optimizer=opt, train_idx=tr, val_idx=va, test_idx=te, **shared)

    return _run_on_streams(start, len(runs), streams, sync_every)


# The smallest measured batch size within 3 % of the best one on the Squirrel-shaped workload (scripts/bench_batched_fit.py on
# the MI355X, profiles/batched_fit.jsonl; EXPERIMENTS.md "A batch of runs in the same six launches" has the table).
DEFAULT_BATCH = 8


def fit_batched(runs, x, adj, labels, epochs, rule="min_val_loss", early_stopping=0, batch=DEFAULT_BATCH, sync_every=32,
                fused_dropout=None, keep_best=False, criterion="nll", metric="acc"):
    """Several independent training runs on the same small graph -- the reference's ten splits (ACM-Pytorch/train.py:49-139),
    or the learning-rate x weight-decay x dropout grid of its hyperparameter_searching.py:51-70 -- ``batch`` at a time IN THE
    SAME LAUNCHES: one captured epoch graph holds the batched six-launch step (small.SmallBatch: grid row = run), the batched
    evaluation forward, the batched metrics and the batched selection, 11 launches per epoch whatever ``batch`` is (streams,
    ``fit_concurrent``, cannot remove launches; they saturate at two runs).

    ``runs``: ``[(model, optimizer, train_idx, val_idx, test_idx)]`` as in ``fit_concurrent``; per run the learning rate, betas,
    eps, weight decay, Adam or AdamW, dropout probability and dropout state may differ freely.  Returns ``[(selected,
    history)]`` in the order of ``runs``; each equals ``fit(..., use_graph=True, sync_every=sync_every)`` of that run alone,
    bit for bit (a grid row executes the single step's instructions in the single step's order).  The graph is replayed
    ``sync_every`` times, then ONE device-to-host copy reads every slot's selection state; runs that stopped or used their
    budget up hand their slot to the next pending run by table writes -- nothing is re-captured.  A stopped run's state is
    frozen on the device while its slot keeps stepping until that look (as with ``fit(sync_every > 1)``).

    ``batch``: slots (1 .. 32).  Default 8: the smallest measured size within 3 % of the best size on the Squirrel-shaped
    workload (scripts/bench_batched_fit.py, profiles/batched_fit.jsonl).

    Where ``SmallPlan.why_not`` or ``SmallBatch.why_not`` objects (a model outside the small-graph envelope -- hidden width 32
    or 64, <= 8 classes, ... --, runs that differ in configuration, a 32-wide and a 64-wide run among them) the call is ``fit_concurrent(..., sync_every=sync_every)`` and the reason is left in
    ``fit_batched.last_refusal`` (None otherwise).  ``keep_best=True``, ``criterion="bce"`` and ``metric="rocauc"`` are not
    implemented here: use ``fit_concurrent``."""
    if keep_best or criterion != "nll" or metric != "acc":
        raise NotImplementedError('fit_batched: keep_best=True, criterion="bce" and metric="rocauc" are not implemented for the '
                                  "batched loop; use fit_concurrent")
    _resident_loop(sync_every, False)
    batch = int(batch)
    if not 1 <= batch <= _lib.SMALL_BATCH_MAX:
        raise ValueError(f"fit_batched: batch must be 1 .. {_lib.SMALL_BATCH_MAX}, not {batch}")
    fit_batched.last_refusal = None
    if int(epochs) < 1 or not runs:
        return [(0.0, []) for _ in runs]
    # one operator set and one feature object for every run (TrainStep would build them per run: the plans must SHARE them).
    # This loop takes no adj_high / adj_un: an adjacency TENSOR is handed on as its own un-normalised twin, as it always was.
    ops, xs = (adj, x) if _is_sharded(adj) else _operators_and_features(runs[0][0], x, adj, None, adj)
    # every run against the envelope before anything is built: the fallback is decided here, not in the middle of the loop
    why, batched = _outside_batched_envelope(runs, xs, ops), None
    if why is None:
        batched = _BatchedRuns(runs, [(xs, ops, labels)] * len(runs), epochs, rule, early_stopping, min(batch, len(runs)), fused_dropout)
        why = batched.refused                         # (what only the built plans can tell)
    if why is not None:
        fit_batched.last_refusal = why
        return fit_concurrent(runs, x, adj, labels, epochs, rule=rule, early_stopping=early_stopping, fused_dropout=fused_dropout,
                              sync_every=sync_every)
    return _drive(batched, sync_every)


fit_batched.last_refusal = None


def fit_batched_graphs(runs, epochs, rule="min_val_loss", early_stopping=0, batch=DEFAULT_BATCH, sync_every=32, fused_dropout=None):
    """``fit_batched`` for runs on DIFFERENT graphs: the synthetic study (synthetic-experiments/train.py:64-164) trains on ten
    generated graphs per edge-homophily level, each with its own adjacency, its own features and its own split, times the
    models and a dropout x weight-decay grid.  ``runs``: ``[(model, optimizer, x, adj, labels, train_idx, val_idx, test_idx)]``;
    graphs of one row count, one input width, one class count and models of one configuration and hidden width share the
    launches (small.SmallGraphBatch: the launches are as wide as the widest graph's, every slot loops with its own widths).
    Runs that name the same ``x`` and ``adj`` objects share their operator set and features.

    Returns ``[(selected, history)]`` in the order of ``runs``; each equals ``fit(..., use_graph=True, sync_every=sync_every)``
    of that run alone, bit for bit.  The epoch loop, the hand-over of a slot and the capture are ``fit_batched``'s.  Where the
    runs cannot share launches the call is ``fit`` run by run and the reason is left in ``fit_batched_graphs.last_refusal``
    (None otherwise).  ``keep_best``, ``criterion="bce"`` and ``metric="rocauc"`` are not implemented here: use ``fit``."""
    _resident_loop(sync_every, False)
    batch = int(batch)
    if not 1 <= batch <= _lib.SMALL_BATCH_MAX:
        raise ValueError(f"fit_batched_graphs: batch must be 1 .. {_lib.SMALL_BATCH_MAX}, not {batch}")
    fit_batched_graphs.last_refusal = None
    if int(epochs) < 1 or not runs:
        return [(0.0, []) for _ in runs]
    made, inputs = {}, []
    for model, _, x, adj, labels, _, _, _ in runs:
        key = (id(x), id(adj))
        if key not in made:                           # one operator set and one feature object per graph, as in fit_batched
            ops, xs = (adj, x) if _is_sharded(adj) else _operators_and_features(model, x, adj, None, adj)
            made[key] = (xs, ops)
        inputs.append(made[key] + (labels,))
    own = [(model, opt, tr, va, te) for model, opt, _, _, _, tr, va, te in runs]
    # every run against the envelope before anything is built, as in fit_batched
    why, batched = _outside_graphs_envelope(own, inputs), None
    if why is None:
        batched = _BatchedRuns(own, inputs, epochs, rule, early_stopping, min(batch, len(runs)), fused_dropout, graphs=True)
        why = batched.refused
    if why is not None:
        fit_batched_graphs.last_refusal = why
        return [fit(model, opt, x, adj, labels, tr, va, te, epochs, rule=rule, early_stopping=early_stopping, use_graph=True,
                    fused_dropout=fused_dropout, sync_every=sync_every) for model, opt, x, adj, labels, tr, va, te in runs]
    return _drive(batched, sync_every)


fit_batched_graphs.last_refusal = None


def _outside_batched_envelope(runs, xs, ops):
    """Why ``fit_batched`` cannot train ``runs`` in the same launches (it then calls ``fit_concurrent``), or None: every run
    inside the fused small-graph step's envelope, all of them configured alike."""
    if _is_sharded(ops):
        return "row-sharded operators"
    return _outside_graphs_envelope(runs, [(xs, ops, None)] * len(runs))


def _outside_graphs_envelope(runs, inputs):
    """``_outside_batched_envelope`` with run k on ``inputs[k]`` = (features, operators, labels): every run inside the fused
    small-graph step's envelope on ITS graph, all models configured alike, all graphs of one row count and one input width."""
    from .small import SmallPlan
    shape0 = None
    for k, ((model, opt, _, _, _), (xs, ops, _)) in enumerate(zip(runs, inputs)):
        why = "row-sharded operators" if _is_sharded(ops) else SmallPlan.why_not(model, xs, ops, opt, need_dropout_state=False)
        if why is None:
            cfg = model.gcns[0]._config()
            shape = (cfg.n_channels, cfg.relu_before, cfg.layernorm, cfg.scale, model.gcns[1].out_features, model.gcns[0].out_features)
            size = (ops.low.n_rows, xs.shape[1])
            shape0, size0 = (shape, size) if shape0 is None else (shape0, size0)
            if shape != shape0:
                why = "the models are configured differently"
                if shape[-1] != shape0[-1]:
                    why = f"hidden width {shape[-1]} (run 0: {shape0[-1]}): {why}"
            elif size[0] != size0[0]:
                why = f"a graph of {size[0]} rows (run 0: {size0[0]}): one row count per batch"
            elif size[1] != size0[1]:
                why = f"{size[1]} input features (run 0: {size0[1]})"
        if why is not None:
            return f"run {k}: {why}"
    return None


class _BatchedRuns:
    """The runs of ``fit_batched`` / ``fit_batched_graphs`` behind the three methods of a run (``_drive``): the two batches
    (training step, evaluation forward), the batched metrics and selection, the runs that hold a slot and those still waiting
    for one.  ``runs[k]`` = (model, optimizer, train_idx, val_idx, test_idx) trains on ``inputs[k]`` = (features, operators,
    labels): the same triple for every run (``small.SmallBatch``), or -- ``graphs`` -- a graph per run
    (``small.SmallGraphBatch``, whose launch widths are formed here from the handles of EVERY run, before the capture).  Built
    and, on the GPU, captured on construction -- unless the first runs' plans cannot share launches: ``refused`` says why."""

    def __init__(self, runs, inputs, epochs, rule, early_stopping, n_slots, fused_dropout, graphs=False):
        from .small import SmallBatch, SmallGraphBatch
        self.runs, self.inputs, self.fused_dropout, self.epochs = runs, inputs, fused_dropout, int(epochs)
        self.name, self.Batch = ("fit_batched_graphs", SmallGraphBatch) if graphs else ("fit_batched", SmallBatch)
        self.pending, self.results = list(range(len(runs))), [None] * len(runs)
        self.live = first = [self._enter() for _ in range(n_slots)]
        Batch = self.Batch
        self.refused = next((r.refused for r in first if r.refused), None) or Batch.why_not([r.step.small for r in first]) \
            or Batch.why_not([r.ev.small for r in first])
        if self.refused is not None:
            return
        if graphs:
            seen = {(id(xs), id(ops)): (xs, ops) for xs, ops, _ in inputs}.values()          # (a graph's handles once)
            self.train_b = Batch([r.step.small for r in first], n_slots, handles=[Batch.handles_of(xs, ops, True) for xs, ops in seen])
            self.eval_b = Batch([r.ev.small for r in first], n_slots, handles=[Batch.handles_of(xs, ops, False) for xs, ops in seen])
        else:
            self.train_b = Batch([r.step.small for r in first], n_slots)
            self.eval_b = Batch([r.ev.small for r in first], n_slots)
        n, n_classes, labels = first[0].step.small.n, first[0].step.small.C, inputs[0][2]
        self.metrics = AF.BatchMetrics(n_slots, n, n_classes, 3, first[0].ev.labels, loss_set=1)
        self.select = AF.BatchSelection(rule, early_stopping, epochs, n_slots, labels.device)
        for i, r in enumerate(first):
            self._bind_slot(i, r)
        self.metrics.flush(), self.select.flush()
        self.train_b.bind(), self.eval_b.bind()
        self.replay = self._epoch                     # (without a GPU there is nothing to capture: an epoch is its launches)
        if labels.is_cuda:
            # as TrainStep._capture: warm up on a snapshot of every run in a slot, put it back, then capture -- no run sees the
            # warm-up steps; the selection states are reset (the warm-up folded epochs in)
            snaps = [r.step._snapshot() for r in first]
            _warm_up(self._epoch, 3)
            for r, snap in zip(first, snaps):
                r.step._restore(snap)
            for i in range(n_slots):
                self.select.reset(i)
            torch.cuda.synchronize()
            # No ``_held_entries`` beside this graph: it reads none.  Neither SmallBatch calls ``model.forward`` -- the launches
            # work on the plans' own buffers, the batched metrics and selection on theirs -- so no layer's P is ever looked up.
            self.replay = _captured(self._epoch)[0].replay

    def _enter(self):
        """The next waiting run for a slot, with its (un-captured) training step and evaluation pass objects -- made exactly as
        ``fit`` makes them, so the run's plans, optimizer state and dropout state are what ``fit`` would train."""
        k, fused_dropout = self.pending.pop(0), self.fused_dropout
        (model, opt, tr, va, te), (xs, ops, labels) = self.runs[k], self.inputs[k]
        step = TrainStep(model, opt, xs, ops, labels, row_weights(tr, xs.shape[0], device=labels.device), use_graph=False,
                         fused_dropout=fused_dropout)
        ev = EvalStep(model, xs, ops, labels, (tr, va, te), loss_set=1, use_graph=False)
        return SimpleNamespace(k=k, model=model, enqueued=0, step=step, ev=ev, refused=step.small_refused or ev.small_refused)

    def _bind_slot(self, i, r):
        """Slot ``i`` of the metrics and the selection reads run ``r``'s logits and loss (None: the slot idles)."""
        if r is None:
            self.metrics.set_slot(i)
            self.select.set_slot(i)
        else:
            self.metrics.set_slot(i, r.ev.small.logits, r.ev.w, r.ev.labels)
            self.select.set_slot(i, r.step.small.loss, self.metrics.out[i])

    def _epoch(self):
        self.train_b.run()
        self.eval_b.run()
        self.metrics.launch()
        self.select.launch()

    def _hand_over(self, i):
        """Slot ``i``'s run has stopped or used its budget up: its result is read, the slot goes to the next waiting run (or
        idles) by table writes -- nothing is re-captured."""
        Batch = self.Batch
        r = self.live[i]
        selected, history, _ = self.select.result(i)
        self.results[r.k] = (selected, history)
        r.model.eval()
        nxt = self.live[i] = self._enter() if self.pending else None
        if nxt is not None:
            why = nxt.refused or Batch.why_not([self.train_b._first(), nxt.step.small]) \
                or Batch.why_not([self.eval_b._first(), nxt.ev.small])
            if why is not None:
                raise RuntimeError(f"{self.name}: run {nxt.k} cannot share the launches of the runs before it ({why}); "
                                   "sort such runs into calls of their own")
        self.train_b.set_slot(i, nxt.step.small if nxt is not None else None)
        self.eval_b.set_slot(i, nxt.ev.small if nxt is not None else None)
        self._bind_slot(i, nxt)

    def enqueue(self, sync_every):
        """Up to ``sync_every`` epochs of every slot (one graph replay each), within the largest budget left among them."""
        live = [r for r in self.live if r is not None]
        todo = min(int(sync_every), max(self.epochs - r.enqueued for r in live))
        for _ in range(todo):
            self.replay()
        for r in live:
            r.enqueued += todo
            r.step._counter_moved(todo, by="plan")

    def finished(self):
        """The look: ONE synchronising copy reads every slot's selection state; runs that are through hand their slots over.
        True once no slot holds a run."""
        state = self.select.poll()
        leaving = [i for i, r in enumerate(self.live) if r is not None and (state[i][1] or r.enqueued >= self.epochs)]
        for i in leaving:
            self._hand_over(i)
        if leaving:
            self.metrics.flush(), self.select.flush()
        return all(r is None for r in self.live)

    def result(self):
        return self.results
