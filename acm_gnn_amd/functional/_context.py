"""What lives for one training step or one model call beside the tensors: the deferred second phases, the CallContext
handed down a forward, the calling thread's ambient context and Tape (``_TLS``: read and written in this module only), the
``with`` blocks that set them and the input pipeline."""
import bisect
import ctypes as C
import threading

import torch

from .. import _lib, tuning
from ._launch import _F32, _Timed, _vp, launch


class DeferredReductions:
    """The pending second phases (acm_reduce_list_t) of the calls made while this object is current: the loss sum and
    the parameter-gradient sums of K3 / acm_proj_bwd / acm_conv_agg_bwd.  Until :meth:`flush` their outputs (the
    loss, every ``.grad`` those kernels produce) are UNDEFINED, so only a loop that owns the whole step may defer
    (``train.TrainStep`` does: nothing reads a gradient between ``backward`` and the flush it issues before the
    optimizer / the gradient all-reduce).  One launch instead of four per step (~5 us each in a replayed graph)."""
    CAP = 96

    def __init__(self):
        self._segs = (_lib.ReduceSeg * self.CAP)()
        self._list = _lib.ReduceList(0, self.CAP, C.cast(self._segs, C.POINTER(_lib.ReduceSeg)))
        self._keep = []                 # workspaces the pending segments read
        self.outputs = []               # (data_ptr, nbytes) of tensors whose content arrives with the flush
        self._allreduce = []            # (tensor, group): row-shard gradient sums to all-reduce right after the flush

    def pointer(self):
        return C.addressof(self._list)

    def hold(self, workspace, outputs, keep=None):
        """A deferred call's workspace, the tensors its second phase will write (`outputs`: address ranges for
        all_adopted) and what must stay allocated for that write (`keep`, default the outputs themselves; pass the
        base buffer when the outputs are views autograd should still be able to adopt -- a held view has one
        reference too many for that)."""
        self._keep.append(workspace)
        self._keep.extend(outputs if keep is None else keep)
        self.outputs.extend((t.data_ptr(), t.numel() * t.element_size()) for t in outputs if t is not None)

    @property
    def pending(self):
        return int(self._list.n)

    def all_adopted(self, tensors):
        """True if every output of a deferred call is (the storage of) at least one of `tensors` -- e.g. the loss and
        the ``.grad`` of every parameter: autograd adopted what the kernels wrote instead of copying or accumulating
        it before the flush."""
        ptrs = sorted(t.data_ptr() for t in tensors if t is not None)
        for a, nb in self.outputs:
            i = bisect.bisect_left(ptrs, a)
            if i == len(ptrs) or ptrs[i] >= a + nb:
                return False
        return True

    def allreduce(self, tensor, group):
        """Row-sharded runs: `tensor` holds this rank's partial sums of replicated-parameter gradients, complete only
        after the flush.  Instead of flushing and all-reducing at every layer's backward, the tensors are collected and
        summed over the ranks right after the ONE flush of the step -- as one coalesced collective where the backend
        offers it (RCCL), one after the other otherwise."""
        self._allreduce.append((tensor, group))

    def flush(self):
        if self._list.n:
            launch("acm_reduce_flush", "reduce_flush", self._keep[0].device, C.byref(self._list))
        if self._allreduce:
            import torch.distributed as dist
            pending, self._allreduce = self._allreduce, []
            group = pending[0][1]
            coalesce = (len(pending) > 1 and all(g is group for _, g in pending) and hasattr(dist, "_coalescing_manager")
                        and dist.get_backend(group) == "nccl")
            with _Timed("all_reduce/gradients", sum(t.numel() * t.element_size() for t, _ in pending)):
                if coalesce:
                    with dist._coalescing_manager(group=group, device=pending[0][0].device, async_ops=False):
                        for t, _ in pending:
                            dist.all_reduce(t, group=group)
                else:
                    for t, g in pending:
                        dist.all_reduce(t, group=g)
        self._keep.clear()

    @property
    def collectives_pending(self):
        return bool(self._allreduce)

    def flushed(self):
        """The list was flushed by someone else (acm_adam_step with acm_adam_config_t.pending): release what it held."""
        assert self._list.n == 0 and not self._allreduce
        self._keep.clear()

    def discard(self):
        self._list.n = 0
        self._keep.clear()
        self._allreduce = []


def _sum_over_ranks(flat, group, defer):
    """All-reduce ``flat`` (row-shard partial sums of replicated parameters' gradients) over ``group``: now, or under a
    deferral list after the step's single flush, whose second phases write those partials."""
    if defer is not None:
        defer.allreduce(flat, group)
    else:
        import torch.distributed as dist
        dist.all_reduce(flat, group=group)


class CallContext:
    """What a caller hands DOWN one forward (and, captured by the autograd Functions, its backward) beside the tensors:

    * ``defer``     a DeferredReductions the second phases of the call's kernels are appended to (or None: reduce at once)
    * ``tail``      a pending fused_loss_tail request for the model's output layer
    * ``pipe``      the training loop's InputPipeline
    * ``link``      the HiddenLink (_hidden.py) between the hidden layer and the layer after it, while the model runs the two
    * ``elision``   what the last aggregate-first hidden layer did with its output: (left unwritten?, the reason if not)

    A context belongs to ONE model call: models.GCN / layers.GraphConvolution take it as ``call=`` (train.TrainStep passes
    its own) or derive a fresh one from the thread's ambient context -- what ``with deferred_reductions()`` /
    ``with fused_loss_tail()`` blocks of the calling thread have set.  Nothing lives in module globals: two models, two
    threads or an exception between two layers cannot see each other's hand-offs, and a backward (which autograd may run on
    another thread) uses the context its forward captured."""
    __slots__ = ("defer", "tail", "pipe", "link", "elision", "grad_enabled")

    def __init__(self, defer=None, tail=None, pipe=None):
        self.defer, self.tail, self.pipe = defer, tail, pipe
        self.link = self.elision = None
        self.grad_enabled = True         # torch.is_grad_enabled() where the layer was called (acm_conv notes it: inside a
                                         # Function's forward it is always off); True = a backward may follow

    @classmethod
    def from_ambient(cls):
        a = _ambient()
        return cls(a.defer, a.tail, a.pipe)

    def defer_ptr(self):
        return self.defer.pointer() if self.defer is not None else None


_TLS = threading.local()


def _ambient():
    """The calling thread's ambient context (created on first use)."""
    c = getattr(_TLS, "call", None)
    if c is None:
        c = _TLS.call = CallContext()
    return c


def _call_or_ambient(call):
    return call if call is not None else CallContext.from_ambient()


class TapeBroken(RuntimeError):
    """A step cannot run on a Tape (see there): something other than this package's Functions sits between them."""


class _TapeCtx:
    """What a Function's forward / backward see in place of autograd's ctx when the call runs on a Tape."""

    def __init__(self, needs_input_grad):
        self.needs_input_grad = needs_input_grad
        self.saved_tensors = ()
        self.non_differentiable = ()

    def save_for_backward(self, *tensors):
        self.saved_tensors = tensors

    def mark_non_differentiable(self, *tensors):
        # (the mixing weights ``att``: Tape.run neither tags them nor gives them requires_grad -- a layer that keeps its
        # ``att`` around must not keep the step's saved activations alive with it)
        self.non_differentiable = tuple(id(t) for t in tensors)

    def release(self):
        """Drop everything the record holds (saved activations, hand-offs parked on the ctx by the Functions)."""
        self.__dict__.clear()
        self.saved_tensors = ()

    def set_materialize_grads(self, value):
        pass                                  # (Tape.backward hands None to outputs without a gradient, as the Functions ask)


class Tape:
    """The training step's own record of the Functions it runs, replayed backwards by ``backward`` -- instead of an autograd
    graph (train.TrainStep, eager steps).  A two-layer step is two or three of this package's Functions in a row with 26
    parameters: autograd spends more host time on them (``Function.apply``, 26 AccumulateGrad nodes, gradient validation,
    the engine's thread hand-off: ~0.3 ms) than the kernels take.  The tape calls ``forward(ctx, *args)`` under no_grad,
    remembers (Function, ctx, args, outputs), and ``backward(out, grad)`` walks the records in reverse: output gradients
    by tensor identity, parameter gradients assigned (added, when a parameter is used twice) to ``.grad``.

    It is only sound while every tensor that carries a gradient between two records is the very object a record returned:
    outputs are marked ``requires_grad`` so that a torch op in between leaves a ``grad_fn`` on its result, and such an argument
    (or a final output the tape did not produce) raises TapeBroken -- the step then runs on autograd, for good."""

    def __init__(self):
        self.records = []
        self.produced = {}                    # id(tensor) -> tensor (kept alive: an id must not be handed to another object)

    def run(self, fn, args):
        needs = []
        for a in args:
            if not isinstance(a, torch.Tensor):
                needs.append(False)
            elif id(a) in self.produced:
                needs.append(True)
            elif a.grad_fn is not None:
                raise TapeBroken(f"{fn.__name__}: an argument was computed by torch operations from tensors that need gradients")
            else:
                needs.append(bool(a.requires_grad))          # a parameter, or a constant (features, a mask tensor)
        ctx = _TapeCtx(tuple(needs))
        with torch.no_grad():
            out = fn.forward(ctx, *args)
        outs = out if isinstance(out, tuple) else (out,)
        if not any(needs):                        # as under autograd: nothing to differentiate, the outputs are constants
            return out                            # (the dropped copy of the input features)
        for o in outs:
            if isinstance(o, torch.Tensor) and o.is_floating_point() and id(o) not in ctx.non_differentiable:
                o.requires_grad_(True)
                self.produced[id(o)] = o
        self.records.append((fn, ctx, args, outs))
        return out

    def release(self):
        """End of the step (or of the attempt): every record lets go of what it saved."""
        for _, ctx, _, _ in self.records:
            ctx.release()
        self.records, self.produced = [], {}

    def backward(self, out, grad):
        if id(out) not in self.produced:
            raise TapeBroken("the model's output is not the output of one of this package's Functions")
        grads = {id(out): grad}
        try:
            self._backward(grads)
        finally:
            self.release()

    def _backward(self, grads):
        with torch.no_grad():
            for fn, ctx, args, outs in reversed(self.records):
                gouts = tuple(grads.pop(id(o), None) if isinstance(o, torch.Tensor) else None for o in outs)
                if all(g is None for g in gouts):
                    continue
                gins = fn.backward(ctx, *gouts)
                if not isinstance(gins, tuple):
                    gins = (gins,)
                for a, g in zip(args, gins):
                    if g is None or not isinstance(a, torch.Tensor):
                        continue
                    if id(a) in self.produced:
                        grads[id(a)] = g if id(a) not in grads else grads[id(a)] + g
                    elif a.requires_grad:
                        if g.stride() != a.stride():          # AccumulateGrad's layout contract: a strided view is copied (a
                            g = g.contiguous()                # deferred output copied too early fails the step's all_adopted check)
                        if a.grad is None:
                            a.grad = g
                        else:
                            a.grad.add_(g)                    # (in place, as AccumulateGrad does without a graph)


class on_tape:
    """``with on_tape(tape): out = model(...)`` -- the Functions the calling thread runs inside go to ``tape``."""

    def __init__(self, tape):
        self.tape = tape

    def __enter__(self):
        self.prev = _current_tape()
        _TLS.tape = self.tape
        return self.tape

    def __exit__(self, *exc):
        _TLS.tape = self.prev
        return False


def _current_tape():
    """The Tape the calling thread's Functions go to (``with on_tape(...)``), or None: autograd."""
    return getattr(_TLS, "tape", None)


def _run(fn, *args):
    """``fn.apply(*args)``, or the same call on the calling thread's Tape."""
    tape = _current_tape()
    return fn.apply(*args) if tape is None else tape.run(fn, args)


class deferred_reductions:
    """``with deferred_reductions() as d: ...; d.flush()`` -- the calls the thread makes inside (and the backward of what
    it ran forward inside) append their second phases to ``d``.  Leaving the block flushes whatever is still pending (or
    drops it when an exception is propagating)."""

    def __enter__(self):
        a = _ambient()
        self.prev, self.d = a.defer, DeferredReductions()
        a.defer = self.d
        return self.d

    def __exit__(self, exc_type, *rest):
        _ambient().defer = self.prev
        if exc_type is None:
            self.d.flush()
        else:
            self.d.discard()
        return False


class deferred_reductions_as:
    """``with deferred_reductions_as(d): ...`` -- make an existing DeferredReductions (or None) the thread's ambient one;
    the caller keeps the responsibility to flush or discard it."""

    def __init__(self, d):
        self.d = d

    def __enter__(self):
        a = _ambient()
        self.prev, a.defer = a.defer, self.d
        return self.d

    def __exit__(self, *exc):
        _ambient().defer = self.prev
        return False


class fused_loss_tail:
    """``with fused_loss_tail(labels, row_weight) as tail: out = model(...)`` -- a request to the model's OUTPUT layer
    (a narrow three-channel ACM layer called with ``output_layer`` set and no post-op) to run its row phase, the
    masked NLL of its logits and its own row-local backward (K3) as ONE kernel (acm_conv_fwd_tail).  Afterwards
    ``tail.matches(out)`` says whether ``out`` is that layer's output; if so ``tail.loss`` / ``tail.dz`` are what
    nll_loss_and_grad(out, labels, row_weight) returns, and ``out.backward(tail.dz)`` skips K3.  Any other gradient
    handed to that layer's backward makes it run K3 as usual, so a request that is not honoured costs nothing but time.

    ``loss_rows`` (a graph.LossRows of the operators the model is called with, built for THIS ``row_weight``; default None:
    the full path): the layer may then take acm_conv_fwd_tail_rows.  The loss,
    ``dz`` and every gradient keep their bits; but the rows of ``out`` (and of the layer's ``att``) whose weight is 0 are
    then ZEROS, not logits -- for a caller that reads the loss alone (train.TrainStep).  ``tail.used_loss_rows`` says
    whether the layer took it."""

    def __init__(self, labels, row_weight, loss_rows=None):
        self.labels, self.row_weight, self.loss_rows = labels, row_weight, loss_rows
        self.used_loss_rows = False
        self.loss = self.dz = self.out = None

    def __enter__(self):
        a = _ambient()
        self.prev = a.tail
        a.tail = self
        return self

    def __exit__(self, *exc):
        _ambient().tail = self.prev
        return False

    def matches(self, out):
        return self.out is not None and out is not None and out.data_ptr() == self.out.data_ptr() \
            and out.shape == self.out.shape


class input_pipeline:
    """``with input_pipeline(pipe): ...`` -- the thread's model calls inside see the training loop's InputPipeline."""

    def __init__(self, pipe):
        self.pipe = pipe

    def __enter__(self):
        a = _ambient()
        self.prev = a.pipe
        a.pipe = self.pipe
        return self.pipe

    def __exit__(self, *exc):
        _ambient().pipe = self.prev
        return False


class InputPipeline:
    """The first layer's input aggregation P_t = A_low dropout_t(x), computed one optimizer step AHEAD inside the layer's
    own backward.  x is constant and the mask of step t + 1 is a function of the step counter (acm_dropout_t.step_offset),
    so P_{t+1} depends on nothing step t computes; the row-local backward kernel of the aggregate-first layer is bound
    by its vector instructions and leaves the memory system idle, the narrow gather is bound by memory latency -- in one
    kernel (two extra waves per workgroup) they overlap, as two kernels they do not.

    Buffers (fixed addresses: a captured graph keeps them): ``filled`` = [dropout(x) padded to 8 columns | P] for the step
    about to run, ``saved`` = the copy of both that the forward's row-local kernel leaves for the backward
    (acm_conv_agg_fwd_t.agg_copy / xs_copy: it reads those rows anyway).  A step runs
    forward (reads filled, writes saved) -> make_next() (filled table <- dropout_{t+1}(x)) -> backward (reads saved;
    its gather waves read the filled table and write the filled P) -> optimizer -> end_step().
    prime() fills ``filled`` for the current counter value; it must be called again whenever the counter is set from
    outside (train.TrainStep does after its warm-up) or x is modified in place (``stale()`` notices the latter between
    eager steps; a captured graph replays without host code, so there the caller has to)."""

    def __init__(self, ops, x, p, state, tag=0):
        # Row-sharded with equal blocks and the replicated input registered (ops.x_full): every rank draws the dropped
        # input of ALL nodes itself (the mask is a function of the global position), so the table has every node's row,
        # P and the saved copies this rank's rows only, and the carried gather needs no exchange -- N ranks run the same
        # step as one.
        self.x_rows = x                                   # the rows the caller hands the model
        src = ops.x_full if getattr(ops, "sharded", False) else x
        n_tab, n = src.shape[0], x.shape[0]
        self.row_offset = int(getattr(ops, "row_offset", 0)) if getattr(ops, "sharded", False) else 0
        self.ops, self.x, self.p, self.state, self.tag = ops, src, float(p), state, int(tag)
        if n_tab == n:
            both = torch.zeros(2, n, 8, dtype=_F32, device=x.device)
            self.filled = (both[0], both[1])
        else:
            self.filled = (torch.zeros(n_tab, 8, dtype=_F32, device=x.device), torch.zeros(n, 8, dtype=_F32, device=x.device))
        self.saved = torch.zeros(2, n, 8, dtype=_F32, device=x.device)
        self.primed = False
        self._x_version = (src._version, x._version)
        self._host_steps = state.host_steps
        self.next_table_ready = False
        self.next_agg_ready = False
        self.adopted = False             # set by the forward that took P from this pipeline (and left its copies in ``saved``)

    @staticmethod
    def eligible(model, ops, x):
        """Conditions under which train.TrainStep pipelines: the twitch-class configuration -- a dense input of 5..8
        features into a three-channel ACM layer of width 64, one device, pattern-only operator, counter-based dropout."""
        from ..graph import FilterOperators
        if tuning.HOST.pipeline <= 0 or not isinstance(ops, FilterOperators) or not isinstance(x, torch.Tensor):
            return False
        if getattr(model, "model_type", None) not in ("acmgcn", "acmgcnp", "acmgcnpp"):
            return False
        if model.model_type == "acmgcnpp":       # the residual Linear reads the table too: its fused form only (it then takes
            lins = getattr(getattr(model, "mlpX", None), "lins", None)          # this step's rows from ``saved`` in its backward)
            if lins is None or len(lins) != 1 or lins[0].out_features > 256:
                return False
        gcns = getattr(model, "gcns", None)
        if not gcns or len(gcns) != 2 or not getattr(model, "fused_dropout", False) or getattr(model, "dropout", 0) <= 0:
            return False
        l0 = gcns[0]
        try:
            cfg = l0._config()
            f_in, f = l0.weight_low.shape
        except AttributeError:
            return False
        if cfg.relu_before or f != 64 or not 4 < f_in <= 8 or x.dim() != 2 or x.shape[1] != f_in:
            return False
        if not ops.implicit or getattr(ops, "general", False) or int(getattr(ops, "hops", 1)) != 1:
            return False
        if ops.sharded:                          # equal blocks + the replicated input: the table is drawn locally (no halo)
            xf = ops.x_full
            if (not ops.uniform or xf is None or xf.dtype != _F32 or xf.dim() != 2 or xf.shape != (ops.low.n_cols, f_in)
                    or xf.device != x.device or xf.requires_grad):
                return False
        if x.dtype != _F32 or x.device != l0.weight_low.device or x.requires_grad:
            return False
        n, nnz = ops.low.n_rows, ops.low.nnz
        min_rows = tuning.HOST.pipeline                                             # below (8192): launch-bound, nothing to hide
        if n != x.shape[0] or n < max(min_rows, 32) or not 12.0 * n < nnz <= 160.0 * n:    # the regime of the fused forward
            return False
        if x.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            return False
        # four gather waves per workgroup of the backward, one workgroup per 16 rows at most (its workspace), 256 at most
        gw = 4                                                                      # gather waves per workgroup
        if not ops.low.build_streams(n_waves=max(gw, min(256 * gw, gw * ((n + 15) // 16)))):
            return False
        return ops.low.stream_waves % gw == 0 and gw <= ops.low.stream_waves <= min(256 * gw, gw * ((n + 15) // 16))

    def table(self):
        """dropout_t(x) of every node the operator's columns name, padded to 8 columns."""
        return self.filled[0]

    def local_table(self):
        """This rank's rows of table() (all of it on one device)."""
        return self.filled[0][self.row_offset:self.row_offset + self.x_rows.shape[0]]

    def agg(self):
        return self.filled[1]

    def _drop_into(self, dst, step_offset):
        d = self.state.spec(self.p, self.tag, 0)
        d.step_offset = int(step_offset)
        n, c = self.x.shape
        launch("acm_dropout", f"dropout/{n}x{c}", self.x.device, n, c, _vp(self.x), self.x.stride(0), _vp(dst), dst.stride(0), 8, C.byref(d))

    def stale(self):
        """The buffers do not belong to the step about to run: never filled, the features edited in place, a step that
        did not finish (exception between make_next and end_step), or the counter advanced by someone else."""
        return (not self.primed or (self.x._version, self.x_rows._version) != self._x_version or self.next_table_ready
                or self.state.host_steps != self._host_steps)

    def prime(self):
        from .ops import spmm                             # (late: ops imports this module)
        self._drop_into(self.filled[0], 0)
        spmm(self.ops.low, self.filled[0], out=self.filled[1], row_scale=self.ops.row_scale)
        self.primed = True
        self._x_version = (self.x._version, self.x_rows._version)
        self._host_steps = self.state.host_steps
        self.next_table_ready = self.next_agg_ready = self.adopted = False

    def refill_spec(self, p):
        """Ask the forward's row-local kernel (acm_conv_agg_fwd_t.next_x / next_drop) to write the NEXT step's dropped input
        over the table rows it reads -- possible where the table holds exactly the rows the layer works on (one device)."""
        if self.filled[0].shape[0] != self.x_rows.shape[0] or self.next_table_ready or self.x.stride(1) != 1:
            return False
        d = self.state.spec(self.p, self.tag, 0)
        d.step_offset = 1
        p.next_x, p.ld_next_x, p.next_drop = self.x.data_ptr(), self.x.stride(0), d
        return True

    def make_next(self):
        """Between the forward and the backward: the next step's dropped input replaces this step's -- only if the forward
        took this step's from the pipeline and left its copies in ``saved`` (``adopted``); a forward that went another way
        (a tuning switch, another path of the layer) may have saved the table itself for its backward.  (Drawing the
        table on a side stream right behind the first layer's forward was built and measured slower on one device:
        DESIGN.md section 9b.)"""
        if not self.adopted:
            return False
        if not self.next_table_ready:
            self._drop_into(self.filled[0], 1)
            self.next_table_ready = True
        return True

    def end_step(self):
        """After the optimizer step (which advanced the counter).  If the layer's backward did not carry the gather (it
        fell back to another path), ``filled`` is stale: prime() again before the next forward."""
        if not (self.next_table_ready and self.next_agg_ready):
            self.primed = False
        self.next_table_ready = self.next_agg_ready = self.adopted = False
        self._host_steps = self.state.host_steps
