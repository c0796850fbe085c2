"""The hand-off between a hidden layer and the layer after it: HiddenLink, the one object both layers and the model talk to,
the records that travel over it, and the two rules -- why not lazy, why not elide -- the layers decide by."""
import weakref
from collections import namedtuple

import torch

from .. import tuning
from ._launch import _F32


# The records that travel over a HiddenLink:
# the consumer's narrow projection, asked to ride the producer's epilogue (acm_conv_agg_fwd_t.next_*): its three weights, its
# relu_before, its width F' and whether it gathers [Z_L | Z_H | struc_low] from packed 32-byte rows (four channels, two columns)
ProjRequest = namedtuple("ProjRequest", "w3 relu f2 pack4")
# what the producer's epilogue projected for the consumer: the tables, the three weights' addresses and the relu they were made with
PreProj = namedtuple("PreProj", "zlh zi ptrs relu")
# the consumer's input gradient, left to the producer's backward kernel (acm_conv_agg_bwd_t.proj_*): dZ, the weights, where the
# kernel writes the consumer's weight gradients, the activation itself and the [n, F] tensor that stands for dX on the way there
LazyGrad = namedtuple("LazyGrad", "dz w3 d_w x placeholder")


class HiddenLink:
    """One producer -> consumer edge of one model call: "layer A's output is layer B's input and nobody else's".  The model
    (models.GCN._two_layers) makes it before the producer runs and hangs it on ``CallContext.link``; both layers talk to it.

    The request, made by the model:
      ``consumer``       the layer behind the producer; its narrow projection may ride the producer's epilogue.  Taken one-shot
                         (``take_request``); a producer that cannot carry it (_AcmAggWide) still consumes it.
      ``grad_private``   nothing but the consumer sends the activation a gradient: the consumer's backward may leave dX and dW'
                         to the producer's backward kernel (``lazy``) instead of running acm_proj_bwd.
      ``bytes_private``  nothing but the consumer reads the activation's bytes (the stronger promise: untouched layers, no
                         hooks -- models.GCN._hidden_is_private): the producer may leave it unwritten.
      ``seal()``         the producer has returned: whatever layer runs next under this link is not its producer.
    What the producer (_AcmAggFirst) left, ``produced``:
      the activation's identity (weakly), whether its backward will run (``backs``), the pre-projection (``pre``, taken
      one-shot by ``take_pre``) and the HiddenToken of an ``out`` it left unwritten (``token``).  Its report (elided, why not)
      goes to ``CallContext.elision``, where it outlives the link: a layer without a link reports as well.
    The lazy gradient (``lazy``): deposited by the consumer's backward where ``awaits_lazy()``, taken one-shot by the
    producer's (``take_lazy``).

    Lifetime.  The link never refers to a Function's ctx and holds the activation WEAKLY; ctxs and the call refer to the link.
    Under autograd ``out -> grad_fn -> ctx -> link -> out`` held strongly would be a cycle through C++ that no collector sees
    (and on a Tape one that keeps the step's tensors for the cyclic collector, which may free them in the middle of a later
    stream capture).  Only ``lazy.x`` is strong, between the consumer's and the producer's backward.  The call drops its
    reference when the model's two-layer section ends, also on an exception.  A backward uses the link its forward captured
    (``ctx.link``), never the call's current one: autograd may run it on another thread after the call has moved on."""
    __slots__ = ("consumer", "grad_private", "bytes_private", "sealed", "backs", "pre", "token", "lazy", "lazy_agreed", "_out")

    def __init__(self, consumer=None, grad_private=False, bytes_private=False):
        self.consumer, self.grad_private, self.bytes_private = consumer, bool(grad_private), bool(bytes_private)
        self.sealed = self.backs = self.lazy_agreed = False
        self.pre = self.token = self.lazy = self._out = None

    # ---- the producer's side
    def take_request(self, f, dev, row_local_only=False):
        """The consumer's ProjRequest when its projection can ride this layer's epilogue, else None.  Default: only where
        the row-local stage runs as its own kernel (``row_local_only``: P = A_low X is given -- the input pipeline, evaluation
        passes -- and the sixteen-rows-per-wave kernel of acm_conv_agg16.hip carries the projection for ~6 us against the ~20 us
        of a separate acm_proj_fwd launch); inside the fused gather kernel it costs what it saves (DESIGN.md section 9a:
        built, measured, removed)."""
        nxt, self.consumer = self.consumer, None
        if nxt is None or not row_local_only or not (tuning.kernel()["rows16"] & tuning.ROWS16_EPI):
            return None
        try:
            w3 = (nxt.weight_low, nxt.weight_high, nxt.weight_mlp)
            cfg = nxt._config()
        except AttributeError:
            return None
        f2 = w3[0].shape[1]
        ok = (f2 <= 2 and all(w.dtype == _F32 and w.is_contiguous() and w.device == dev and
                                                       tuple(w.shape) == (f, f2) for w in w3))
        return ProjRequest(w3, bool(cfg.relu_before), f2, cfg.n_channels == 4 and f2 == 2) if ok else None

    def produced(self, out, backs, pre=None, token=None):
        self._out, self.backs, self.pre, self.token = weakref.ref(out), bool(backs), pre, token

    def seal(self):
        self.consumer, self.sealed = None, True

    def take_lazy(self):
        lazy, self.lazy = self.lazy, None
        return lazy

    # ---- the consumer's side
    def take_pre(self, x, w3, relu):
        """(zlh, zi) the producer projected for (x, w3, relu), or None."""
        pre, self.pre = self.pre, None
        out = self._out() if self._out is not None else None
        if pre is None or out is None or not isinstance(x, torch.Tensor):
            return None
        if (x.data_ptr() == out.data_ptr() and x.shape == out.shape and x.stride() == out.stride() and pre.relu == bool(relu)
                and tuple(w.data_ptr() for w in w3) == pre.ptrs):
            return pre.zlh, pre.zi
        return None

    def carries_gradient_of(self, x):
        """``x`` is the very object the producer returned, it carries a gradient edge to that producer (under autograd its
        ``grad_fn`` is the node of the forward that registered here, on a Tape that forward's record: either marks what it
        returns ``requires_grad``), that producer's backward will run and nothing else sends ``x`` a gradient."""
        return (self.grad_private and self.backs and self._out is not None and self._out() is x and x.requires_grad)

    def unwritten(self, x):
        """``x`` is the activation its producer left unwritten (the object, or a tensor over its memory), unwritten still."""
        return self.token is not None and self.token.names(x)

    def ensure_written(self, x):
        """A reader needs the bytes of ``x``: written now if it is the unwritten activation."""
        if self.unwritten(x):
            self.token.write(x)

    def awaits_lazy(self):
        return self.lazy_agreed and self.lazy is None


def lazy_hidden_why_not(defer, hops, post_relu=True, post_scale=None, head_stats=True):
    """Why the gradient of a hidden activation cannot be left to the producing layer's backward kernel
    (acm_conv_agg_bwd_t.proj_*) -- None: it can.  The ONE statement of the rule: the consuming layer decides with it whether
    to go lazy (_AcmLiteral: its own two arguments), the producing layer whether it may leave the activation unwritten, which
    only the lazy backward can do without it (_AcmAggFirst: with its post-op and head statistics as well).
    ONLY under a deferral list: the consumer's dW' is then written by a LATER kernel than the one its backward returns from --
    exactly the contract of DeferredReductions ("every .grad is undefined until the flush").  Without one, autograd's
    AccumulateGrad may ADD the still unwritten dW' to an existing .grad right behind that node (zero_grad(set_to_none=False),
    gradient accumulation, hooks), or the producer's backward may never run (torch.autograd.grad on a subset)."""
    if defer is None:
        return "no deferral list (CallContext.defer): the following layer materialises its input gradient"
    if int(hops) != 1:
        return "k-hop operators"
    if not post_relu:
        return "no fused ReLU behind the layer"
    if post_scale is not None:
        return "a post_scale mask tensor"
    if not head_stats:
        return "no head statistics (no gradient is asked of the layer)"
    return None


def hidden_elision_why_not(call, nxt, agg_given, sharded, needs_grad, hops, post_relu, post_scale, head_stats, f, query):
    """Why an aggregate-first layer stores its output although only the following layer consumes it -- None: it may stay
    unwritten.  ``call.link``: the open link it produces for (none, or sealed: no promise); ``nxt``: the ProjRequest its epilogue
    carries; ``query(proj_f)``: the library's answer (acm_conv_agg_out_optional), or None where it lacks the symbol."""
    link = call.link
    if not tuning.HOST.elide_hidden:
        return "tuning: elide_hidden=0"
    if link is None or link.sealed or not link.bytes_private:
        return "the model did not promise that only the following layer reads the hidden activation"
    if query is None:
        return "library has no query symbol (acm_conv_agg_out_optional)"
    if nxt is None:
        return "the following layer's projection does not ride this layer's epilogue"
    if not agg_given:
        return "the row-local stage is not a launch of its own (no P = A_low X at hand)"
    if sharded:
        return "row-sharded operators"
    if 0 < tuning.HOST.csr_features <= f:
        return "tuning: csr_features would count the hidden activation's zeros"
    if needs_grad:
        why = lazy_hidden_why_not(call.defer, hops, post_relu, post_scale, head_stats)
        if why is not None:
            return why
    if not query(nxt.f2 if needs_grad else 0):
        return "the library declines these shapes (acm_conv_agg_out_optional)"
    return None


class HiddenToken:
    """A hidden activation its layer left unwritten (acm_conv_agg_fwd_t.out == NULL): the tensor the layer returned is an
    identity token, and this object is the one place that knows whether its bytes exist (``written``) and how to make them
    (``write``).  The HiddenLink holds it; it holds the token weakly and nothing of the link's or a ctx's."""
    __slots__ = ("written", "_launch", "_token", "_fresh")

    def __init__(self, token, launch):
        self.written, self._launch, self._token, self._fresh = False, launch, weakref.ref(token), None

    def names(self, x):
        """``x`` is the unwritten token (the object, or a tensor over the same memory)."""
        tok = self._token()
        return (not self.written and tok is not None and isinstance(x, torch.Tensor)
                and (x is tok or (x.data_ptr() == tok.data_ptr() and x.shape == tok.shape)))

    def write(self, into=None):
        """The row, written now unless it has been: into ``into`` (a tensor over the token's memory), else into the token while
        it is alive, else into a fresh tensor.  Returns the tensor that holds it (None: written once into a token that is gone)."""
        if not self.written:
            out = into if into is not None else self._token()
            if out is None:
                out = self._fresh = self._launch.fresh()
            self._launch(out)
            self.written, self._launch = True, None
            return out
        return into if into is not None else (self._token() if self._token() is not None else self._fresh)


def ensure_hidden_written(call, x):
    """A consumer is about to read the bytes of ``x``: if it is a hidden activation its layer left unwritten, write it now."""
    link = getattr(call, "link", None)
    if link is not None:
        link.ensure_written(x)
