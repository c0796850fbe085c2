"""The unwritten hidden activation (tuning key ``elide_hidden``) without a GPU: the one predicate the hidden layer and the
layer behind it decide by, and the test double -- which lacks acm_conv_agg_out_optional -- training exactly as before."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fake_lib  # noqa: E402


def test_symbol_tuning_key_and_header():
    from acm_gnn_amd import _lib, tuning
    lib = _lib.load()
    assert lib.acm_version() == 29 == _lib.ABI_VERSION                    # a new entry point, the same ABI number
    assert _lib.OUT_OPTIONAL_SYMBOL == "acm_conv_agg_out_optional" in _lib.EXPORTED_SYMBOLS and hasattr(lib, _lib.OUT_OPTIONAL_SYMBOL)
    assert lib.acm_conv_agg_out_optional(None, 10, 1) == 0                # a question, not a launch: no device needed
    assert tuning.HOST_DEFAULTS["elide_hidden"] == 1 and tuning.HOST_RANGES["elide_hidden"] == (0, 1)
    assert tuning.parse("elide_hidden=0") == ({}, {"elide_hidden": 0})
    with tuning.override(elide_hidden=0):
        assert tuning.HOST.elide_hidden == 0
    assert tuning.HOST.elide_hidden == 1


def test_query_and_launchers_share_the_predicate_on_the_host():
    """acm_conv_agg_out_optional over a table of argument blocks (host code only: it reads the block, nothing behind it)."""
    import ctypes as C
    from acm_gnn_amd import _lib
    lib = _lib.load()
    buf = (C.c_float * 64)()                       # any 16-byte aligned non-NULL address
    ptr = C.addressof(buf) + (-C.addressof(buf)) % 16

    def ask(proj_f, n=100, **kw):
        p = _lib.ConvAggFwd()
        p.f_in, p.f_pad, p.f_out, p.n_channels, p.agg_given, p.post_relu = 7, 8, 64, 3, 1, 1
        p.ld_agg = p.ld_xs = 8
        p.ld_out = 64
        p.next_f, p.next_zlh, p.next_zi, p.head_stats, p.ld_head_stats = 2, ptr, ptr, ptr, 12
        for k, v in kw.items():
            setattr(p, k, v)
        return lib.acm_conv_agg_out_optional(C.byref(p), n, proj_f)

    assert ask(2) == 1 and ask(0) == 1 and ask(1, next_f=1) == 1
    assert ask(1) == 0                                        # the backward would carry another width than the forward projected
    assert ask(2, head_stats=None) == 0 and ask(0, head_stats=None) == 1        # an evaluation pass keeps no statistics
    assert ask(2, post_relu=0) == 0 and ask(2, post_scale=ptr, ld_post_scale=64) == 0
    assert ask(2, n_channels=4) == 0 and ask(0, n_channels=4) == 0
    assert ask(2, agg_given=0) == 0 and ask(2, next_f=0) == 0 and ask(2, next_zlh=None) == 0
    assert ask(2, f_out=32) == 0 and ask(0, f_in=3, f_pad=4) == 1 and ask(2, f_in=3, f_pad=4, next_f=2) == 0   # backward: f_pad 8
    assert ask(2, f_pad=4) == 0                               # f_pad does not belong to f_in
    assert ask(2, n=2 ** 31 // 64) == 0                       # 32-bit element offsets
    assert ask(-1) == 0 and ask(2, n=-1) == 0
    assert ask(2, out=ptr + 4, ld_out=63) == 1                # `out` itself is not looked at: the question is about its absence


def test_shared_lazy_and_elide_predicates():
    from acm_gnn_amd import functional as AF, tuning
    d = AF.DeferredReductions()
    assert AF.lazy_hidden_why_not(d, 1) is None
    assert "deferral" in AF.lazy_hidden_why_not(None, 1)
    assert "hop" in AF.lazy_hidden_why_not(d, 2)
    assert "ReLU" in AF.lazy_hidden_why_not(d, 1, post_relu=False)
    assert "post_scale" in AF.lazy_hidden_why_not(d, 1, post_scale=torch.ones(2, 2))
    assert "statistics" in AF.lazy_hidden_why_not(d, 1, head_stats=False)

    asked = []
    yes = lambda pf: (asked.append(pf), True)[1]                     # noqa: E731
    nxt = ((None, None, None), False, 2, False)

    def why(defer=d, promise=True, nxt=nxt, agg_given=True, sharded=False, grad=True, hops=1, relu=True, scale=None, stats=True,
            f=64, query=yes):
        call = AF.CallContext(defer=defer)
        call.next_private = promise
        return AF.hidden_elision_why_not(call, nxt, agg_given, sharded, grad, hops, relu, scale, stats, f, query)

    assert why() is None and asked == [2]                            # a training step asks about both halves ...
    assert why(grad=False, defer=None, stats=False) is None and asked == [2, 0]     # ... an evaluation pass about the forward
    assert "promise" in why(promise=False)
    assert "no query symbol" in why(query=None)
    assert "epilogue" in why(nxt=None)
    assert "row-local" in why(agg_given=False)
    assert "sharded" in why(sharded=True)
    assert "deferral" in why(defer=None) and "hop" in why(hops=2) and "ReLU" in why(relu=False)
    assert "post_scale" in why(scale=torch.ones(1, 1)) and "statistics" in why(stats=False)
    assert "declines" in why(query=lambda pf: False)
    with tuning.override(elide_hidden=0):
        assert "elide_hidden=0" in why()
    with tuning.override(csr_features=64):
        assert "csr_features" in why()
    with tuning.override(csr_features=0):
        assert why() is None


def test_an_unwritten_token_is_written_once_for_whoever_asks():
    import gc
    import weakref
    from acm_gnn_amd import functional as AF

    class Launch:
        def __init__(self):
            self.log = []

        def fresh(self):
            return torch.zeros(3, 2)

        def __call__(self, out):
            self.log.append(out)
            out.fill_(7.0)

    call = AF.CallContext()
    token, other, launch = torch.zeros(3, 2), torch.zeros(3, 2), Launch()
    log = launch.log
    call.elided = tok = AF.HiddenToken(token, launch)
    AF.ensure_hidden_written(call, other)
    AF.ensure_hidden_written(call, None)
    AF.ensure_hidden_written(None, token)
    assert log == [] and not tok.written and tok.names(token) and not tok.names(other)
    AF.ensure_hidden_written(call, token)
    AF.ensure_hidden_written(call, token)
    assert len(log) == 1 and log[0] is token and float(token.min()) == 7.0 and tok.written and not tok.names(token)
    assert tok.write() is token and tok.write(token) is token and len(log) == 1
    # a token that is gone: the row goes into a fresh tensor, once
    t2 = torch.zeros(3, 2)
    tok2 = AF.HiddenToken(t2, launch)
    del t2
    fresh = tok2.write()
    assert fresh is not None and float(fresh.min()) == 7.0 and tok2.write() is fresh and len(log) == 2
    # no reference cycle: dropping the last reference frees the launch record (and what it keeps) without the collector
    gc.disable()
    try:
        l3 = Launch()
        ref = weakref.ref(l3)
        tok3 = AF.HiddenToken(token, l3)
        del l3, tok3
        assert ref() is None
    finally:
        gc.enable()


def test_the_model_promises_only_for_untouched_layers():
    from acm_gnn_amd import GCN
    model = GCN(7, 64, 2, 2, 50, 0.0, "acmgcnp", 0)
    assert model._hidden_is_private()
    h = model.gcns[0].register_forward_hook(lambda m, i, o: None)
    assert not model._hidden_is_private()
    h.remove()
    assert model._hidden_is_private()
    inner = model.gcns[1].forward
    model.gcns[1].forward = lambda *a, **k: inner(*a, **k)          # a wrapper on the instance could read its input
    assert not model._hidden_is_private()
    del model.gcns[1].forward
    assert model._hidden_is_private()
    assert not GCN(7, 64, 2, 2, 50, 0.0, "acmgcnpp", 0)._hidden_is_private()


def _setup(seed=3):
    from acm_gnn_amd import GCN, data as D
    from acm_gnn_amd.graph import CsrGraph, FilterOperators
    adj, _, y_np, _, _ = D.synthetic_dataset("tiny", seed=seed)
    low, _ = D.build_filters(adj)
    ops = FilterOperators(CsrGraph.from_scipy(low, "cpu"))
    n = adj.shape[0]
    x = torch.randn(n, 7, generator=torch.Generator().manual_seed(seed))
    y = torch.from_numpy(y_np)
    w = torch.full((n,), 1.0 / n)
    torch.manual_seed(0)
    model = GCN(7, 64, int(y.max()) + 1, 2, n, 0.0, "acmgcnp", 0)
    return model, ops, x, y, w


def test_the_double_lacks_the_query_symbol_stores_the_row_and_trains_as_before(monkeypatch):
    fake = fake_lib.install(monkeypatch)
    from acm_gnn_amd import FusedAdam, _lib, train as T, tuning
    assert getattr(fake, _lib.OUT_OPTIONAL_SYMBOL, None) is None
    outs, fwd = [], fake.acm_conv_agg_fwd
    monkeypatch.setattr(fake, "acm_conv_agg_fwd", lambda a, p, *r: (outs.append(bool(p._obj.out)), fwd(a, p, *r))[1])
    runs = {}
    for switch in (1, 0):
        with tuning.override(elide_hidden=switch):
            model, ops, x, y, w = _setup()
            step = T.TrainStep(model, FusedAdam(model.parameters(), lr=0.01, weight_decay=5e-4), x, ops, y, w, small_step=False)
            losses = [float(step()) for _ in range(4)]
            assert not step.hidden_elided
            assert ("no query symbol" if switch else "elide_hidden=0") in step.hidden_elided_refused, step.hidden_elided_refused
            ev = T.EvalStep(model, x, ops, y, [torch.arange(0, x.shape[0], 2)], loss_set=0, small_step=False)
            logits, _, _ = ev()
            assert not ev.hidden_elided and ("no query symbol" if switch else "elide_hidden=0") in ev.hidden_elided_refused
            runs[switch] = (losses, [p.detach().clone() for p in model.parameters()], logits.clone())
    assert outs and all(outs)                                        # every forward of the hidden layer was handed an `out`
    assert runs[1][0] == runs[0][0] and np.isfinite(runs[1][0]).all() and runs[1][0][-1] < runs[1][0][0]
    assert all(torch.equal(a, b) for a, b in zip(runs[1][1], runs[0][1])) and torch.equal(runs[1][2], runs[0][2])
