"""The hidden activation that is not stored (tuning key ``elide_hidden``; acm_conv_agg_fwd_t.out == NULL in the sixteen-rows
row-local stage, acm_conv_agg_bwd_t.out == NULL in the proj_* carriers of its backward, which form the row again).

The reference of every comparison is the storing path -- the same entry points with ``out`` given, ``elide_hidden=0`` at step
level -- and every comparison is ``torch.equal``: the row formed again is the same instruction sequence on the same bits."""
import ctypes as C
import itertools

import numpy as np
import pytest
import scipy.sparse as sp
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F_IN, FP, F = 7, 8, 64


def _pattern_graph(n, seed):
    """A symmetric 0/1 pattern of mean degree about 4 (plus the diagonal) as a pattern-only operator."""
    from acm_gnn_amd.graph import CsrGraph
    rng = np.random.default_rng(seed)
    m = 2 * n
    r, c = rng.integers(0, n, m), rng.integers(0, n, m)
    a = sp.csr_matrix((np.ones(m, np.float32), (r, c)), shape=(n, n))
    a = ((a + a.T + sp.identity(n, dtype=np.float32)) > 0).astype(np.float32).tocsr()
    a.sort_indices()
    dev = torch.device(DEV)
    g = CsrGraph.from_csr(torch.from_numpy(a.indptr.astype("int32")).to(dev), torch.from_numpy(a.indices.astype("int32")).to(dev), None, n)
    return g


def _operands(n, pf, seed, negative=False):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)                                       # noqa: E731
    t = dict(agg=r(n, FP), xs=r(n, FP), w=[r(F_IN, F) * 0.3 for _ in range(3)], vec=[r(F) * 0.2 for _ in range(3)],
             lnw=[torch.rand(F, generator=g) + 0.5 for _ in range(3)], lnb=[r(F) * 0.1 for _ in range(3)], mix=r(3, 3),
             nw=[(r(F, pf) * 0.2).contiguous() for _ in range(3)], dz=r(n, 3 * pf), nxg=r(n, FP), nrs=torch.rand(n, generator=g) + 0.1)
    if negative:                # P W_L, (X - P) W_H and X W_I all negative: every channel is zero behind its ReLU, so is the row
        t["agg"] = torch.rand(n, FP, generator=g) + 0.1
        t["xs"] = t["agg"] + torch.rand(n, FP, generator=g) + 0.1
        t["w"] = [-(torch.rand(F_IN, F, generator=g) + 0.05) for _ in range(3)]
    t["agg"][:, F_IN:] = 0
    t["xs"][:, F_IN:] = 0
    return {k: ([u.to(DEV) for u in v] if isinstance(v, list) else v.to(DEV)) for k, v in t.items()}


def _run(lib, graph, c, n, pf, ln, p_drop, step, store, gather):
    """acm_conv_agg_fwd (row-local stage over a given P, the following layer's projection in its epilogue) and
    acm_conv_agg_bwd (carrying that layer's projection backward; ``gather``: and the next step's input gather), with the
    row stored (``store``) or not.  Returns the statuses and everything either call wrote."""
    from acm_gnn_amd import _lib, functional as AF
    drop = _lib.Dropout()
    drop.p, drop.tag, drop.seed, drop.step = p_drop, 1, 1234567, step.data_ptr()
    out = torch.full((n, F), float("nan"), device=DEV) if store else None
    att, stats = torch.empty(n, 4, device=DEV), torch.empty(n, 12, device=DEV)
    zlh, zi = torch.empty(n, 2 * pf, device=DEV), torch.empty(n, pf, device=DEV)
    p = _lib.ConvAggFwd()
    p.f_in, p.f_pad, p.f_out, p.relu_after, p.relu_mlp, p.layernorm, p.scale, p.n_channels = F_IN, FP, F, 1, 1, int(ln), 3.0, 3
    p.xs, p.ld_xs, p.xg, p.ld_xg = c["xs"].data_ptr(), FP, c["xs"].data_ptr(), FP
    p.w_low, p.w_high, p.w_mlp = (t.data_ptr() for t in c["w"])
    p.ld_w = F
    p.att_vec, p.ln_weight, p.ln_bias = AF._ptr_array(c["vec"]), AF._ptr_array(c["lnw"]), AF._ptr_array(c["lnb"])
    p.att_mix = c["mix"].data_ptr()
    if store:
        p.out = out.data_ptr()
    p.ld_out = F
    p.agg, p.ld_agg, p.agg_given = c["agg"].data_ptr(), FP, 1
    p.att, p.post_relu, p.post_drop = att.data_ptr(), 1, drop
    p.head_stats, p.ld_head_stats = stats.data_ptr(), 12
    p.next_w_low, p.next_w_high, p.next_w_mlp = (t.data_ptr() for t in c["nw"])
    p.next_ld_w, p.next_f, p.next_relu = pf, pf, 0
    p.next_zlh, p.ld_next_zlh, p.next_zi, p.ld_next_zi = zlh.data_ptr(), 2 * pf, zi.data_ptr(), pf
    optional = lib.acm_conv_agg_out_optional(C.byref(p), n, pf)
    st_f = lib.acm_conv_agg_fwd(graph.handle, C.byref(p), None, 0, None)
    q = _lib.ConvAggBwd()
    q.f_in, q.f_pad, q.f_out, q.relu_after, q.relu_mlp, q.layernorm, q.scale, q.n_channels = F_IN, FP, F, 1, 1, int(ln), 3.0, 3
    q.agg, q.ld_agg, q.xs, q.ld_xs = c["agg"].data_ptr(), FP, c["xs"].data_ptr(), FP
    q.w_low, q.w_high, q.w_mlp = (t.data_ptr() for t in c["w"])
    q.ld_w = F
    q.att_vec, q.ln_weight, q.ln_bias = AF._ptr_array(c["vec"]), AF._ptr_array(c["lnw"]), AF._ptr_array(c["lnb"])
    q.att_mix = c["mix"].data_ptr()
    d_params = torch.full((3 * F_IN * F + 9 * F + 9,), float("nan"), device=DEV)
    d_w = torch.full((3 * F * pf,), float("nan"), device=DEV)
    q.d_params, q.post_relu, q.post_drop = d_params.data_ptr(), 1, drop
    q.head_stats, q.ld_head_stats = stats.data_ptr(), 12
    if store:
        q.out = out.data_ptr()
    q.ld_out = F
    q.proj_dz, q.ld_proj_dz = c["dz"].data_ptr(), 3 * pf
    q.proj_w_low, q.proj_w_high, q.proj_w_mlp = (t.data_ptr() for t in c["nw"])
    q.proj_ld_w, q.proj_f, q.proj_d_w = pf, pf, d_w.data_ptr()
    nagg = None
    if gather:
        nagg = torch.full((n, FP), float("nan"), device=DEV)
        q.next_a, q.next_xg, q.ld_next_xg = graph.handle, c["nxg"].data_ptr(), FP
        q.next_row_scale, q.next_agg, q.ld_next_agg = c["nrs"].data_ptr(), nagg.data_ptr(), FP
    nbytes = C.c_size_t()
    assert lib.acm_conv_agg_bwd_workspace_bytes(n, F_IN, F, C.byref(nbytes)) == 0
    ws = torch.empty(nbytes.value // 4 + 1, device=DEV)
    st_b = lib.acm_conv_agg_bwd(n, C.byref(q), C.c_void_p(ws.data_ptr()), ws.numel() * 4, None) if st_f == 0 else -1
    torch.cuda.synchronize()
    return dict(st_f=st_f, st_b=st_b, optional=optional, out=out, att=att, head_stats=stats, next_zlh=zlh, next_zi=zi,
                d_params=d_params, proj_d_w=d_w, next_agg=nagg)


COMPARED = ("d_params", "proj_d_w", "next_agg", "head_stats", "next_zlh", "next_zi", "att")


# n: fewer rows than one wave step, a ragged last step, several steps; the gather carrier with streams for four waves is ONE
# workgroup, whose four backward waves then loop (133: three steps, 1 029: seventeen with a ragged end)
@pytest.mark.parametrize("gather,n", [(False, 1), (False, 17), (False, 133), (True, 1), (True, 17), (True, 133), (True, 1029)],
                         ids=lambda v: ("gather" if v else "plain") if isinstance(v, bool) else f"n{v}")
def test_backward_forms_the_unstored_row_again_bit_for_bit(gather, n):
    from acm_gnn_amd import _lib
    lib = _lib.load()
    graph = _pattern_graph(n, seed=n)
    if gather:
        assert graph.build_streams(n_waves=4) and graph.stream_waves == 4
    step = torch.full((1,), 5, dtype=torch.int64, device=DEV)
    cases = list(itertools.product((1, 2), (False, True), (0.0, 0.1, 0.9), (False,))) + [(2, True, 0.1, True), (1, False, 0.0, True)]
    for pf, ln, p_drop, negative in cases:
        what = f"proj_f={pf} ln={ln} p={p_drop} negative={negative}"
        c = _operands(n, pf, seed=100 * n + pf, negative=negative)
        ref = _run(lib, graph, c, n, pf, ln, p_drop, step, True, gather)
        got = _run(lib, graph, c, n, pf, ln, p_drop, step, False, gather)
        assert ref["st_f"] == 0 and ref["st_b"] == 0, (what, lib.acm_last_error())
        # the NULL launches themselves succeeded (no fallback could have stood in), as the query said they would
        assert got["optional"] == 1 and got["st_f"] == 0 and got["st_b"] == 0, (what, got["st_f"], got["st_b"], lib.acm_last_error())
        for key in COMPARED:
            if ref[key] is None:
                continue
            assert torch.isfinite(ref[key]).all(), (what, key)
            assert torch.equal(ref[key], got[key]), (what, key, float((ref[key] - got[key]).abs().max()))
        if negative:
            assert float(ref["out"].abs().max()) == 0.0, what
        elif p_drop < 0.5 and n > 1:
            assert float(ref["out"].abs().max()) > 0.0, what           # (the comparison is not one of zeros)


def test_other_null_forms_keep_their_errors():
    """out == NULL outside the envelope: no next projection, the fused gather forward, a backward without proj_dz riders'
    conditions -- an error status, never a launch."""
    from acm_gnn_amd import _lib
    lib = _lib.load()
    n, pf = 40, 2
    graph = _pattern_graph(n, seed=3)
    c = _operands(n, pf, seed=9)
    step = torch.zeros(1, dtype=torch.int64, device=DEV)
    ok = _run(lib, graph, c, n, pf, True, 0.1, step, False, False)
    assert ok["optional"] == 1 and ok["st_f"] == 0 and ok["st_b"] == 0
    from acm_gnn_amd import functional as AF
    p = _lib.ConvAggFwd()
    p.f_in, p.f_pad, p.f_out, p.relu_after, p.relu_mlp, p.layernorm, p.scale, p.n_channels = F_IN, FP, F, 1, 1, 1, 3.0, 3
    p.xs, p.ld_xs, p.xg, p.ld_xg = c["xs"].data_ptr(), FP, c["xs"].data_ptr(), FP
    p.w_low, p.w_high, p.w_mlp = (t.data_ptr() for t in c["w"])
    p.ld_w, p.ld_out = F, F
    p.att_vec, p.ln_weight, p.ln_bias = AF._ptr_array(c["vec"]), AF._ptr_array(c["lnw"]), AF._ptr_array(c["lnb"])
    p.att_mix = c["mix"].data_ptr()
    att, agg = torch.empty(n, 4, device=DEV), torch.empty(n, FP, device=DEV)
    p.att, p.post_relu = att.data_ptr(), 1
    p.agg, p.ld_agg, p.agg_given = c["agg"].data_ptr(), FP, 1
    ws = graph.workspace(FP)
    # (1) the row-local stage without a next projection: nobody would ever see the row
    assert lib.acm_conv_agg_out_optional(C.byref(p), n, 0) == 0
    assert lib.acm_conv_agg_fwd(graph.handle, C.byref(p), C.c_void_p(ws.data_ptr()), ws.numel() * 4, None) == 1
    # (2) the gather forward (no P given), with a next projection
    zlh, zi = torch.empty(n, 2 * pf, device=DEV), torch.empty(n, pf, device=DEV)
    p.next_w_low, p.next_w_high, p.next_w_mlp = (t.data_ptr() for t in c["nw"])
    p.next_ld_w, p.next_f = pf, pf
    p.next_zlh, p.ld_next_zlh, p.next_zi, p.ld_next_zi = zlh.data_ptr(), 2 * pf, zi.data_ptr(), pf
    p.agg, p.agg_given = agg.data_ptr(), 0
    assert lib.acm_conv_agg_out_optional(C.byref(p), n, pf) == 0
    assert lib.acm_conv_agg_fwd(graph.handle, C.byref(p), C.c_void_p(ws.data_ptr()), ws.numel() * 4, None) == 1
    # (3) the query ties the backward half to head_stats and the fused ReLU
    p.agg, p.agg_given = c["agg"].data_ptr(), 1
    assert lib.acm_conv_agg_out_optional(C.byref(p), n, 0) == 1 and lib.acm_conv_agg_out_optional(C.byref(p), n, pf) == 0
    stats = torch.empty(n, 12, device=DEV)
    p.head_stats, p.ld_head_stats = stats.data_ptr(), 12
    assert lib.acm_conv_agg_out_optional(C.byref(p), n, pf) == 1 and lib.acm_conv_agg_out_optional(C.byref(p), n, 3 - pf) == 0
    p.post_relu = 0
    assert lib.acm_conv_agg_out_optional(C.byref(p), n, pf) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------- step level
def _step_case(n=2048, seed=7):
    from acm_gnn_amd import data as D
    from acm_gnn_amd.distributed import make_sharded_operators
    adj = D.chung_lu_graph(n, 20 * n, 400, seed=seed)                   # mean degree 40: the input pipeline's regime
    low, deg = D.build_filters(adj)
    ops = make_sharded_operators(low, deg, torch.device(DEV))
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n, F_IN, generator=g).to(DEV)
    y = torch.randint(0, 2, (n,), generator=g).to(DEV)
    return ops, x, y


def _train_and_eval(ops, x, y, elide, tune, steps=6):
    from acm_gnn_amd import GCN, FusedAdamW, functional as AF, train as T
    n = x.shape[0]
    tune(pipeline=1024, elide_hidden=elide)
    torch.manual_seed(0)
    model = GCN(F_IN, 64, 2, 2, n, 0.1, "acmgcnp", 0, variant=False, attn_layernorm=True).to(DEV)
    model.dropout_state = AF.DropoutState(torch.device(DEV), seed=31)
    opt = FusedAdamW(model.parameters(), lr=0.01, weight_decay=1e-3)
    w = T.row_weights(torch.arange(0, n, 3, device=DEV), n)
    step = T.TrainStep(model, opt, x, ops, y, w, use_graph=True, small_step=False)       # (the general path, not the fused small step)
    assert step.pipe is not None
    losses = []
    for _ in range(steps):
        step()
        losses.append(float(step.loss))
    ev = T.EvalStep(model, x, ops, y, [torch.arange(0, n, 2, device=DEV), torch.arange(1, n, 2, device=DEV)], use_graph=True,
                    small_step=False)
    logits, accs, vloss = ev()
    # the launches of one more (eager) evaluation forward and of one more eager training step, by label
    from acm_gnn_amd import functional as AF2
    timer = AF2.KernelTimer()
    AF2.set_kernel_timer(timer)
    try:
        T.EvalStep(model, x, ops, y, [torch.arange(0, n, 2, device=DEV)], loss_set=0, small_step=False)()
    finally:
        AF2.set_kernel_timer(None)
    labels = sorted(timer.events)
    return dict(labels=labels, losses=losses, params=[p.detach().clone() for p in model.parameters()], logits=logits.clone(), accs=accs,
                vloss=vloss, step=step, ev=ev)


@pytest.fixture(scope="module")
def step_case():
    return _step_case()


def test_captured_step_and_evaluation_pass_equal_the_storing_path(step_case, tune):
    ops, x, y = step_case
    ref = _train_and_eval(ops, x, y, 0, tune)
    got = _train_and_eval(ops, x, y, 1, tune)
    assert not ref["step"].hidden_elided and "elide_hidden=0" in ref["step"].hidden_elided_refused
    assert not ref["ev"].hidden_elided and "elide_hidden=0" in ref["ev"].hidden_elided_refused
    assert got["step"].hidden_elided and got["step"].hidden_elided_refused is None, got["step"].hidden_elided_refused
    assert got["ev"].hidden_elided and got["ev"].hidden_elided_refused is None, got["ev"].hidden_elided_refused
    # the evaluation forward runs the same launches in both arms: nobody asked for the unwritten row's bytes (conv_agg_out)
    assert got["labels"] == ref["labels"] and any(k.startswith("conv_agg_epi/") for k in got["labels"]), (ref["labels"], got["labels"])
    assert not any(k.startswith("conv_agg_out/") for k in got["labels"])
    assert ref["losses"] == got["losses"], (ref["losses"], got["losses"])
    assert all(torch.equal(a, b) for a, b in zip(ref["params"], got["params"]))
    assert torch.equal(ref["logits"], got["logits"]) and ref["accs"] == got["accs"] and ref["vloss"] == got["vloss"]


def _hidden_layer_pass(ops, x, elide, tune, with_defer, write=False):
    """One forward / backward of the two-layer model on autograd with the step's context made by hand; returns the hidden
    activation (as a consumer sees it after asking for its bytes), the gradients and what the layer reported."""
    from acm_gnn_amd import GCN, functional as AF
    n = x.shape[0]
    tune(pipeline=1024, elide_hidden=elide)
    torch.manual_seed(0)
    model = GCN(F_IN, 64, 2, 2, n, 0.1, "acmgcnp", 0, variant=False, attn_layernorm=True).to(DEV)
    model.fused_dropout = True
    model.dropout_state = AF.DropoutState(torch.device(DEV), seed=31)
    model.train()
    assert AF.InputPipeline.eligible(model, ops, x)                          # (builds the operator's id streams)
    pipe = AF.InputPipeline(ops, x, 0.1, model.dropout_state, tag=0)       # (P at hand: the row-local stage is its own launch)
    pipe.prime()
    defer = AF.DeferredReductions() if with_defer else None
    call = AF.CallContext(defer=defer, pipe=pipe)
    from acm_gnn_amd import layers as L
    seen = {}
    conv = L.AF.acm_conv

    def spy(inp, *a, **k):                      # (the layers' entry point: the second call is the output layer's)
        if isinstance(inp, torch.Tensor) and inp.shape[1] == 64:
            seen["elided"] = call.link is not None and call.link.token is not None and not call.link.token.written
            if write:
                AF.ensure_hidden_written(call, inp)
                seen["hidden"] = inp.detach().clone()
        return conv(inp, *a, **k)

    L.AF.acm_conv = spy
    try:
        out = model(x, ops, None, None, call=call)
    finally:
        L.AF.acm_conv = conv
    pipe.make_next()
    out.backward(torch.ones_like(out) / n)
    if defer is not None:
        defer.flush()
    torch.cuda.synchronize()
    grads = {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}
    return dict(seen=seen, grads=grads, elision=call.elision, out=out.detach().clone())


def test_materialisation_helper_writes_the_stored_row(step_case, tune):
    """A consumer that asks for the bytes of an unwritten hidden activation gets the forward's row: one more launch of the
    row-local stage over the copies the forward left for the backward."""
    ops, x, _ = step_case
    ref = _hidden_layer_pass(ops, x, 0, tune, True, write=True)
    got = _hidden_layer_pass(ops, x, 1, tune, True, write=True)
    assert ref["elision"][0] is False and not ref["seen"]["elided"]
    assert got["elision"] == (True, None) and got["seen"]["elided"]
    assert float(ref["seen"]["hidden"].abs().max()) > 0
    assert torch.equal(ref["seen"]["hidden"], got["seen"]["hidden"])
    assert torch.equal(ref["out"], got["out"])
    assert ref["grads"].keys() == got["grads"].keys() and all(torch.equal(ref["grads"][k], got["grads"][k]) for k in ref["grads"])


def test_a_call_without_a_deferral_list_does_not_elide(step_case, tune):
    """Without CallContext.defer the literal layer materialises its input gradient (it cannot go lazy): the hidden layer must
    know that up front and store its row; the gradients are the storing path's.  With one, the same pass elides."""
    ops, x, _ = step_case
    ref = _hidden_layer_pass(ops, x, 0, tune, False)
    got = _hidden_layer_pass(ops, x, 1, tune, False)
    assert got["elision"][0] is False and "deferral" in got["elision"][1] and not got["seen"]["elided"]
    assert torch.equal(ref["out"], got["out"])
    assert ref["grads"].keys() == got["grads"].keys() and all(torch.equal(ref["grads"][k], got["grads"][k]) for k in ref["grads"])
    lazy = _hidden_layer_pass(ops, x, 1, tune, True)
    assert lazy["elision"] == (True, None) and lazy["seen"]["elided"]
    stored = _hidden_layer_pass(ops, x, 0, tune, True)
    assert torch.equal(stored["out"], lazy["out"])
    assert all(torch.equal(stored["grads"][k], lazy["grads"][k]) for k in stored["grads"])
