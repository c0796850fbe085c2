"""What train.TrainStep and train.EvalStep send to the library in the steps nothing else pins, on the test double: the step
whose unproven tape breaks, the step whose gradient is not adopted, the BCE step, and a step and a pass over a model whose
``forward`` lacks the ``call`` keyword.  The entry-point sequences were recorded on the commit before train.py stated the model
call, the redo and the capture once; that refactoring, and any after it, must reproduce them."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from step_double import _Calls, _headline_step, _setup, _Wrapper  # noqa: E402

_AGG_FWD, _AGG_BWD = "acm_conv_agg_fwd", "acm_conv_agg_bwd"
_OUTPUT_LAYER = ["acm_conv_fwd_tail", "acm_conv_fwd", "acm_nll_loss", "acm_conv_bwd_local", "acm_conv_bwd_spmm"]   # (the double declines the tail)
_PRIME = ["acm_dropout", "acm_spmm_ex"]                                          # InputPipeline.prime()
_LAUNCHES = {
    # the aborted forward (up to the residual add), then the whole step on autograd
    "broken-tape": ["acm_linear_fwd", (_AGG_FWD, "out")]
                   + ["acm_linear_fwd", (_AGG_FWD, "out"), "acm_proj_fwd_at"] + _OUTPUT_LAYER
                   + ["acm_proj_bwd", (_AGG_BWD, "grad_out"), "acm_linear_bwd", "acm_adam_step", "acm_reduce_flush"],
    # the deferring attempt and its flush, then the pipeline primed again and the step without deferral
    "not-adopted": _PRIME + [(_AGG_FWD, "next_zlh", "agg_copy", "next_x")] + _OUTPUT_LAYER + [(_AGG_BWD, "proj_dz", "next_agg"), "acm_reduce_flush"]
                   + _PRIME + [(_AGG_FWD, "out", "next_zlh", "agg_copy", "next_x")] + _OUTPUT_LAYER
                   + ["acm_proj_bwd", (_AGG_BWD, "out", "grad_out", "next_agg"), "acm_adam_step"],
    # no loss-tail request: the output layer's forward, then the BCE launch
    "bce": [(_AGG_FWD, "next_zlh", "agg_copy", "next_x"), "acm_conv_fwd", "acm_bce_loss", "acm_conv_bwd_local", "acm_conv_bwd_spmm",
            (_AGG_BWD, "proj_dz", "next_agg"), "acm_adam_step", "acm_reduce_flush"],
    # through the ambient contexts: the tail is asked, the reductions are deferred into the optimizer's launch
    "wrapper": ["acm_dropout", (_AGG_FWD, "out"), "acm_proj_fwd_at"] + _OUTPUT_LAYER + [(_AGG_BWD, "out", "proj_dz"), "acm_adam_step", "acm_reduce_flush"],
    "wrapper-eval": [(_AGG_FWD, "next_zlh"), "acm_conv_fwd", "acm_eval_metrics"],
}


def _np_bce_loss(fake):
    """acm_bce_loss as include/acm_hip.h states it, on host pointers: sum_i w_i / C * sum_c bce(z_ic, [c == y_i]) and dz."""
    from fake_lib import _vec, _view

    def bce(n, c, z, ldz, y, w, loss, dz, ldd, ws, wsb, defer, stream):
        Z, W = _view(z, n, c, ldz).astype(np.float64), _vec(w, n).astype(np.float64)[:, None] / c
        T = (np.arange(c)[None, :] == _vec(y, n, np.int64)[:, None]).astype(np.float64)
        if dz:
            _view(dz, n, c, ldd)[...] = W * (1.0 / (1.0 + np.exp(-Z)) - T)
        return fake._emit(defer, [(_vec(loss, 1), float((W * (np.maximum(Z, 0) - Z * T + np.log1p(np.exp(-np.abs(Z))))).sum()))])

    def nbytes(n, out):
        out._obj.value = 4
        return 0

    return bce, nbytes


def _install(monkeypatch):
    """The double with the query symbol (tests/fake_lib_elide.py) and the BCE launch, behind the recorder."""
    import fake_lib_elide
    fake = fake_lib_elide.install(monkeypatch)
    fake.acm_bce_loss, fake.acm_bce_loss_workspace_bytes = _np_bce_loss(fake)
    return fake, _Calls(monkeypatch, fake)


def _count_passes(model):
    """A buffer that every forward of ``model`` moves: a redone step that did not put the buffers back would count twice."""
    model.register_buffer("passes", torch.zeros(()))

    def count(m, args):
        m.passes.add_(1)

    model.register_forward_pre_hook(count)


def _state_after(step):
    """What a redone step must not count twice: the model's buffers, the optimizer's step counts, the dropout counter's shadow."""
    ds = getattr(step.model, "dropout_state", None)
    return ([b.clone() for b in step.model.buffers()], [float(st["step"]) for st in step.opt.state.values()],
            ds.host_steps if ds is not None else None)


def _same_state(a, b):
    return len(a[0]) == len(b[0]) and all(torch.equal(p, q) for p, q in zip(a[0], b[0])) and a[1] == b[1] and a[2] == b[2]


def _broken_tape_step(tape):
    """test_deferred_reductions_cpu's ACM-GCN++ with F.dropout masks: its residual add is a torch operation, so the first taped
    step aborts after the forward and is redone on autograd."""
    from acm_gnn_amd import GCN, FusedAdamW, data as D, train as T
    from acm_gnn_amd.distributed import make_sharded_operators
    adj, x_np, y_np, (tr, _, _), _ = D.synthetic_dataset("tiny", seed=3)
    low, deg = D.build_filters(adj)
    ops = make_sharded_operators(low, deg, torch.device("cpu"))
    x, y = torch.from_numpy(D.row_normalize_features(x_np)), torch.from_numpy(y_np)
    w = T.row_weights(torch.from_numpy(tr), y.shape[0])
    torch.manual_seed(0)
    model = GCN(7, 64, int(y.max()) + 1, 2, y.shape[0], 0.4, "acmgcnpp", 0, attn_layernorm=True)
    _count_passes(model)
    step = T.TrainStep(model, FusedAdamW(model.parameters(), lr=0.01), x, ops, y, w, small_step=False, tape=tape, fused_dropout=False)
    torch.manual_seed(5)
    return step


def test_a_broken_tape_is_redone_once_and_counts_once(monkeypatch):
    _, calls = _install(monkeypatch)
    plain = _broken_tape_step(tape=False)
    want_loss = float(plain())
    step = _broken_tape_step(tape=True)
    calls.clear()
    loss = float(step())
    assert step._tape is False and not step._tape_proven, "the residual add is a torch operation: the tape must have broken"
    assert calls.log == _LAUNCHES["broken-tape"], calls.log
    assert loss == want_loss
    got, want = _state_after(step), _state_after(plain)
    assert _same_state(got, want), (got, want)
    assert float(step.model.passes) == 1.0 and got[1] and set(got[1]) == {1.0}


def test_a_gradient_not_adopted_is_redone_once_and_counts_once(monkeypatch):
    """test_host_stack_cpu's stub: ``all_adopted`` says no once, the step flushes, gives deferral up and runs again."""
    from acm_gnn_amd import functional as AF, tuning
    _, calls = _install(monkeypatch)
    with tuning.override(pipeline=32):
        plain, model, _, _, _ = _headline_step()
        _count_passes(model)
        want_loss = float(plain())
        step, model, _, _, _ = _headline_step()
        _count_passes(model)
        real, asked = AF.DeferredReductions.all_adopted, []
        monkeypatch.setattr(AF.DeferredReductions, "all_adopted", lambda self, t: (asked.append(1), real(self, t) and len(asked) > 1)[1])
        assert step.pipe is not None
        calls.clear()
        loss = float(step())
    assert asked == [1] and step._defer is False and plain._defer is True
    assert calls.log == _LAUNCHES["not-adopted"], calls.log
    np.testing.assert_allclose(loss, want_loss, rtol=1e-5, atol=1e-6)
    got, want = _state_after(step), _state_after(plain)
    assert _same_state(got, want), (got, want)
    assert float(step.model.passes) == 1.0 and set(got[1]) == {1.0} and got[2] == 1


def _wrapper_problem(wrap):
    """The headline model with counter-based masks, bare or behind the thin wrapper, its optimizer advancing the counter."""
    from acm_gnn_amd import FusedAdamW, functional as AF
    model, ops, x, y, w = _setup(dropout=0.3, pattern_only=True, attn_layernorm=True)
    model.fused_dropout, model.dropout_state = True, AF.DropoutState("cpu", seed=3)
    opt = FusedAdamW(model.parameters(), lr=0.01)
    opt.also_advance = model.dropout_state.step
    return (_Wrapper(model) if wrap else model), opt, ops, x, y, w


def _sets(n):
    return [torch.arange(0, n, 3), torch.arange(1, n, 3), torch.arange(2, n, 3)]


@pytest.mark.parametrize("case", ["bce", "wrapper", "wrapper-eval"])
def test_the_launch_sequence_of_a_warm_step(monkeypatch, case):
    from acm_gnn_amd import train as T, tuning
    _, calls = _install(monkeypatch)
    with tuning.override(pipeline=32):
        if case == "bce":
            step = _headline_step(criterion="bce")[0]
        else:
            model, opt, ops, x, y, w = _wrapper_problem(wrap=True)
            step = T.TrainStep(model, opt, x, ops, y, w, small_step=False)
            assert step._tape is True and step.pipe is None
        step(), step()
        if case == "wrapper-eval":
            step = T.EvalStep(model, x, ops, y, _sets(x.shape[0]), small_step=False)
            step()                                               # (the first pass over a static input leaves P for the next)
        calls.clear()
        step()
    assert calls.log == _LAUNCHES[case], (case, calls.log)


def test_a_model_without_the_call_keyword_trains_and_evaluates_as_the_bare_model(monkeypatch):
    """Three eager steps and an evaluation pass through the ambient contexts equal, bit for bit, those of the bare GCN that is
    handed the step's CallContext."""
    from acm_gnn_amd import train as T
    _install(monkeypatch)
    runs = {}
    for wrap in (False, True):
        model, opt, ops, x, y, w = _wrapper_problem(wrap)
        step = T.TrainStep(model, opt, x, ops, y, w, small_step=False)
        losses = [float(step()) for _ in range(3)]
        assert step._defer is True and step._tape is True and step.pipe is None
        logits, accs, val_loss = T.EvalStep(model, x, ops, y, _sets(x.shape[0]), small_step=False)()
        ds = model.dropout_state
        runs[wrap] = (losses, [p.detach().clone() for p in model.parameters()], logits.clone(), accs, val_loss, ds.host_steps, int(ds.step))
    bare, wrapped = runs[False], runs[True]
    assert wrapped[0] == bare[0] and np.isfinite(bare[0]).all()
    assert len(wrapped[1]) == len(bare[1]) and all(torch.equal(a, b) for a, b in zip(wrapped[1], bare[1]))
    assert torch.equal(wrapped[2], bare[2]) and wrapped[3:] == bare[3:] and bare[5] == 3 == bare[6]
