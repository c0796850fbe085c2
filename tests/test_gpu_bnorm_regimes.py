"""The deep mlpX stack (acm_bnorm_*, acm_linear_fwd_shift, acm_gemm_shift) on hidden columns far off centre, on the GPU: every case of
tests/bnorm_regimes.py through functional.residual_mlp (training forward + backward, running buffers, evaluation), every form the
shifted transposed product dispatches to, CSR input, GCN("acmgcnpp", init_layers_X=2) end to end, bit-identical repeats, pitch padding.

The rule is ``bnorm_regimes.compare``: every piece alone against float64, in units of what the textbook form loses in float32 (or
2^-23 of the piece's own terms), no absolute floor, no pooling over columns.  M = 16 is the largest err / unit measured on an MI355X
over all of these cases, rounded up to a power of two: 13.9 in the model case (dbeta of an ordinary column and db_0 of OFF100:
the gradient that reaches the stack there comes out of the ACM layers' own kernels, whose margin is the mixing head's), 7.1 over
the stack's own cases (dgamma of an ordinary column behind an OFF1000 one, L = 3); per kind of piece and column class in
EXPERIMENTS.md ("BatchNorm off centre").  The stack's first form (acm_bnorm_fold / acm_bnorm_param_bwd) -- both products on the uncentred activations,
c = beta - mu a folded into the bias -- measured up to 32.1 on the stack's cases (dgamma RARE2 / RARE3 / ordinary 32.1 / 27.5 / 25.8,
dW_i[k, :] OFF10 / OFF1000 18.3 / 10.5, dgamma OFF1000 17.1, y in evaluation mode 9.7) and fails five of the eight.  Every comparing test prints its figures
before it asserts."""
import functools

import numpy as np
import pytest
import torch

import bnorm_regimes as B
import mlp_stack_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
IDS = [f"{h}-L{L}-p{p}" for h, L, p in B.case_ids()]
STACK_LABELS = {"bnorm_stats", "bnorm_fold", "bnorm_param_bwd", "bnorm_bwd", "linear_fwd", "gemm_TN", "gemm_NN"}      # (linear_fwd: the shifted one too)


def _timed(fn):
    from acm_gnn_amd import functional as AF
    timer = AF.KernelTimer()
    AF.set_kernel_timer(timer)
    try:
        out = fn()
    finally:
        AF.set_kernel_timer(None)
    return out, set(k.split("/")[0] for k in timer.events)


@pytest.mark.parametrize("cid", B.case_ids(), ids=IDS)
def test_residual_mlp_on_every_case(cid):
    case = B.case_of(*cid)
    got, used = _timed(lambda: B.run_stack(case, DEV))
    assert STACK_LABELS <= used and not used & {"bias_act", "bias_act_bwd"}, used
    assert set(got) == set(B.reference(case.key, np.float64)[0])
    B.compare(case, got, B.M, what=f"residual_mlp {cid}", log=print)


def test_csr_input():
    """The first product is acm_spmm_v + acm_bias_act; everything behind the first BatchNorm is the same path."""
    case = B.case_of(64, 2, 0.0)
    got, used = _timed(lambda: B.run_stack(case, DEV, sparse=True))
    assert STACK_LABELS | {"bias_act", "spmm_v"} <= used and "bias_act_bwd" not in used, used
    assert "dX" not in got and "dW0[2,:]" in got
    B.compare(case, got, B.M, what="residual_mlp csr", log=print)


def test_every_form_of_the_shifted_transposed_product(tune):
    """8200 x 64 is past the row-panel threshold: M_c = G^T (H - 1 mu^T) takes the split-bf16 row-panel kernel by default, the tile
    kernel with split-K when that form is switched off, and the tile kernel again where the fp32 row-panel form (which has no
    shifted load) is forced for everything it covers; dZ = G W goes through the split-bf16, row-panel and tile NN kernels
    alongside.  (The 203-row cases reach the unsplit tile kernel only; the shifted forward product is always the tile kernel.)"""
    from acm_gnn_amd import tuning
    case = B.big_case()
    assert case.n == 8200 and set(case.cols) == {"OFF100", "DEAD"} and tuning.kernel()["gemm_forms"] & 7 == 7
    runs = {}
    for name, forms in (("split-bf16", 7), ("tile", 0), ("fp32 row-panel forced", 9)):
        tune(gemm_forms=forms)
        runs[name], used = _timed(lambda: B.run_stack(case, DEV))
        assert STACK_LABELS <= used, used
        B.compare(case, runs[name], B.M, what=f"8200 x 64 {name}", log=print)
    k = case.cols["OFF100"]
    assert not np.array_equal(runs["split-bf16"][f"dgamma0[{k}]"], runs["tile"][f"dgamma0[{k}]"])          # (another kernel did run)
    for piece in (f"dgamma0[{k}]", f"dW1[:,{k}]", "y"):                    # the forced row-panel form leaves the shifted products alone
        assert np.array_equal(runs["fp32 row-panel forced"][piece], runs["tile"][piece]), piece


@pytest.mark.parametrize("n,m,f,forms", [(203, 33, 33, 7), (203, 64, 64, 7), (203, 40, 8, 7), (8200, 64, 64, 7), (8200, 64, 64, 0), (8200, 7, 64, 7),
                                          (16400, 200, 24, 7)])
def test_gemm_shift_alone(n, m, f, forms, tune):
    """acm_gemm_shift against float64 on a B whose columns sit 1, 100 and 10 000 spreads off zero, relative to sum |a| |b - shift|
    (the bound of tests/test_gpu_kernels.py's transposed products); into a pitch-padded destination; the same bits twice."""
    from acm_gnn_amd import functional as AF
    tune(gemm_forms=forms)
    g = torch.Generator().manual_seed(n + m + f)
    a, b = torch.randn(n, m, generator=g), torch.randn(n, f, generator=g)
    shift = torch.tensor([1.0, 100.0, 1e4])[torch.arange(f) % 3] * torch.rand(f, generator=g).add(0.5)
    b = b + shift
    centred = b.double() - shift.double()
    ref, scale = a.double().T @ centred, a.abs().double().T @ centred.abs()
    out = torch.full((m, f + 3), 7.0, device=DEV)
    AF.gemm(a.to(DEV), b.to(DEV), trans_a=True, b_shift=shift.to(DEV), out=out[:, :f])
    err = float(((out[:, :f].cpu().double() - ref).abs() / (scale + 1e-30)).max())
    print(f"gemm_shift {n}x{m}x{f} forms {forms}: {err:.2e}")
    assert err < 3e-6 and bool((out[:, f:] == 7.0).all())
    again = AF.gemm(a.to(DEV), b.to(DEV), trans_a=True, b_shift=shift.to(DEV))
    assert torch.equal(again, out[:, :f])


def test_gemm_shift_refuses_what_no_form_takes():
    from acm_gnn_amd import functional as AF
    a, b = torch.randn(50, 20, device=DEV), torch.randn(20, 30, device=DEV)
    with pytest.raises(RuntimeError, match="acm_gemm_shift"):
        AF.gemm(a, b, b_shift=torch.zeros(30, device=DEV))                # not transposed: ACM_EUNSUPPORTED, never a silent other product


@pytest.mark.parametrize("n,f_in,f_out", [(203, 8, 33), (203, 33, 64), (203, 64, 33), (203, 256, 5)])
def test_linear_fwd_shift_alone_and_its_padding(n, f_in, f_out):
    """(X - 1 shift^T) W^T + b against float64 relative to sum |x - shift| |w| + |b|, X and Y in pitch-padded buffers whose pad
    columns keep their sentinel; f_in = 8 is a width the unshifted entry hands to its narrow streaming kernel."""
    from acm_gnn_amd.functional._launch import _vp, launch
    from acm_gnn_amd.functional.ops import _gemm_workspace
    g = torch.Generator().manual_seed(n + f_in + f_out)
    shift = torch.tensor([1.0, 100.0, 1e4])[torch.arange(f_in) % 3] * torch.rand(f_in, generator=g).add(0.5)
    x = torch.full((n, f_in + 3), 5.0)
    x[:, :f_in] = torch.randn(n, f_in, generator=g) + shift
    w, bias = torch.randn(f_out, f_in, generator=g), torch.randn(f_out, generator=g)
    centred = x[:, :f_in].double() - shift.double()
    ref = centred @ w.double().T + bias.double()
    scale = centred.abs() @ w.double().abs().T + bias.double().abs()
    xd, wd, bd, sd = x.to(DEV), w.to(DEV), bias.to(DEV), shift.to(DEV)
    y = torch.full((n, f_out + 5), 9.0, device=DEV)
    ws, nbytes = _gemm_workspace(xd.device, 0, 1, n, f_out, f_in)
    launch("acm_linear_fwd_shift", None, xd.device, n, f_in, f_out, _vp(xd), xd.stride(0), _vp(sd), _vp(wd), wd.stride(0), _vp(bd), 0, None,
           _vp(y), y.stride(0), _vp(ws), nbytes)
    err = float(((y[:, :f_out].cpu().double() - ref).abs() / scale).max())
    print(f"linear_fwd_shift {n}x{f_in}x{f_out}: {err:.2e}")
    assert err < 3e-6 and bool((y[:, f_out:] == 9.0).all())


@pytest.mark.parametrize("f_out,f_in", [(33, 33), (64, 64), (5, 256)])
def test_fold_and_param_bwd_keep_their_padding(f_out, f_in):
    """acm_bnorm_fold(_centred) and acm_bnorm_param_bwd(_centred) on pitch-padded W, W', M and dW: the formulas of include/acm_hip.h in float64, and
    sentinels in every pad column afterwards."""
    from acm_gnn_amd.functional._launch import _vp, launch
    g = torch.Generator().manual_seed(f_out + f_in)
    pad = lambda t, v: torch.cat([t, torch.full((t.shape[0], 3), v)], 1).to(DEV)     # noqa: E731
    w, m = torch.randn(f_out, f_in, generator=g), torch.randn(f_out, f_in, generator=g)
    bias, s, beta = torch.randn(f_out, generator=g), torch.randn(f_out, generator=g), torch.randn(f_in, generator=g)
    stats = torch.rand(4, f_in, generator=g) + 0.5
    wp, mp = pad(w, 1.5), pad(m, 2.5)
    wf, dw = torch.full((f_out, f_in + 3), 3.5, device=DEV), torch.full((f_out, f_in + 3), 4.5, device=DEV)
    bf, dbeta, dgamma = torch.empty(f_out, device=DEV), torch.empty(f_in, device=DEV), torch.empty(f_in, device=DEV)
    dev = wp.device
    bias_d, s_d, beta_d, stats_d = bias.to(DEV), s.to(DEV), beta.to(DEV), stats.to(DEV)      # (alive until the kernels have run)
    launch("acm_bnorm_fold_centred", None, dev, f_out, f_in, _vp(wp), wp.stride(0), _vp(bias_d), _vp(beta_d), _vp(stats_d), _vp(wf), wf.stride(0),
           _vp(bf))
    launch("acm_bnorm_param_bwd_centred", None, dev, f_out, f_in, _vp(mp), mp.stride(0), _vp(s_d), _vp(wp), wp.stride(0), _vp(beta_d), _vp(stats_d),
           _vp(dw), dw.stride(0), _vp(dbeta), _vp(dgamma))
    w64, m64, st = w.double(), m.double(), stats.double()
    close = lambda got, want: float((got.cpu().double() - want).abs().max()) <= 1e-5 * float(want.abs().max())     # noqa: E731
    assert close(wf[:, :f_in], w64 * st[2]) and close(bf, bias.double() + w64 @ beta.double())
    assert close(dw[:, :f_in], m64 * st[2] + torch.outer(s.double(), beta.double()))
    assert close(dbeta, s.double() @ w64) and close(dgamma, st[1] * (w64 * m64).sum(0))
    assert bool((wf[:, f_in:] == 3.5).all()) and bool((dw[:, f_in:] == 4.5).all())
    assert bool((wp[:, f_in:] == 1.5).all()) and bool((mp[:, f_in:] == 2.5).all())
    # the uncentred pair under its first names: c = stats row 3 in beta's place, dgamma = r (q - mu dbeta)
    launch("acm_bnorm_fold", None, dev, f_out, f_in, _vp(wp), wp.stride(0), _vp(bias_d), _vp(stats_d), _vp(wf), wf.stride(0), _vp(bf))
    launch("acm_bnorm_param_bwd", None, dev, f_out, f_in, _vp(mp), mp.stride(0), _vp(s_d), _vp(wp), wp.stride(0), _vp(stats_d), _vp(dw), dw.stride(0),
           _vp(dbeta), _vp(dgamma))
    assert close(wf[:, :f_in], w64 * st[2]) and close(bf, bias.double() + w64 @ st[3])
    assert close(dw[:, :f_in], m64 * st[2] + torch.outer(s.double(), st[3]))
    assert close(dbeta, s.double() @ w64) and close(dgamma, st[1] * ((w64 * m64).sum(0) - st[0] * (s.double() @ w64)))
    assert bool((wf[:, f_in:] == 3.5).all()) and bool((dw[:, f_in:] == 4.5).all())


@pytest.mark.parametrize("cid", [(33, 3, B.P_DROP), (64, 2, 0.0)], ids=["33-L3-p0.3", "64-L2"])
def test_two_launches_give_the_same_bits(cid):
    case = B.case_of(*cid)
    first, second = B.run_stack(case, DEV), B.run_stack(case, DEV)
    assert set(first) == set(second)
    for name, v in first.items():
        assert np.array_equal(v, second[name]), name


# ---------------------------------------------------------------------------------------------- the model end to end
MODEL_N, MODEL_HIDDEN, MODEL_CLASSES = B.N, 64, 3


def _recording_forward_torch(record):
    """mlp_stack_ref.forward_torch, line by line, keeping the tensors whose gradients are the terms of the per-column sums."""
    def forward_torch(x, lins, bns, eps=R.EPS):
        z = x
        for (w, b), (gamma, beta) in zip(lins[:-1], bns):
            pre = z @ w.T + b
            h = torch.relu(pre)
            xhat = (h - h.mean(0)) / torch.sqrt(h.var(0, unbiased=False) + eps)
            z = xhat * gamma + beta
            pre.retain_grad()
            z.retain_grad()
            record.update(pre=pre, xhat=xhat, z=z)
        return z @ lins[-1][0].T + lins[-1][1]
    return forward_torch


@functools.lru_cache(maxsize=None)
def _model_problem():
    """GCN("acmgcnpp", init_layers_X=2) on 203 nodes with mlpX.lins.0's bias rows edited as bnorm_regimes edits a first layer, and
    the biases of its two Linears settled off the ReLUs' rounding noise; parameters as float64 CPU tensors."""
    from acm_gnn_amd import GCN
    from oracle import acm_oracle as O
    from test_gpu_mlp_stack import _graph
    low, high, _ = O.filters_linkx(_graph(MODEL_N, 9))
    g = torch.Generator().manual_seed(2)
    x = torch.randn(MODEL_N, B.F_IN, generator=g)
    y = torch.randint(0, MODEL_CLASSES, (MODEL_N,), generator=g)
    torch.manual_seed(5)
    model = GCN(B.F_IN, MODEL_HIDDEN, MODEL_CLASSES, 2, MODEL_N, 0.0, "acmgcnpp", 0, variant=False, attn_layernorm=True, init_layers_X=2)
    with torch.no_grad():
        model.mlpX.bns[0].weight.uniform_(0.5, 1.5)
        model.mlpX.bns[0].bias.uniform_(-0.5, 0.5)
        lins = [[lin.weight.detach().numpy().copy(), lin.bias.detach().numpy().copy()] for lin in model.mlpX.lins]
        bns = [(model.mlpX.bns[0].weight.detach().numpy().copy(), model.mlpX.bns[0].bias.detach().numpy().copy())]
        cols = B.columns(MODEL_HIDDEN)
        B._edit_layer(x.numpy().astype(np.float64), lins[0][0], lins[0][1], cols)
        B._settle(x.numpy(), lins, bns, cols)
        for lin, (w, b) in zip(model.mlpX.lins, lins):
            lin.weight.copy_(torch.from_numpy(w))
            lin.bias.copy_(torch.from_numpy(b))
    return model, x, y, torch.arange(0, MODEL_N, 2), low, high, cols


@functools.lru_cache(maxsize=None)
def _model_reference(dtype):
    """{piece: value} (and, in float64, {piece: floor}) of tests/test_gpu_mlp_stack.py::_oracle_logits under the mean NLL."""
    from oracle import acm_oracle as O
    import test_gpu_mlp_stack as T
    model, x, y, idx, low, high, cols = _model_problem()
    params = {k: v.detach().cpu().to(dtype).clone().requires_grad_(True) for k, v in model.named_parameters() if k not in ("fea_param", "xX_param")}
    record = {}
    saved, threads = R.forward_torch, torch.get_num_threads()
    R.forward_torch = _recording_forward_torch(record)
    torch.set_num_threads(1)                       # (the float32 oracle's error is the unit: the same sum order wherever this runs)
    try:
        logits = T._oracle_logits(params, x.to(dtype), low.to(dtype), high.to(dtype), 0.0, {})
        O.nll_loss_on(logits, y, idx).backward()
    finally:
        R.forward_torch = saved
        torch.set_num_threads(threads)
    grads = {k: v.grad.double().numpy() for k, v in params.items() if k.startswith("mlpX.")}
    out, floors = _model_pieces(logits.detach().double().numpy(), grads), {}
    g0, dz, xhat = record["pre"].grad.double().numpy(), record["z"].grad.double().numpy(), record["xhat"].detach().double().numpy()
    for k in range(MODEL_HIDDEN):
        floors[f"mlpX.lins.0.bias[{k}]"] = B.EPS32 * float(np.abs(g0[:, k]).sum())
        floors[f"mlpX.bns.0.weight[{k}]"] = B.EPS32 * float(np.abs(dz[:, k] * xhat[:, k]).sum())
        floors[f"mlpX.bns.0.bias[{k}]"] = B.EPS32 * float(np.abs(dz[:, k]).sum())
    for name, v in out.items():
        floors.setdefault(name, B.EPS32 * float(np.abs(v).max(initial=0.0)))
    return out, floors


def _model_pieces(logits, grads):
    out = {"logits": logits, "mlpX.lins.1.bias": grads["mlpX.lins.1.bias"]}
    for k in range(MODEL_HIDDEN):
        out[f"mlpX.lins.1.weight[:,{k}]"] = grads["mlpX.lins.1.weight"][:, k]
        out[f"mlpX.lins.0.weight[{k},:]"] = grads["mlpX.lins.0.weight"][k, :]
        for name in ("mlpX.lins.0.bias", "mlpX.bns.0.weight", "mlpX.bns.0.bias"):
            out[f"{name}[{k}]"] = np.asarray(grads[name][k])
    return {k: np.asarray(v, np.float64) for k, v in out.items()}


def test_acmgcnpp_end_to_end():
    import copy
    from acm_gnn_amd.graph import clear_cache
    clear_cache()
    model, x, y, idx, low, high, cols = _model_problem()
    ref64, floors = _model_reference(torch.float64)
    ref32, _ = _model_reference(torch.float32)
    h = torch.relu(x.double() @ model.mlpX.lins[0].weight.double().T + model.mlpX.lins[0].bias.double())
    ratio = (h.mean(0) / h.std(0, unbiased=False))[[cols["OFF10"], cols["OFF100"], cols["OFF1000"]]]
    assert torch.allclose(ratio, torch.tensor([10.0, 100.0, 1000.0], dtype=torch.float64), rtol=0.1) and bool((h[:, cols["DEAD"]] == 0).all())
    dev_model = copy.deepcopy(model).to(DEV).train()
    lowd, highd, idxd = low.to(DEV), high.to(DEV), idx.to(DEV)

    def run():
        out = dev_model(x.to(DEV), lowd, highd, None)
        torch.nn.functional.nll_loss(torch.log_softmax(out, 1)[idxd], y.to(DEV)[idxd]).backward()
        return out
    out, used = _timed(run)
    assert {"bnorm_stats", "bnorm_fold", "bnorm_param_bwd", "bnorm_bwd", "linear_fwd"} <= used and "bias_act_bwd" not in used, used
    grads = {k: p.grad.detach().cpu().double().numpy() for k, p in dev_model.named_parameters() if k.startswith("mlpX.")}
    got = _model_pieces(out.detach().cpu().double().numpy(), grads)
    table = B.ratios(got, ref64, floors, ref32)
    name, (err, unit, worst) = max(table.items(), key=lambda kv: kv[1][2])
    print(f"BNREG model | worst {name} err {err:.3e} unit {unit:.3e} ratio {worst:.2f} | logits ratio {table['logits'][2]:.2f}")
    bad = {k: v for k, v in table.items() if not v[2] <= B.M}
    assert not bad, {k: (f"{e:.3e}", f"{u:.3e}", f"{r:.1f}") for k, (e, u, r) in sorted(bad.items(), key=lambda kv: -kv[1][2])[:12]}
