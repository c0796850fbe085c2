"""Masked BCE-with-logits on one-hot labels (acm_bce_loss, ABI 29) on the MI355X: the kernel against float64 torch, the autograd
Function and its deferred second phase, and TrainStep(criterion="bce") against autograd, across its three step forms."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _case(n, c, seed):
    """Logits randn * 4 with 16 entries at +/- 100; a third of the rows have weight 0 and label -1; a few weighted rows carry
    the label C (the all-zero target)."""
    g = torch.Generator().manual_seed(seed)
    z = torch.randn(n, c, generator=g) * 4
    flat = z.view(-1)
    where = torch.randperm(flat.numel(), generator=g)[:16]
    flat[where] = torch.where(torch.arange(where.numel()) % 2 == 0, 100.0, -100.0)
    y = torch.randint(0, c, (n,), generator=g)
    off = torch.rand(n, generator=g) < 1 / 3
    if n >= 3:
        off[0], off[1] = False, True
    w = torch.rand(n, generator=g) / n + 1.0 / n
    w[off] = 0.0
    y[off] = -1
    on = (~off).nonzero().view(-1)
    y[on[:: max(on.numel() // 3, 1)][:4]] = c
    return z, y, w


def _reference(z, y, w):
    zd = z.double().requires_grad_(True)
    c = z.shape[1]
    target = (y.view(-1, 1) == torch.arange(c).view(1, -1)).double()          # -1 and C: all zeros
    per_row = F.binary_cross_entropy_with_logits(zd, target, reduction="none").mean(1)
    loss = (w.double() * per_row).sum()
    loss.backward()
    return float(loss.detach()), zd.grad


@pytest.mark.parametrize("n,c", [(5, 2), (257, 3), (2708, 7), (300, 64), (262_444, 2)])
def test_bce_kernel_against_float64_torch(n, c):
    from acm_gnn_amd import functional as AF
    z, y, w = _case(n, c, n + c)
    want_loss, want_dz = _reference(z, y, w)
    zd, yd, wd = z.to(DEV), y.to(DEV), w.to(DEV)
    loss, dz = AF.bce_loss_and_grad(zd, yd, wd)
    got_loss, got = float(loss), dz.cpu()
    err = (got.double() - want_dz).abs()
    bound = (2e-6 * w.double() / c).view(-1, 1)
    print(f"n={n} C={c}: loss {got_loss!r} vs {want_loss!r} (rel {abs(got_loss - want_loss) / abs(want_loss):.2e}); "
          f"max dz error / bound {float((err / bound.clamp_min(1e-300)).max()):.3f}")
    assert abs(got_loss - want_loss) <= 5e-6 * abs(want_loss)
    assert bool((err <= bound).all())
    assert bool((got[w == 0] == 0).all()) and bool(torch.isfinite(got).all()) and np.isfinite(got_loss)
    # a column slice of a wider buffer as logits, and a strided gradient buffer
    wide = torch.full((n, c + 5), 7.0, device=DEV)
    wide[:, 2:2 + c] = zd
    grad_buf = torch.full((n, c + 3), -3.0, device=DEV)
    loss_s, dz_s = AF.bce_loss_and_grad(wide[:, 2:2 + c], yd, wd, out=grad_buf[:, 1:1 + c])
    assert dz_s.data_ptr() == grad_buf[:, 1:1 + c].data_ptr()
    assert float(loss_s) == got_loss and torch.equal(dz_s.cpu(), got)
    assert bool((grad_buf[:, 0] == -3.0).all()) and bool((grad_buf[:, 1 + c:] == -3.0).all())
    # loss only: the same bits; reruns: the same bits
    assert float(AF.bce_loss(zd, yd, wd)) == got_loss
    for _ in range(3):
        l2, d2 = AF.bce_loss_and_grad(zd, yd, wd)
        assert float(l2) == got_loss and torch.equal(d2.cpu(), got)


def test_masked_bce_function_and_deferred_loss():
    from acm_gnn_amd import functional as AF
    z, y, w = _case(1000, 3, 11)
    _, want_dz = _reference(z, y, w)
    zd = z.to(DEV).requires_grad_(True)
    loss = AF.masked_bce(zd, y.to(DEV), w.to(DEV))
    (loss * 1.5).backward()
    bound = (1.5 * 2e-6 * w.double() / 3).view(-1, 1) + 1e-12
    assert bool(((zd.grad.cpu().double() - 1.5 * want_dz).abs() <= bound).all())
    now = float(loss.detach())
    with AF.deferred_reductions() as pending:
        later = AF.masked_bce(zd.detach(), y.to(DEV), w.to(DEV))
        assert pending.pending >= 1
    assert float(later) == now                               # the flush at the end of the block: the same tree, the same bits


def _tiny(seed=1):
    from acm_gnn_amd import data as D, train as T
    from acm_gnn_amd.graph import CsrGraph, FilterOperators
    adj, x_np, y_np, (tr, va, te), _ = D.synthetic_dataset("tiny", seed=seed)
    low, deg = D.build_filters(adj)
    ops = FilterOperators(CsrGraph.from_scipy(low, DEV))
    x, y = torch.from_numpy(D.row_normalize_features(x_np)).to(DEV), torch.from_numpy(y_np).to(DEV)
    idx = torch.from_numpy(tr).to(DEV)
    return ops, x, y, idx, T.row_weights(idx, x.shape[0])


def _model():
    from acm_gnn_amd import GCN
    torch.manual_seed(0)
    return GCN(7, 64, 2, 2, 2000, 0.0, "acmgcnp", 0, variant=False).to(DEV)


def test_train_step_bce_first_step_matches_autograd():
    from acm_gnn_amd import FusedAdamW, train as T
    from acm_gnn_amd.graph import clear_cache
    clear_cache()
    ops, x, y, idx, w = _tiny()
    ref_model = _model()
    ref_model.train()
    out = ref_model(x, ops, None, None)
    ref_loss = F.binary_cross_entropy_with_logits(out[idx], F.one_hot(y, 2)[idx].float())
    ref_loss.backward()
    want = {k: p.grad.detach().clone() for k, p in ref_model.named_parameters() if p.grad is not None}
    del out
    model = _model()
    step = T.TrainStep(model, FusedAdamW(model.parameters(), lr=0.01, weight_decay=1e-3), x, ops, y, w, criterion="bce")
    assert step.small is None and step.criterion == "bce"
    loss = step._forward_backward()                          # gradients and loss complete on return, no update
    # both losses are fp32 sums of the same 2000 x 2 terms in different orders
    assert abs(float(loss) - float(ref_loss)) <= 1e-5 * abs(float(ref_loss)), (float(loss), float(ref_loss))
    assert len(want) >= 10
    for k, p in model.named_parameters():
        if k not in want:
            assert p.grad is None, k
            continue
        tol = 1e-4 * max(1.0, float(want[k].abs().max()))               # test_gpu_oracle.py's rule for this model
        assert float((p.grad - want[k]).abs().max()) < tol, k


def test_train_step_bce_tape_autograd_and_captured_agree():
    from acm_gnn_amd import FusedAdamW, train as T
    from acm_gnn_amd.graph import clear_cache
    clear_cache()
    ops, x, y, idx, w = _tiny()
    losses = {}
    for form, kw in (("tape", {}), ("autograd", dict(tape=False)), ("graph", dict(use_graph=True))):
        model = _model()
        step = T.TrainStep(model, FusedAdamW(model.parameters(), lr=0.01, weight_decay=1e-3), x, ops, y, w, criterion="bce", **kw)
        losses[form] = [float(step()) for _ in range(5)]
        assert step.small is None
    assert losses["tape"] == losses["autograd"]              # the same kernels in the same order: the same bits
    np.testing.assert_allclose(losses["graph"], losses["tape"], rtol=1e-5)      # test_graph_replayed_step_equals_eager's rule
    assert losses["tape"][-1] < losses["tape"][0]


def test_small_plan_is_refused_for_bce_and_nll_is_untouched():
    import scipy.sparse as sp
    from acm_gnn_amd import FusedAdam, GCN, SparseFeatures, data as D, train as T
    from acm_gnn_amd.distributed import make_sharded_operators
    from acm_gnn_amd.graph import clear_cache
    clear_cache()
    rng = np.random.default_rng(0)
    n, f_in, ncls = 2708, 300, 7                             # Cora-sized, CSR features: where criterion="nll" gets the small plan
    a = sp.random(n, n, density=0.0015, random_state=rng, format="csr")
    a = sp.csr_matrix(((a + a.T) > 0).astype(np.float32))
    low, deg = D.build_filters(a)
    ops = make_sharded_operators(low, deg, torch.device(DEV))
    x_np = (rng.random((n, f_in)) < 0.02).astype(np.float32)
    xs = SparseFeatures.from_scipy(sp.csr_matrix(x_np), DEV)
    y = torch.from_numpy(rng.integers(0, ncls, n)).to(DEV)
    w = T.row_weights(torch.arange(0, n, 2, device=DEV), n)
    steps = {}
    for name, kw in (("default", {}), ("nll", dict(criterion="nll")), ("bce", dict(criterion="bce"))):
        torch.manual_seed(0)
        model = GCN(f_in, 64, ncls, 2, n, 0.0, "acmgcn", 0, variant=False).to(DEV)
        steps[name] = T.TrainStep(model, FusedAdam(model.parameters(), lr=0.01), xs, ops, y, w, **kw)
    assert steps["default"].small is not None and steps["nll"].small is not None, steps["nll"].small_refused
    assert steps["bce"].small is None and "bce" in steps["bce"].small_refused
    a_, b_ = [float(steps["default"]()) for _ in range(3)], [float(steps["nll"]()) for _ in range(3)]
    assert a_ == b_                                          # the keyword's default changes nothing: the same bits
    assert np.isfinite(float(steps["bce"]()))
    with pytest.raises(ValueError, match="criterion"):
        T.TrainStep(model, FusedAdam(model.parameters(), lr=0.01), xs, ops, y, w, criterion="mse")
