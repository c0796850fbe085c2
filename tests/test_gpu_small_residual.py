"""ACM-GCN++ (``GCN(..., "acmgcnpp", init_layers_X=1)``) on the fused small-graph step: seven launches (evaluation: four) --
csrc/acm_small.hip's launch 0 and the residual forms of launches 1, 2, 4 and 6 -- against the float64 oracle
(``oracle.acm_oracle.gcn_forward(model_type="acmgcnpp")`` with the three dropout masks regenerated: tag 0 on the stored
feature values, tags 1 and 2 on [n, hidden]) and against the general path of the library; the evaluation pass, ``fit`` with
``keep_best``, determinism, a model without the branch, and the refusals.  Every training test first asserts that the small
path was taken (``SmallPlan.why_not(...) is None``, ``step.small is not None``): none passes by running the general path twice."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp
import torch

from oracle import acm_oracle as O
from oracle.philox import dropout_factors
from test_gpu_small import GRAPHS, _case, _filters64, _runs_agree

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SEED, STEP = 0x1234ABCD5678, 5
# (variant, structure_info, attn_layernorm)
CELLS = [(0, 0, False), (1, 0, False), (0, 1, True), (1, 1, True), (0, 0, True)]
_cell_id = lambda c: f"v{c[0]}s{c[1]}ln{int(c[2])}"                                  # noqa: E731


def _model(case, f_in, classes, cell, hidden, p_drop, seed=0, **kw):
    from acm_gnn_amd import GCN, functional as AF
    v, s, ln = cell
    torch.manual_seed(seed)
    model = GCN(f_in, hidden, classes, 2, case["n"], p_drop, "acmgcnpp", s, variant=bool(v), attn_layernorm=ln, **kw).to(DEV)
    with torch.no_grad():                             # LayerNorm parameters away from (1, 0): their gradients must be live
        for name, p in model.named_parameters():
            if "layer_norm" in name:
                p.add_(0.3 * torch.randn_like(p))
    if p_drop > 0:
        model.fused_dropout = True
        model.dropout_state = AF.DropoutState(torch.device(DEV), seed=SEED)
        model.dropout_state.step.fill_(STEP)
    return model


def _masks(case, hidden, p_drop):
    """The three keep-masks of one step as the kernels draw them: tag 0 on the nnz(X) stored values (element (position, 0)),
    tags 1 and 2 on [n, hidden]."""
    n = case["n"]
    xs = sp.csr_matrix(case["x_np"])
    xs.sort_indices()
    fx = dropout_factors(SEED, STEP, 0, p_drop, xs.nnz, 1)[:, 0]
    mx = np.zeros(case["x_np"].shape)
    mx[np.repeat(np.arange(n), np.diff(xs.indptr)), xs.indices] = (fx > 0)
    mh = (dropout_factors(SEED, STEP, 1, p_drop, n, hidden) > 0).astype(np.float64)
    mr = (dropout_factors(SEED, STEP, 2, p_drop, n, hidden) > 0).astype(np.float64)
    return mx, mh, mr


def _oracle_step(case, model, cell, hidden, p_drop):
    """loss, logits, gradients of one training step by the float64 oracle (test_gpu_small._oracle_step, with the residual
    branch's parameters and its mask)."""
    v, s, ln = cell
    params = {k: t.detach().cpu().double().requires_grad_(True) for k, t in model.state_dict().items()
              if k.startswith("gcns.") or k.startswith("mlpX.lins.0.")}
    assert {"mlpX.lins.0.weight", "mlpX.lins.0.bias"} <= set(params)
    low_t, high_t, un_t = _filters64(case["adj"])
    x = torch.from_numpy(case["x_np"]).double()
    masks = None
    if p_drop > 0:
        mx, mh, mr = _masks(case, hidden, p_drop)
        # every column of the residual's mask keeps some rows and drops some, and it is not the hidden layer's mask
        assert (mr.sum(0) > 0).all() and (mr.sum(0) < case["n"]).all() and not np.array_equal(mr, mh)
        masks = {"x": torch.from_numpy(mx), "hidden": torch.from_numpy(mh), "xX": torch.from_numpy(mr)}
    p_eff = float(np.float32(1.0) - np.float32(1.0) / (np.float32(1.0) / (np.float32(1.0) - np.float32(p_drop)))) if p_drop > 0 else 0.0
    out = O.gcn_forward(params, x, low_t, high_t, un_t if s else None, model_type="acmgcnpp", variant=v, structure_info=s,
                        attn_layernorm=ln, dropout=p_eff, training=True, masks=masks)
    loss = O.nll_loss_on(out, torch.from_numpy(case["y"]), torch.from_numpy(case["tr"]))
    loss.backward()
    return float(loss), out.detach(), {k: t.grad for k, t in params.items()}


def _ref_key(key):
    li, name = key
    return f"mlpX.lins.0.{name}" if li == "mlpX" else f"gcns.{li}.{name}"


def _check_one_step(case, f_in, classes, cell, hidden, p_drop, edit=None):
    from acm_gnn_amd import train as T
    from acm_gnn_amd.small import SmallPlan
    model = _model(case, f_in, classes, cell, hidden, p_drop)
    if edit is not None:
        edit(model)
    model.train()
    assert SmallPlan.why_not(model, case["xs"], case["ops"]) is None
    y = torch.from_numpy(case["y"]).to(DEV)
    w = T.row_weights(torch.from_numpy(case["tr"]).to(DEV), case["n"])
    plan = SmallPlan(model, case["xs"], case["ops"], y, w, optimizer=None, update=False)
    assert plan.residual and plan.p.residual == 1
    assert ("mlpX", "weight") in plan.grads and ("mlpX", "bias") in plan.grads
    loss = float(plan.run())
    torch.cuda.synchronize()
    ref_loss, ref_out, ref_grads = _oracle_step(case, model, cell, hidden, p_drop)
    figures = [("loss", abs(loss - ref_loss), 2e-5 * abs(ref_loss) + 1e-6)]
    scale = float(ref_out.abs().max()) + 1e-6
    figures.append(("logits", float((plan.logits.cpu() - ref_out).abs().max()), 2e-5 * scale + 1e-5))
    for key, g in plan.grads.items():
        ref = ref_grads[_ref_key(key)]
        assert ref is not None, key
        figures.append((key, float((g.cpu() - ref).abs().max()), 2e-4 * float(ref.abs().max()) + 1e-7))
    print("\n".join(f"{k}: err {e:.3e} tol {t:.3e}" for k, e, t in figures))
    np.testing.assert_allclose(loss, ref_loss, rtol=2e-5, atol=1e-6)
    bad = [(k, e, t) for k, e, t in figures[1:] if not e <= t]
    assert not bad, bad
    return plan, ref_grads


@pytest.mark.parametrize("p_drop", [0.0, 0.5], ids=["nodrop", "drop"])
@pytest.mark.parametrize("hidden", [32, 64])
@pytest.mark.parametrize("cell", CELLS, ids=_cell_id)
def test_one_step_matches_the_float64_oracle(cell, hidden, p_drop):
    adj, f_in, classes = GRAPHS["eight"]()
    assert (adj.shape[0], f_in, classes) == (300, 64, 8)
    plan, ref_grads = _check_one_step(_case(adj, f_in, classes, seed=11, s=cell[1]), f_in, classes, cell, hidden, p_drop)
    assert float(ref_grads["mlpX.lins.0.weight"].abs().max()) > 0 and float(ref_grads["mlpX.lins.0.bias"].abs().max()) > 0


def _edge_case(f_in, classes, s):
    """The "pieces" graph (700 nodes, a hub of 600 neighbours: a long row of the operator, whose record in launch 4 carries
    db_X) with: node 3 without features (xX = drop(relu(b_X))), node 5 with EVERY feature and feature 2 on EVERY node (both
    longer than the feature handles' chunk: the fourth sum goes through the slot buffer in launches 1 and 6), and feature
    columns 0, 1 and the last without an entry."""
    adj, _, _ = GRAPHS["pieces"]()
    n = adj.shape[0]
    rng = np.random.default_rng(23)
    x_np = (rng.random((n, f_in)) < 0.02).astype(np.float32) * rng.uniform(0.5, 1.5, (n, f_in)).astype(np.float32)
    x_np[5] = rng.uniform(0.5, 1.5, f_in)
    x_np[:, 2] = rng.uniform(0.5, 1.5, n)
    x_np[:, [0, 1, f_in - 1]] = 0.0
    case = _case(adj, f_in, classes, seed=11, s=s, x_np=x_np)
    x_np = case["x_np"]
    assert not x_np[3].any() and not x_np[:, [0, 1, f_in - 1]].any()
    return case


def _edit_bias(model):
    """Some columns of b_X dead for every row, some alive for every row."""
    with torch.no_grad():
        b = model.mlpX.lins[0].bias
        b[1::5] = -50.0
        b[3::5] = 50.0


@pytest.mark.parametrize("f_in,classes,hidden,cell", [(67, 3, 64, (0, 1, True)), (67, 8, 32, (1, 0, False)), (600, 8, 64, (1, 1, True)),
                                                      (600, 3, 32, (0, 0, False))],
                         ids=["f67_c3_h64", "f67_c8_h32", "f600_c8_h64", "f600_c3_h32"])
def test_the_shapes_where_it_can_go_wrong(f_in, classes, hidden, cell):
    case = _edge_case(f_in, classes, cell[1])
    if f_in == 600:
        assert case["xs"].csr.n_long_rows > 0 and case["xs"].csr_t.n_long_rows > 0       # node 5's row, feature 2's column
    else:
        assert case["xs"].csr_t.n_long_rows > 0                                           # feature 2's column (700 entries)
    plan, ref_grads = _check_one_step(case, f_in, classes, cell, hidden, 0.5, edit=_edit_bias)
    assert plan.low.n_long_rows > 0                                                       # the hub
    gw, gb = ref_grads["mlpX.lins.0.weight"], ref_grads["mlpX.lins.0.bias"]
    assert not gw[:, [0, 1, f_in - 1]].any() and not plan.grads[("mlpX", "weight")][:, [0, 1, f_in - 1]].any()
    assert not gb[1::5].any() and not plan.grads[("mlpX", "bias")][1::5].any()            # dead for every row
    assert gb[3::5].abs().min() > 0


@pytest.mark.parametrize("use_graph", [False, True], ids=["eager", "graph"])
@pytest.mark.parametrize("decoupled", [False, True], ids=["adam", "adamw"])
def test_training_run_equals_the_general_path(decoupled, use_graph):
    """12 steps of TrainStep on the small path against TrainStep(small_step=False): same seeds, same masks, the same optimizer
    arithmetic -- parameters, both moments and the step counts of every tensor (mlpX's two among them) and the dropout
    counter.  Feature column 0 is empty: with weight decay its column of W_X still moves, as FusedAdam.step moves it."""
    from acm_gnn_amd import FusedAdam, FusedAdamW, functional as AF, train as T
    from acm_gnn_amd.small import SmallPlan
    cell, p_drop = ((0, 1, True) if decoupled else (1, 0, False)), 0.5
    # The graph and features of test_gpu_small.test_training_run_equals_the_general_path ("pieces": a hub row cut into pieces;
    # 300 features at 1 % density), with feature column 0 emptied.  NOT _edge_case's node that carries every feature: its
    # first-layer row is ~100 times any other node's, so one ReLU of that row flipping on a 1e-5 parameter difference (Adam
    # turns a gradient element of 1e-9 with 0.5 % summation-order error into exactly that) changes a whole column of dW1 --
    # measured: the two paths agree to 7 digits for five steps, then part at the sixth.  One step on that node is pinned
    # against the oracle above; a twelve-step comparison of two correct fp32 implementations needs inputs that do not
    # amplify their last bits.
    adj, f_in, classes = GRAPHS["pieces"]()
    rng = np.random.default_rng(5)
    x_np = (rng.random((adj.shape[0], f_in)) < 0.01).astype(np.float32) * rng.uniform(0.5, 1.5, (adj.shape[0], f_in)).astype(np.float32)
    x_np[:, 0] = 0.0
    case = _case(adj, f_in, classes, seed=5, s=cell[1], x_np=x_np)
    assert not case["x_np"][:, 0].any()
    y = torch.from_numpy(case["y"]).to(DEV)
    w = T.row_weights(torch.from_numpy(case["tr"]).to(DEV), case["n"])

    def run(small):
        model = _model(case, f_in, classes, cell, 64, p_drop, seed=3)
        model.dropout_state = AF.DropoutState(torch.device(DEV), seed=77)
        opt = (FusedAdamW if decoupled else FusedAdam)(model.parameters(), lr=0.02, weight_decay=5e-3)
        if small:
            assert SmallPlan.why_not(model, case["xs"], case["ops"], opt) is None
        step = T.TrainStep(model, opt, case["xs"], case["ops"], y, w, use_graph=use_graph, small_step=None if small else False)
        assert (step.small is not None) == small, step.small_refused
        w0 = model.mlpX.lins[0].weight.detach().clone()
        losses = [float(step()) for _ in range(12)]
        return model, opt, losses, w0

    ma, oa, la, w0 = run(True)
    mb, ob, lb, _ = run(False)
    np.testing.assert_allclose(la, lb, rtol=3e-5, atol=1e-6)
    _runs_agree(ma, oa, mb, ob, 12, p_drop)
    for name in ("weight", "bias"):
        ta, tb = getattr(ma.mlpX.lins[0], name), getattr(mb.mlpX.lins[0], name)
        assert float(oa.state[ta]["step"]) == float(ob.state[tb]["step"]) == 12.0
        torch.testing.assert_close(oa.state[ta]["exp_avg_sq"], ob.state[tb]["exp_avg_sq"], rtol=5e-3, atol=1e-9)
    # the empty feature column: a zero gradient, and still its weight-decay update -- equal on both paths
    wa, wb = ma.mlpX.lins[0].weight, mb.mlpX.lins[0].weight
    assert not torch.equal(wa[:, 0], w0[:, 0])
    torch.testing.assert_close(wa[:, 0], wb[:, 0], rtol=1e-5, atol=1e-8)       # (12 steps of a few fp32 roundings each)
    for k in ("exp_avg", "exp_avg_sq"):
        assert float(oa.state[wa][k][:, 0].abs().max()) <= (0.0 if decoupled else 1e-3)
        torch.testing.assert_close(oa.state[wa][k][:, 0], ob.state[wb][k][:, 0], rtol=1e-5, atol=1e-12)


def test_evaluation_pass_and_fit_with_keep_best():
    from acm_gnn_amd import FusedAdamW, functional as AF, train as T, tuning
    adj, f_in, classes = GRAPHS["eight"]()
    cell = (0, 1, True)
    case = _case(adj, f_in, classes, seed=9, s=1)
    n = case["n"]
    y = torch.from_numpy(case["y"]).to(DEV)
    idx = torch.randperm(n, generator=torch.Generator().manual_seed(0)).to(DEV)
    sets = (idx[: n // 2], idx[n // 2: 3 * n // 4], idx[3 * n // 4:])
    model = _model(case, f_in, classes, cell, 64, 0.5)
    ev_s = T.EvalStep(model, case["xs"], case["ops"], y, sets)
    ev_g = T.EvalStep(model, case["xs"], case["ops"], y, sets, small_step=False)
    ev_c = T.EvalStep(model, case["xs"], case["ops"], y, sets, use_graph=True)
    assert ev_s.small is not None and ev_s.small.residual and ev_g.small is None and ev_c.small is not None
    (o1, a1, l1), (o2, a2, l2), (o3, a3, l3) = ev_s(), ev_g(), ev_c()
    assert float((o1 - o2).abs().max()) <= 2e-5 * (float(o2.abs().max()) + 1e-6) + 1e-5
    assert torch.equal(o1, o3) and a1 == a3

    def fit(small):
        m = _model(case, f_in, classes, cell, 64, 0.5, seed=4)
        m.dropout_state = AF.DropoutState(torch.device(DEV), seed=5)
        opt = FusedAdamW(m.parameters(), lr=0.01, weight_decay=1e-3)
        with tuning.override(small_step=16384 if small else 0):
            sel, hist = T.fit(m, opt, case["xs"], case["ops"], y, *sets, epochs=12, use_graph=True, sync_every=32, keep_best=True)
        return m, sel, hist

    ma, sel_a, hist_a = fit(True)
    _, sel_b, hist_b = fit(False)
    assert len(hist_a) == len(hist_b) == 12
    np.testing.assert_allclose([h[0] for h in hist_a], [h[0] for h in hist_b], rtol=5e-4)
    np.testing.assert_allclose([h[4] for h in hist_a], [h[4] for h in hist_b], rtol=5e-4)
    assert abs(sel_a - sel_b) <= 0.02
    # the model left behind is the selected epoch's, mlpX's two tensors included: it evaluates to the reported accuracy
    ev = T.EvalStep(ma, case["xs"], case["ops"], y, sets)
    assert ev.small is not None
    _, accs, _ = ev()
    assert abs(accs[2] - sel_a) < 1e-6


def test_the_step_is_deterministic_and_the_replay_equals_the_eager_call():
    from acm_gnn_amd import FusedAdamW, functional as AF, train as T
    cell, f_in, classes = (0, 1, True), 300, 3
    case = _edge_case(f_in, classes, 1)
    y = torch.from_numpy(case["y"]).to(DEV)
    w = T.row_weights(torch.from_numpy(case["tr"]).to(DEV), case["n"])

    def run(use_graph):
        model = _model(case, f_in, classes, cell, 64, 0.6, seed=3)
        model.dropout_state = AF.DropoutState(torch.device(DEV), seed=77)
        opt = FusedAdamW(model.parameters(), lr=0.02, weight_decay=5e-3)
        step = T.TrainStep(model, opt, case["xs"], case["ops"], y, w, use_graph=use_graph)
        assert step.small is not None and step.small.residual and step.small.low.n_long_rows > 0
        losses = [float(step()) for _ in range(8)]
        state = [p.detach().clone() for p in model.parameters()]
        for p in model.parameters():
            st = opt.state.get(p, {})
            state += [st[k].detach().clone() for k in ("exp_avg", "exp_avg_sq", "step") if k in st]
        return losses, state

    la, sa = run(False)
    for use_graph in (False, True):
        lb, sb = run(use_graph)
        assert la == lb and len(sa) == len(sb)
        for u, v in zip(sa, sb):
            assert torch.equal(u, v)


def test_a_model_without_the_branch_plans_as_before():
    from acm_gnn_amd import GCN, FusedAdam, _lib, train as T
    from acm_gnn_amd.small import SmallPlan
    adj, f_in, classes = GRAPHS["eight"]()
    case = _case(adj, f_in, classes, seed=11, s=0)
    torch.manual_seed(0)
    model = GCN(f_in, 64, classes, 2, case["n"], 0.0, "acmgcnp", 0).to(DEV)
    opt = FusedAdam(model.parameters(), lr=0.01)
    y = torch.from_numpy(case["y"]).to(DEV)
    w = T.row_weights(torch.from_numpy(case["tr"]).to(DEV), case["n"])
    plan = SmallPlan(model, case["xs"], case["ops"], y, w, opt)
    assert not plan.residual and plan.p.residual == 0 and plan.p.res[0].param is None and plan.p.drop_res.p == 0
    nbytes, with_res = C.c_size_t(), C.c_size_t()
    lib = _lib.load()
    handles = (plan.low.handle, case["xs"].csr.handle, case["xs"].csr_t.handle)
    assert lib.acm_small_step_workspace_bytes(*handles, C.byref(nbytes)) == 0
    assert plan.workspace.numel() * 4 == nbytes.value
    shape = _lib.SmallStep()
    shape.f_in = f_in
    assert lib.acm_small_step_workspace_bytes_for(*handles, C.byref(shape), C.byref(with_res)) == 0 and with_res.value == nbytes.value
    shape.residual = 1
    assert lib.acm_small_step_workspace_bytes_for(*handles, C.byref(shape), C.byref(with_res)) == 0 and with_res.value > nbytes.value
    assert np.isfinite(float(plan.run()))


def test_a_residual_step_on_the_smaller_workspace_is_refused():
    from acm_gnn_amd import _lib, train as T
    from acm_gnn_amd.small import SmallPlan
    adj, f_in, classes = GRAPHS["eight"]()
    case = _case(adj, f_in, classes, seed=11, s=0)
    model = _model(case, f_in, classes, (0, 0, False), 64, 0.0)
    y = torch.from_numpy(case["y"]).to(DEV)
    w = T.row_weights(torch.from_numpy(case["tr"]).to(DEV), case["n"])
    plan = SmallPlan(model, case["xs"], case["ops"], y, w, optimizer=None, update=False)
    nbytes = C.c_size_t()
    lib = _lib.load()
    assert lib.acm_small_step_workspace_bytes(plan.low.handle, case["xs"].csr.handle, case["xs"].csr_t.handle, C.byref(nbytes)) == 0
    assert plan.workspace.numel() * 4 > nbytes.value
    plan.p.workspace_bytes = nbytes.value
    with pytest.raises(RuntimeError, match="workspace"):
        plan.run()
    assert lib.acm_small_step(plan.low.handle, case["xs"].csr.handle, case["xs"].csr_t.handle, C.byref(plan.p), None) == 2     # ACM_ESHAPE


def test_refusals_keep_the_general_path_and_fit_batched_falls_back():
    from acm_gnn_amd import FusedAdam, functional as AF, train as T
    from acm_gnn_amd.small import SmallPlan
    adj, f_in, classes = GRAPHS["eight"]()
    case = _case(adj, f_in, classes, seed=11, s=0)
    y = torch.from_numpy(case["y"]).to(DEV)
    w = T.row_weights(torch.from_numpy(case["tr"]).to(DEV), case["n"])
    cell = (0, 0, False)

    def trains(model, opt, reason):
        assert SmallPlan.why_not(model, case["xs"], case["ops"], opt) == reason
        step = T.TrainStep(model, opt, case["xs"], case["ops"], y, w)
        assert step.small is None and step.small_refused == reason
        losses = [float(step()) for _ in range(3)]
        assert all(np.isfinite(losses)) and losses[-1] < losses[0]

    deep = _model(case, f_in, classes, cell, 64, 0.0, init_layers_X=2)
    trains(deep, FusedAdam(deep.parameters(), lr=0.01), "mlpX with 2 Linears (init_layers_X = 1 only)")
    nobias = _model(case, f_in, classes, cell, 64, 0.0)
    nobias.mlpX.lins[0] = torch.nn.Linear(f_in, 64, bias=False).to(DEV)
    trains(nobias, FusedAdam(nobias.parameters(), lr=0.01), "mlpX Linear without bias")
    part = _model(case, f_in, classes, cell, 64, 0.0)
    trains(part, FusedAdam(list(part.gcns.parameters()), lr=0.01), "a parameter of mlpX is not in the optimizer's group")

    n = case["n"]

    def make(k):
        m = _model(case, f_in, classes, cell, 64, 0.5, seed=20 + k)
        m.dropout_state = AF.DropoutState(torch.device(DEV), seed=100 + k)
        idx = torch.randperm(n, generator=torch.Generator().manual_seed(k)).to(DEV)
        return m, FusedAdam(m.parameters(), lr=0.01, weight_decay=1e-3), idx[: n // 2], idx[n // 2: 3 * n // 4], idx[3 * n // 4:]

    got = T.fit_batched([make(k) for k in range(3)], case["xs"], case["ops"], y, 6, rule="min_val_loss", batch=2, sync_every=4)
    why = T.fit_batched.last_refusal
    assert why is not None and "residual" in why, why
    want = T.fit_concurrent([make(k) for k in range(3)], case["xs"], case["ops"], y, 6, rule="min_val_loss", sync_every=4)
    assert len(got) == 3
    for k in range(3):
        assert got[k][0] == want[k][0] and got[k][1] == want[k][1], k
