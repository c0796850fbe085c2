"""The headline training path against a recorded run of the imported reference (ACM-Geometric dialect).

What bench.py times -- the two-layer acmgcnp with the attention LayerNorm live, AdamW, counter-based dropout drawn inside the
kernels, the first layer on the 16-row aggregate-first kernels with the input pipeline (functional.InputPipeline: the backward
carries next step's P = A_low dropout(x)), FusedAdamW flushing the deferred reductions in its own launch, the whole step one
captured graph, on operators relabelled by degree -- trained for 120 epochs on three fixed splits of a 32 768-node heavy-tailed
graph (tests/golden/graph_twitch_syn.npz), exactly as tests/golden/make_accuracy_golden.py (``twitch_syn --dialect geometric``)
trained the reference: same seeded CPU initialisation, the library's own masks injected into the reference by the row the
degree relabelling gives each node (tests/replay.py: PhiloxDropout(dense=True, rows=...)), same optimizer, same selection rule
(ACM-Geometric/train.py:66-81, :111-139; logger.py:17-35).  TrainStep is handed the reference's adjacency TENSORS in the
reference's node order, so operators_for -> relabel_by_degree -> the row translation at the boundary are inside the test.
variant 0 is the headline cell; variant 1 (ACMII, the reference script's default) trains the mask-form ACMII kernels.

Bounds (BASELINE.md section 4c has the measured figures they come from):
  * early trajectory -- training loss and validation NLL over the first 5 / first 10 epochs: the constants of
    test_gpu_accuracy._judge_replay for lr >= 0.05 (rtol 2e-4 / 1e-3), kept where the reference's own second run (run "b": CSR
    operands, 3 threads -- another fp32 summation order) stays inside half of them against run "a", otherwise 4 x the largest
    a-to-b relative gap over those epochs (_early_rtol computes this from the two recordings);
  * whole run -- the three-strength +-0.2 pp criterion of BASELINE.md section 4a (_judge_replay, selection = first maximum of
    the validation accuracy); the per-split bound on the self-selected accuracy is max(0.4 pp, 4 x the largest per-split
    a-to-b difference).
"""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, load_npz
from oracle import acm_oracle as O
from replay import degree_order, load_twitch_syn
from test_gpu_accuracy import _judge_replay

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_DATA = {}
_RUNS = {}                # (variant, split) -> the captured single-step replay (shared by the tests below)


def _data():
    """The fixture graph and the reference's filters, built on the host with scipy as ACM-Geometric/train.py:69-81 does
    (oracle.filters_linkx / row_normalize_sp: float64 normalisation of I + A, cast to float32 COO; features row-normalised)."""
    if not _DATA:
        n, a, x_raw, labels, masks = load_twitch_syn(os.path.join(GOLDEN, "graph_twitch_syn.npz"))     # missing: an error
        low, high, _ = O.filters_linkx(a)
        x = torch.tensor(np.asarray(O.row_normalize_sp(x_raw).todense()))
        assert x.dtype == torch.float32 and x.shape == (n, 7)
        perm, inv = degree_order(np.diff(a.indptr))
        _DATA.update(n=n, a=a, x=x, labels=torch.from_numpy(labels), masks=masks, low=low, high=high, perm=perm, inv=inv)
    return _DATA


def _records(variant):
    name = f"twitch_syn_v{variant}"
    return (name, load_npz(os.path.join(GOLDEN, f"accuracy_{name}_philox.npz")),
            load_npz(os.path.join(GOLDEN, f"accuracy_{name}_b_philox.npz")))


def _rel_gap(got, ref):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    return float(np.max(np.abs(got - ref) / np.abs(ref)))


def _early_rtol(rec, rec_b):
    """(rtol over the first 5 epochs, over the first 10; the measured a-to-b gaps): see the module docstring."""
    out, gaps = [], []
    for k, const in ((5, 2e-4), (10, 1e-3)):
        gap = max(_rel_gap(rec_b[f"hist_{s}"][:k, c], rec[f"hist_{s}"][:k, c]) for s in rec["cfg"]["splits"] for c in (0, 1))
        gaps.append(gap)
        out.append(const if 2.0 * gap <= const else 4.0 * gap)
    return tuple(out), tuple(gaps)


def _probe_kernels(variant, d, low_d, high_d, xd, yd, w):
    """Launch labels of ONE eager step of a throw-away model of the same configuration (functional.KernelTimer)."""
    from acm_gnn_amd import GCN, FusedAdamW, functional as AF, train as T
    torch.manual_seed(5)
    model = GCN(7, 64, 2, 2, d["n"], 0.1, "acmgcnp", 0, variant=bool(variant), attn_layernorm=True).to(DEV)
    model.fused_dropout = True
    model.dropout_state = AF.DropoutState(torch.device(DEV), seed=5)
    step = T.TrainStep(model, FusedAdamW(model.parameters(), lr=0.05, weight_decay=1e-3), xd, low_d, yd, w, high_d, None,
                       use_graph=False)
    timer = AF.KernelTimer()
    AF.set_kernel_timer(timer)
    try:
        step()
        torch.cuda.synchronize()
    finally:
        AF.set_kernel_timer(None)
    return sorted(set(k.split("/")[0] for k in timer.events))


def _replay(variant, split, use_graph=True, steps_per_graph=1, pipeline_input=None, epochs=None):
    """One split of the recorded experiment on the path under test; returns the curves (training loss, validation NLL, train /
    validation / test accuracy -- the accuracies after every CALL of the step, i.e. every ``steps_per_graph`` epochs)."""
    from acm_gnn_amd import GCN, FusedAdamW, functional as AF, layers, train as T
    from acm_gnn_amd.graph import clear_cache
    name, rec, _ = _records(variant)
    cfg = rec["cfg"]
    d = _data()
    n = d["n"]
    epochs = int(cfg["epochs"] if epochs is None else epochs)
    assert cfg["dialect"] == "geometric" and cfg["optimizer"] == "adamw" and cfg["attn_layernorm"] == 1
    assert epochs % steps_per_graph == 0
    clear_cache()
    xd, yd = d["x"].to(DEV), d["labels"].to(DEV)
    low_d, high_d = d["low"].to(DEV), d["high"].to(DEV)        # the reference's tensors, the reference's node order
    tr, va, te = (torch.from_numpy(np.nonzero(m)[0]).to(DEV) for m in d["masks"][split])
    default_device = layers._default_device
    layers._default_device = lambda: torch.device("cpu")      # seeded CPU initialisation, like the reference run
    try:
        torch.manual_seed(1000 + split)
        model = GCN(xd.shape[1], cfg["hidden"], int(d["labels"].max()) + 1, cfg["num_layers"], n, cfg["dropout"], cfg["model"],
                    cfg["structure_info"], variant=bool(cfg["variant"]), attn_layernorm=True).to(DEV)
    finally:
        layers._default_device = default_device
    model.fused_dropout = True
    model.dropout_state = st = AF.DropoutState(torch.device(DEV), seed=int(cfg["philox_seed"]) + split)
    opt = FusedAdamW(model.parameters(), lr=cfg["lr"], weight_decay=cfg["weight_decay"])
    w = T.row_weights(tr, n)
    step = T.TrainStep(model, opt, xd, low_d, yd, w, high_d, None, use_graph=use_graph, steps_per_graph=steps_per_graph,
                       pipeline_input=pipeline_input)
    # ---- the path under test is the one running
    ops = step.adj
    assert ops.perm is not None and not torch.equal(ops.perm.cpu(), torch.arange(n)), "the operators must be relabelled"
    assert np.array_equal(ops.perm.cpu().numpy(), d["perm"]) and np.array_equal(ops.inv_perm.cpu().numpy(), d["inv"])
    assert step._permuted and ops.low.n_long_rows > 0 and ops.low.max_degree > 2 * ops.low.chunk     # a hub in several pieces
    assert step.small is None, "a 32 768-node graph is not the fused small-graph step's"
    route = AF._conv_route(step.x, ops, model.gcns[0]._config(), xd.shape[1], cfg["hidden"])
    if cfg["variant"]:
        assert step.pipe is None and route == "acmii", route
    else:
        assert route == "agg", route
        assert (step.pipe is not None) == (pipeline_input is not False)
    ev = T.EvalStep(model, xd, low_d, yd, (tr, va, te), high_d, None, loss_set=1, use_graph=use_graph)
    assert ev.small is None
    losses, vals, acc_tr, acc_va, acc_te = [], [], [], [], []
    for _ in range(epochs // steps_per_graph):
        loss = step()
        losses.extend([float(v) for v in step.losses] if steps_per_graph > 1 else [float(loss)])
        _, (a_tr, a_va, a_te), val_nll = ev()
        vals.append(val_nll)
        acc_tr.append(a_tr)
        acc_va.append(a_va)
        acc_te.append(a_te)
    assert int(st.step.item()) == epochs
    if step.pipe is not None:
        assert step.pipe.primed
    k = int(np.argmax(acc_va))                                  # logger.py:20,33-34: the first maximum
    return dict(losses=losses, vals=vals, acc_tr=acc_tr, acc_va=acc_va, acc_te=acc_te, selected=acc_te[k], selected_epoch=k,
                tensors=(d, low_d, high_d, xd, yd, w))


def _headline_run(variant, split):
    if (variant, split) not in _RUNS:
        _RUNS[(variant, split)] = _replay(variant, split)
    return _RUNS[(variant, split)]


def test_host_degree_order_is_the_operators_permutation():
    """The masks were recorded by the row tests/replay.degree_order gives every node: it must be graph.relabel_by_degree's."""
    from acm_gnn_amd import graph
    d = _data()
    graph.clear_cache()
    low_d, high_d = d["low"].to(DEV), d["high"].to(DEV)
    ops = graph.operators_for(low_d, high_d)
    assert ops.perm is not None
    assert np.array_equal(ops.perm.cpu().numpy(), d["perm"]) and np.array_equal(ops.inv_perm.cpu().numpy(), d["inv"])
    assert 12 * d["n"] < ops.low.nnz <= 160 * d["n"]


@pytest.mark.parametrize("variant", [0, 1])
def test_headline_path_replays_the_reference_run(variant):
    """Every split of the recorded run on the captured headline step; the path conditions, the early trajectory and the
    whole-run criterion of the module docstring.  Every figure is printed before it is asserted."""
    name, rec, rec_b = _records(variant)
    cfg = rec["cfg"]
    assert cfg["epochs"] >= 100 and len(cfg["splits"]) >= 3 and rec_b["cfg"]["splits"] == cfg["splits"]
    runs = {s: _headline_run(variant, s) for s in cfg["splits"]}
    d, low_d, high_d, xd, yd, w = runs[cfg["splits"][0]]["tensors"]
    used = _probe_kernels(variant, d, low_d, high_d, xd, yd, w)
    print(f"\n{name}: launches of one eager step: {used}")
    if variant:
        assert "conv_acmii_v_fwd" in used and "conv_acmii_v_bwd" in used, used          # the ACMII mask route
    else:
        assert "conv_agg_epi" in used and any(k.startswith("conv_agg_bwd+gather") for k in used), used    # the input pipeline
    assert any(k.startswith("adam+flush") for k in used), used                         # the flush inside the optimizer launch
    # ---- early trajectory
    (tol5, tol10), (gap5, gap10) = _early_rtol(rec, rec_b)
    early = {}
    for s in cfg["splits"]:
        hist, run = rec[f"hist_{s}"], runs[s]
        early[s] = {"loss5": _rel_gap(run["losses"][:5], hist[:5, 0]), "val5": _rel_gap(run["vals"][:5], hist[:5, 1]),
                    "loss10": _rel_gap(run["losses"][:10], hist[:10, 0]), "val10": _rel_gap(run["vals"][:10], hist[:10, 1])}
    print(f"{name}: reference a-to-b relative gap, epochs 0-4: {gap5:.3g} (bound {tol5:.3g}), epochs 0-9: {gap10:.3g} "
          f"(bound {tol10:.3g}); this run, per split: {early}")
    first_bad = {s: next((e for e in range(cfg["epochs"])
                          if abs(runs[s]["losses"][e] - rec[f"hist_{s}"][e, 0]) > tol10 * abs(rec[f"hist_{s}"][e, 0])), None)
                 for s in cfg["splits"]}
    print(f"{name}: first epoch whose training loss is off by more than {tol10:.3g}, per split: {first_bad}")
    for s in cfg["splits"]:
        hist, run = rec[f"hist_{s}"], runs[s]
        np.testing.assert_allclose(run["losses"][:5], hist[:5, 0], rtol=tol5, err_msg=f"training loss, split {s}")
        np.testing.assert_allclose(run["vals"][:5], hist[:5, 1], rtol=tol5, err_msg=f"validation NLL, split {s}")
        np.testing.assert_allclose(run["losses"][:10], hist[:10, 0], rtol=tol10, err_msg=f"training loss, split {s}")
        np.testing.assert_allclose(run["vals"][:10], hist[:10, 1], rtol=tol10, err_msg=f"validation NLL, split {s}")
    # ---- whole run
    per_split_ab = np.abs(np.asarray(rec_b["test_acc"]) - np.asarray(rec["test_acc"]))
    split_bound = max(0.004, 4.0 * float(per_split_ab.max()))
    print(f"{name}: self-selected accuracy, reference a-to-b per split {np.round(100 * per_split_ab, 3).tolist()} pp -> per-split "
          f"bound {100 * split_bound:.2f} pp; selected epochs {[runs[s]['selected_epoch'] for s in cfg['splits']]}")
    results = {s: (runs[s]["selected"], runs[s]["vals"], runs[s]["acc_te"]) for s in cfg["splits"]}
    extra = {"train_loss": {str(s): runs[s]["losses"] for s in cfg["splits"]},
             "val_acc": {str(s): runs[s]["acc_va"] for s in cfg["splits"]},
             "early_rel_gap": {str(s): v for s, v in early.items()}, "early_rtol": [tol5, tol10],
             "reference_a_to_b_early_rel_gap": [gap5, gap10], "per_split_bound_pp": 100 * split_bound, "launches": used}
    _judge_replay(name, rec, results, f"accuracy_replay_{name}.json", path_label="headline path (captured, relabelled"
                  + (", ACMII mask form)" if variant else ", input pipeline)"), bounds=(0.002, split_bound),
                  selection="max_val_acc", early_rtol=(tol5, tol10), extra=extra)


def test_headline_run_in_its_other_forms():
    """Split 0 of variant 0 once more: the eager step and four steps per captured graph give the captured single-step run bit
    for bit; without the input pipeline the first ten epochs agree to the per-step tolerance of
    test_gpu_train.test_input_pipeline_matches_plain_step (rtol 2e-4, atol 1e-5 on the loss)."""
    name, rec, _ = _records(0)
    split = rec["cfg"]["splits"][0]
    base = _headline_run(0, split)
    eager = _replay(0, split, use_graph=False)
    for key in ("losses", "vals", "acc_tr", "acc_va", "acc_te"):
        assert eager[key] == base[key], (key, next(i for i, (p, q) in enumerate(zip(eager[key], base[key])) if p != q))
    four = _replay(0, split, steps_per_graph=4)
    assert four["losses"] == base["losses"]
    for key in ("vals", "acc_tr", "acc_va", "acc_te"):
        assert four[key] == base[key][3::4], key
    plain = _replay(0, split, pipeline_input=False, epochs=10)
    print(f"\n{name}: pipelined against plain step, first ten epochs: loss rel gap {_rel_gap(base['losses'][:10], plain['losses']):.3g}, "
          f"validation NLL rel gap {_rel_gap(base['vals'][:10], plain['vals']):.3g}")
    np.testing.assert_allclose(base["losses"][:10], plain["losses"], rtol=2e-4, atol=1e-5)
    np.testing.assert_allclose(base["vals"][:10], plain["vals"], rtol=2e-4, atol=1e-5)
