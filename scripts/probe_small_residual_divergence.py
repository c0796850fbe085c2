#!/usr/bin/env python3
"""Run ON THE GPU BOX: where do the small-graph step and the general path of ACM-GCN++ part over twelve training steps?  Both are
stepped side by side from one state on the one-step edge case of tests/test_gpu_small_residual.py (one node carries every
feature); after every step the two losses and, per parameter, the largest difference with that element's Adam moments on both
paths are printed.  profiles/small_residual_divergence.txt is its output; EXPERIMENTS.md ("ACM-GCN++ on the small-graph
step", Numerics) reads it: under Adam the paths agree to seven digits for five steps and part at the sixth in W1 (whole
columns at once: one ReLU of the dominant node), mlpX's tensors two steps later; under AdamW they agree throughout.

    python scripts/probe_small_residual_divergence.py > profiles/small_residual_divergence.txt"""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
import test_gpu_small_residual as R
from acm_gnn_amd import FusedAdam, FusedAdamW, functional as AF, train as T
DEV = "cuda:0"
for decoupled in (False, True):
    cell, f_in, classes, p_drop = ((0, 1, True) if decoupled else (1, 0, False)), 300, 3, 0.5
    case = R._edge_case(f_in, classes, cell[1])
    y = torch.from_numpy(case["y"]).to(DEV)
    w = T.row_weights(torch.from_numpy(case["tr"]).to(DEV), case["n"])
    def mk(small):
        model = R._model(case, f_in, classes, cell, 64, p_drop, seed=3)
        model.dropout_state = AF.DropoutState(torch.device(DEV), seed=77)
        opt = (FusedAdamW if decoupled else FusedAdam)(model.parameters(), lr=0.02, weight_decay=5e-3)
        step = T.TrainStep(model, opt, case["xs"], case["ops"], y, w, small_step=None if small else False)
        assert (step.small is not None) == small
        return model, opt, step
    ma, oa, sa = mk(True); mb, ob, sb = mk(False)
    for it in range(12):
        la, lb = float(sa()), float(sb())
        rows = []
        for (k, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
            d = (pa - pb).abs()
            if float(d.max()) > 0:
                i = int(d.argmax())
                sta, stb = oa.state.get(pa, {}), ob.state.get(pb, {})
                extra = ""
                if sta:
                    extra = " m %.3e/%.3e v %.3e/%.3e" % (float(sta["exp_avg"].flatten()[i]), float(stb["exp_avg"].flatten()[i]),
                                                        float(sta["exp_avg_sq"].flatten()[i]), float(stb["exp_avg_sq"].flatten()[i]))
                rows.append((float(d.max()), k, i, int((d > 1e-4).sum()), extra))
        rows.sort(reverse=True)
        print("decoupled", decoupled, "step", it, "loss %.7f %.7f" % (la, lb), flush=True)
        for r in rows[:5]:
            print("    %.3e %s idx %d n>1e-4 %d%s" % r)
