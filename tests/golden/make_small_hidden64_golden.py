#!/usr/bin/env python
"""The bits of the 64-wide fused small-graph step as the commit BEFORE the step became a template over the hidden width
computed them, written to tests/golden/small_hidden64_bits.npz (needs the MI355X):

    python tests/golden/make_small_hidden64_golden.py

The case (helpers of tests/test_gpu_small.py): the 300-node random graph of GRAPHS["eight"] (64 input features, 8 classes),
ACMII with the structure channel and LayerNorm (CONFIGS[3]), hidden width 64, dropout 0.5, FusedAdamW.

    single/losses             20 losses of 20 updating eager steps (TrainStep on the small path), float32 bits as uint32
    single/param/<name>       every parameter of both layers after the 20 steps, as uint32
    single/sq/<name>          its exp_avg_sq, as uint32
                              (a tensor of more than 1024 elements: the 32 bytes of the SHA-256 of those uint32s, as uint8 --
                              equal digests are equal bits, and the file stays a few tens of KB)
    batched/history/<k>       fit_batched, two runs (seeds 0 and 1) in two slots, 20 epochs: the history rows as float64 bits
    batched/param/<k>/<name>  the parameters of run k of at most 4096 elements, as uint32 or as that digest

tests/test_gpu_small_hidden.py runs `single` and `batched` below again and compares bit for bit.
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]     # the package, and tests/ for the helpers
STEPS = 20
PATH = os.path.join(HERE, "small_hidden64_bits.npz")

BIG = 1024


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32).numpy().view(np.uint32).copy()


def _pack(bits):
    """The uint32 view itself, or its digest for a large tensor."""
    if bits.size <= BIG:
        return bits
    return np.frombuffer(hashlib.sha256(np.ascontiguousarray(bits).tobytes()).digest(), np.uint8).copy()


def _setup():
    import test_gpu_small as S
    adj, f_in, classes = S.GRAPHS["eight"]()
    cfg = S.CONFIGS[3]
    case = S._case(adj, f_in, classes, seed=11, s=cfg["s"])
    return S, case, f_in, classes, cfg


def _make(S, case, f_in, classes, cfg, k):
    from acm_gnn_amd import FusedAdamW, functional as AF
    model = S._model(case, f_in, classes, cfg, 0.5, seed=k)
    model.dropout_state = AF.DropoutState(torch.device(S.DEV), seed=300 + k)
    return model, FusedAdamW(model.parameters(), lr=0.01, weight_decay=5e-3)


def single(tweak=None):
    """``tweak(plan)``: called on the step's SmallPlan before the first step."""
    from acm_gnn_amd import train as T
    S, case, f_in, classes, cfg = _setup()
    model, opt = _make(S, case, f_in, classes, cfg, 0)
    y = torch.from_numpy(case["y"]).to(S.DEV)
    w = T.row_weights(torch.from_numpy(case["tr"]).to(S.DEV), case["n"])
    step = T.TrainStep(model, opt, case["xs"], case["ops"], y, w, use_graph=False)
    assert step.small is not None, step.small_refused
    if tweak is not None:
        tweak(step.small)
    out = {"single/losses": _bits(torch.stack([step().detach().clone() for _ in range(STEPS)]))}
    for name, p in model.named_parameters():
        if name.startswith("gcns.") and p in opt.state:
            out[f"single/param/{name}"] = _pack(_bits(p))
            out[f"single/sq/{name}"] = _pack(_bits(opt.state[p]["exp_avg_sq"]))
    return out


def batched():
    from acm_gnn_amd import train as T
    S, case, f_in, classes, cfg = _setup()
    n = case["n"]
    y = torch.from_numpy(case["y"]).to(S.DEV)
    runs = []
    for k in range(2):
        perm = np.random.default_rng(40 + k).permutation(n)
        sets = [torch.from_numpy(np.sort(perm[a:b])).to(S.DEV) for a, b in ((0, 120), (120, 210), (210, 300))]
        runs.append((*_make(S, case, f_in, classes, cfg, k), *sets))
    got = T.fit_batched(runs, case["xs"], case["ops"], y, STEPS, batch=2, sync_every=5)
    assert T.fit_batched.last_refusal is None, T.fit_batched.last_refusal
    out = {}
    for k, (_, hist) in enumerate(got):
        assert len(hist) == STEPS
        out[f"batched/history/{k}"] = np.asarray(hist, np.float64).view(np.uint64)
        for name, p in runs[k][0].named_parameters():
            if name.startswith("gcns.") and p.numel() <= 4096:
                out[f"batched/param/{k}/{name}"] = _pack(_bits(p))
    return out


if __name__ == "__main__":
    rec = {**single(), **batched()}
    again = {**single(), **batched()}
    assert all(np.array_equal(rec[k], again[k]) for k in rec), "the case is not reproducible"
    path = sys.argv[1] if len(sys.argv) > 1 else PATH
    np.savez_compressed(path, **rec)
    print(path, os.path.getsize(path), "bytes,", len(rec), "arrays")
