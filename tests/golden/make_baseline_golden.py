#!/usr/bin/env python
"""Recorded outputs of the synthetic study's OWN model code (synthetic-experiments/baseline_models) for the five model types,
written to tests/golden/baseline_cases.npz.  The reference is imported at generation time only (it needs nothing but torch):

    python tests/golden/make_baseline_golden.py <path of the reference checkout>

One 96-node undirected graph WITHOUT self loops -- node 0 has degree 40, node 95 is isolated -- with the study's filters
(synthetic-experiments/train.py:72-78: adj_low = D^-1 (I + A), adj_high = I - adj_low, handed over as torch sparse tensors),
12 features, 5 classes, hidden width 32.  Per model type (mlp, gcn, sgc, acmgcn, acmsgc), from ``torch.manual_seed(SEED)``:

    <mt>/init/<name>   every entry of the fresh model's state_dict
    <mt>/logits        eval-mode output
    <mt>/loss          training-mode (dropout 0) NLL on the recorded index set, train.py:125-127
    <mt>/grad/<name>   the gradient of every parameter that has one after loss.backward()
    <mt>/traj          ten training losses under Adam(lr=0.05, weight_decay=5e-4), the study's defaults (dropout 0)
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
SEED, N, F_IN, CLASSES, HIDDEN, STEPS = 20240, 96, 12, 5, 32, 10
MODEL_TYPES = ("mlp", "gcn", "sgc", "acmgcn", "acmsgc")


def graph(rng):
    a = np.zeros((N, N), np.float32)
    a[0, 1:41] = 1                                        # the hub: degree 40
    for i in range(1, N - 1):                             # ~2 further neighbours per node among 1 .. 94; node 95 stays isolated
        for j in rng.choice(np.arange(1, N - 1), size=2, replace=False):
            if j != i:
                a[i, j] = 1
    a = np.maximum(a, a.T)
    np.fill_diagonal(a, 0)
    assert a[0].sum() == 40 and a[N - 1].sum() == 0 and (a == a.T).all()
    return a


def main(ref_root):
    sys.path.insert(0, os.path.join(ref_root, "synthetic-experiments"))
    from baseline_models.models import GCN                # noqa: E402  (the reference's)
    rng = np.random.RandomState(SEED)
    a = graph(rng)
    full = torch.from_numpy(a) + torch.eye(N)
    adj_low = (1.0 / full.sum(1))[:, None] * full         # normalize(): D^-1 (I + A), float32 as the study holds it
    adj_high = torch.eye(N) - adj_low
    x = torch.from_numpy(rng.standard_normal((N, F_IN)).astype(np.float32))
    labels = torch.from_numpy(rng.randint(0, CLASSES, N).astype(np.int64))
    train_idx = torch.from_numpy(np.sort(rng.choice(N, 40, replace=False)).astype(np.int64))
    low_sp, high_sp = adj_low.to_sparse(), adj_high.to_sparse()
    csr = adj_low.to_sparse_csr()
    out = {"indptr": csr.crow_indices().numpy().astype(np.int32), "indices": csr.col_indices().numpy().astype(np.int32),
           "vals": csr.values().numpy().astype(np.float32), "x": x.numpy(), "labels": labels.numpy(), "train_idx": train_idx.numpy(),
           "seed": np.int64(SEED), "hidden": np.int64(HIDDEN), "classes": np.int64(CLASSES)}

    def loss_of(model):
        model.train()
        logp = F.log_softmax(model(x, low_sp, high_sp), dim=1)
        return F.nll_loss(logp[train_idx], labels[train_idx])

    for mt in MODEL_TYPES:
        torch.manual_seed(SEED)
        model = GCN(nfeat=F_IN, nhid=HIDDEN, nclass=CLASSES, dropout=0.0, model_type=mt)
        for name, t in model.state_dict().items():
            # low_param / high_param / mlp_param are never initialised by the reference: recorded as zeros, never compared
            out[f"{mt}/init/{name}"] = np.zeros(tuple(t.shape), np.float32) if name.endswith("_param") and t.numel() == 1 else t.numpy().copy()
        model.eval()
        with torch.no_grad():
            out[f"{mt}/logits"] = model(x, low_sp, high_sp).numpy().copy()
        loss = loss_of(model)
        loss.backward()
        out[f"{mt}/loss"] = np.float32(loss.item())
        for name, p in model.named_parameters():
            if p.grad is not None:
                out[f"{mt}/grad/{name}"] = p.grad.numpy().copy()
        with torch.no_grad():
            for name, p in model.named_parameters():      # the uninitialised scalars would otherwise decay from garbage
                if name.endswith("_param") and p.numel() == 1:
                    p.zero_()
        opt = torch.optim.Adam(model.parameters(), lr=0.05, weight_decay=5e-4)
        traj = []
        for _ in range(STEPS):
            opt.zero_grad()
            loss = loss_of(model)
            loss.backward()
            opt.step()
            traj.append(loss.item())
        out[f"{mt}/traj"] = np.asarray(traj, np.float32)
    path = os.path.join(HERE, "baseline_cases.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
