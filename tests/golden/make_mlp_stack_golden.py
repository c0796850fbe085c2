"""Record the reference's deep MLP (Linear -> ReLU -> BatchNorm1d -> dropout(p = 0) -> ... -> Linear) -> tests/golden/mlp_stack_cases.npz.

    python tests/golden/make_mlp_stack_golden.py /path/to/ACM-GNN

Imports ``MLP`` from ``ACM-Pytorch/models/layers.py`` of the reference checkout and runs it in float64 on the CPU.  Per case
(n <= 257 rows, widths <= 24, 2 and 3 Linears; one case with a hidden unit that never fires): the input, every parameter, a
fixed upstream gradient, ``relu(mlp(x))`` in training mode and all gradients of ``sum(dy * relu(mlp(x)))``, the running
statistics and ``num_batches_tracked`` after one and after three training forwards, and the evaluation-mode output after
those three.  tests/mlp_stack_ref.py (the numpy restatement the other tests measure against) is pinned to these numbers."""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
# name: (rows, in, hidden, out, Linears, index of a hidden unit of the first layer that never fires or -1)
CASES = {"wide2": (257, 7, 24, 24, 2, -1), "deep3": (64, 13, 16, 9, 3, 5), "tiny2": (5, 3, 4, 2, 2, -1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("reference", help="checkout of the reference repository")
    ap.add_argument("--out", default=os.path.join(HERE, "mlp_stack_cases.npz"))
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(os.path.abspath(args.reference), "ACM-Pytorch", "models"))
    from layers import MLP
    rec = {"cases": np.array(sorted(CASES))}
    for k, (name, (n, f_in, hid, f_out, n_lins, dead)) in enumerate(sorted(CASES.items())):
        torch.manual_seed(100 + k)
        mlp = MLP(f_in, hid, f_out, n_lins, dropout=0.0).double().cpu()
        with torch.no_grad():
            for bn in mlp.bns:                               # (the defaults, weight 1 and bias 0, would hide both from the gradients)
                bn.weight.uniform_(0.5, 1.5)
                bn.bias.uniform_(-0.5, 0.5)
            if dead >= 0:
                mlp.lins[0].weight[dead].zero_()
                mlp.lins[0].bias[dead] = -1.0
        x = torch.randn(n, f_in, dtype=torch.float64) * 1.5 + 0.25
        dy = torch.randn(n, f_out, dtype=torch.float64)
        mlp.train()
        y = torch.relu(mlp(x, input_tensor=True))
        (y * dy).sum().backward()
        rec[f"{name}:shape"] = np.array([n, f_in, hid, f_out, n_lins, dead], np.int64)
        rec[f"{name}:x"], rec[f"{name}:dy"], rec[f"{name}:y"] = x.numpy(), dy.numpy(), y.detach().numpy()
        for i, lin in enumerate(mlp.lins):
            rec[f"{name}:W{i}"], rec[f"{name}:b{i}"] = lin.weight.detach().numpy().copy(), lin.bias.detach().numpy().copy()
            rec[f"{name}:dW{i}"], rec[f"{name}:db{i}"] = lin.weight.grad.numpy().copy(), lin.bias.grad.numpy().copy()
        bns = list(mlp.bns)[:n_lins - 1]
        for i, bn in enumerate(bns):
            rec[f"{name}:gamma{i}"], rec[f"{name}:beta{i}"] = bn.weight.detach().numpy().copy(), bn.bias.detach().numpy().copy()
            rec[f"{name}:dgamma{i}"], rec[f"{name}:dbeta{i}"] = bn.weight.grad.numpy().copy(), bn.bias.grad.numpy().copy()
            rec[f"{name}:rm1_{i}"], rec[f"{name}:rv1_{i}"] = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()
            rec[f"{name}:nbt1_{i}"] = np.int64(bn.num_batches_tracked.item())
        with torch.no_grad():
            mlp(x, input_tensor=True)
            mlp(x, input_tensor=True)
        for i, bn in enumerate(bns):
            rec[f"{name}:rm3_{i}"], rec[f"{name}:rv3_{i}"] = bn.running_mean.numpy().copy(), bn.running_var.numpy().copy()
            rec[f"{name}:nbt3_{i}"] = np.int64(bn.num_batches_tracked.item())
        mlp.eval()
        with torch.no_grad():
            rec[f"{name}:y_eval"] = torch.relu(mlp(x, input_tensor=True)).numpy()
        print(name, tuple(y.shape), "dead unit" if dead >= 0 else "")
    np.savez_compressed(args.out, **rec)
    print("wrote", args.out, os.path.getsize(args.out), "bytes")


if __name__ == "__main__":
    main()
