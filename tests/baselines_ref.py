"""float64 restatement of the synthetic study's five models (mlp, gcn, sgc, acmgcn, acmsgc), written from their semantics --
not from the reference's text -- as the comparison arm wherever dropout masks are involved.  tests/test_baselines_cpu.py pins
it to the recorded fixture (tests/golden/baseline_cases.npz).

    mlp      relu -> dropout between two  X W_mlp  products
    gcn      A (dropout(relu(A (X W1))) W2)
    sgc      A^hops (X W)
    acm layer   L = act(A (X W_l)), H = act((I - A) (X W_h)), M = act(X W_m);   act = relu (acmgcn) or identity (acmsgc)
                alpha = softmax(sigmoid([L v_l, H v_h, M v_m]) att_vec / 3);      out = 3 (alpha_l L + alpha_h H + alpha_m M)
    acmgcn   layer(dropout(relu(layer(dropout(X)))))          acmsgc   layer(dropout(X))

``params``: name -> array with the reference's state_dict names (``gcns.<i>.<name>``).  ``masks``: multiplicative factors (0 or
1 / (1 - p)) per dropout site, ``{"x": [n, F_in], "hidden": [n, hidden]}``; a missing site is not dropped."""
import numpy as np
import torch

MODEL_TYPES = ("mlp", "gcn", "sgc", "acmgcn", "acmsgc")


def _t(a):
    return a.detach().double() if isinstance(a, torch.Tensor) else torch.from_numpy(np.asarray(a, np.float64))


def dense_operator(indptr, indices, vals):
    """CSR arrays -> the dense float64 matrix."""
    n = len(indptr) - 1
    a = np.zeros((n, n))
    rows = np.repeat(np.arange(n), np.diff(indptr))
    np.add.at(a, (rows, np.asarray(indices)), np.asarray(vals, np.float64))
    return torch.from_numpy(a)


def _acm_layer(p, i, x, a_low, relu):
    w = lambda name: p[f"gcns.{i}.{name}"]          # noqa: E731
    act = torch.relu if relu else (lambda t: t)
    high = torch.eye(a_low.shape[0], dtype=torch.float64) - a_low
    lo, hi, ml = act(a_low @ (x @ w("weight_low"))), act(high @ (x @ w("weight_high"))), act(x @ w("weight_mlp"))
    score = torch.sigmoid(torch.cat([lo @ w("att_vec_low"), hi @ w("att_vec_high"), ml @ w("att_vec_mlp")], 1))
    alpha = torch.softmax(score @ w("att_vec") / 3.0, 1)
    return 3.0 * (alpha[:, 0:1] * lo + alpha[:, 1:2] * hi + alpha[:, 2:3] * ml)


def forward(params, model_type, x, a_low, masks=None, hops=1):
    """Logits (float64 torch tensor; differentiable in the entries of ``params`` that are tensors requiring grad)."""
    p = {k: _t(v) if not (isinstance(v, torch.Tensor) and v.requires_grad) else v for k, v in params.items()}
    masks = masks or {}
    x, a_low = _t(x), _t(a_low)
    drop = lambda t, site: t * _t(masks[site]) if site in masks else t          # noqa: E731
    if model_type == "mlp":
        return drop(torch.relu(x @ p["gcns.0.weight_mlp"]), "hidden") @ p["gcns.1.weight_mlp"]
    if model_type == "gcn":
        h = drop(torch.relu(a_low @ (x @ p["gcns.0.weight_low"])), "hidden")
        return a_low @ (h @ p["gcns.1.weight_low"])
    if model_type == "sgc":
        z = x @ p["gcns.0.weight_low"]
        for _ in range(hops):
            z = a_low @ z
        return z
    if model_type == "acmgcn":
        h = drop(torch.relu(_acm_layer(p, 0, drop(x, "x"), a_low, True)), "hidden")
        return _acm_layer(p, 1, h, a_low, True)
    if model_type == "acmsgc":
        return _acm_layer(p, 0, drop(x, "x"), a_low, False)
    raise ValueError(model_type)


def nll(logits, labels, idx):
    logp = torch.log_softmax(logits, 1)
    lab = torch.as_tensor(np.asarray(labels), dtype=torch.int64)
    idx = torch.as_tensor(np.asarray(idx), dtype=torch.int64)
    return -logp[idx, lab[idx]].mean()


def trainable(params):
    """float64 leaf copies of the floating-point entries."""
    return {k: _t(v).clone().requires_grad_(True) for k, v in params.items()}


def loss_and_grads(params, model_type, x, a_low, labels, idx, masks=None, hops=1):
    """(loss, {name: gradient}) -- names whose gradient is None (parameters outside the forward) are left out."""
    p = trainable(params)
    loss = nll(forward(p, model_type, x, a_low, masks, hops), labels, idx)
    loss.backward()
    return float(loss.detach()), {k: v.grad for k, v in p.items() if v.grad is not None}


def trajectory(params, model_type, x, a_low, labels, idx, steps, lr=0.05, weight_decay=5e-4):
    """Training losses of ``steps`` Adam steps (torch.optim.Adam in float64, L2 weight decay; dropout 0)."""
    p = trainable(params)
    opt = torch.optim.Adam(list(p.values()), lr=lr, weight_decay=weight_decay)
    out = []
    for _ in range(steps):
        opt.zero_grad()
        loss = nll(forward(p, model_type, x, a_low), labels, idx)
        loss.backward()
        opt.step()
        out.append(float(loss.detach()))
    return out


def case_params(case, model_type):
    """The recorded initial state_dict of one model type: name -> array."""
    pre = f"{model_type}/init/"
    return {k[len(pre):]: case[k] for k in case if k.startswith(pre)}
