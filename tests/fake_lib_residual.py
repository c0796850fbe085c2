"""The test double's acm_small_step with the ACM-GCN++ residual branch: it reads ``residual``, the two tensors of ``res`` and
``drop_res`` from the struct (and the hidden width, as tests/fake_lib_hidden.py does) and runs the step through the oracle --
layer 2 sees drop(relu(fea1)) + drop_res(relu(x_d W_X^T + b_X)).  With it come the two entry points the host asks before it
offers such a plan: ``acm_small_step_has_residual`` and ``acm_small_step_workspace_bytes_for``.  A block without the residual
goes to fake_lib_hidden's step unchanged.  TEST DOUBLE, CPU suite only."""
import numpy as np

import fake_lib
import fake_lib_hidden
from fake_lib import _vec, _view, dropout_factors

WIDTHS = fake_lib_hidden.WIDTHS


def _adam(p, v, t, gr):
    """acm_adam_step's arithmetic on one tensor's views (fake_lib_hidden.acm_small_step's, stated once)."""
    f32 = np.float32
    m, vv, step = _vec(t.exp_avg, len(v)), _vec(t.exp_avg_sq, len(v)), _vec(t.step, 1)
    kk = float(step[0]) + 1.0
    step_size = f32(p.lr / (1.0 - p.beta1 ** kk))
    bc2_sqrt = f32((1.0 - p.beta2 ** kk) ** 0.5)
    gg = gr.copy()
    if p.weight_decay != 0:
        if p.decoupled:
            v *= f32(1.0 - p.lr * p.weight_decay)
        else:
            gg = gg + f32(p.weight_decay) * v
    m += f32(1.0 - p.beta1) * (gg - m)
    vv[...] = vv * f32(p.beta2) + f32(1.0 - p.beta2) * gg * gg
    v -= step_size * (m / (np.sqrt(vv) / bc2_sqrt + f32(p.eps)))


def acm_small_step(self, a, x, xt, pp, stream):
    import scipy.sparse as sp
    import torch
    from acm_gnn_amd import _lib
    from oracle import acm_oracle as O
    p = pp._obj
    if int(p.residual) == 0:
        return fake_lib_hidden.acm_small_step(self, a, x, xt, pp, stream)
    if int(p.residual) != 1:
        self._err = b"acm_small_step: residual must be 0 or 1 (got %d)" % int(p.residual)
        return 1
    if not (p.res[0].param and p.res[1].param):
        self._err = b"acm_small_step: residual without its parameters"
        return 1
    g = self._get(a)
    n, C_, k = g.n_rows, int(p.n_classes), int(p.n_channels)
    hidden = int(p.hidden) or 64
    if hidden not in WIDTHS:
        self._err = b"acm_small_step: hidden width %d (32 | 64)" % hidden
        return 4
    self.small_calls = getattr(self, "small_calls", 0) + 1
    self.small_residual_calls = getattr(self, "small_residual_calls", 0) + 1
    self.small_drop_res = (float(p.drop_res.p), int(p.drop_res.tag), int(p.drop_res.row_offset))
    pat = sp.csr_matrix((np.ones(len(g.indices)), g.indices, g.indptr), shape=(n, n))
    rs = _vec(p.row_scale, n).astype(np.float64)
    low = torch.from_numpy((sp.diags(rs) @ pat).toarray())
    high = torch.eye(n, dtype=torch.float64) - low
    raw = torch.from_numpy((pat - sp.identity(n)).toarray())
    fx = self._get(x)
    f_in = int(p.f_in)
    vals = _vec(p.x_vals, len(fx.indices)).astype(np.float64)
    train = bool(p.train)
    if train:
        vals = vals * dropout_factors(p.drop_in, len(vals), 1)[:, 0]
    xd = torch.from_numpy(sp.csr_matrix((vals, fx.indices, fx.indptr), shape=(n, f_in)).toarray())
    names = {_lib.SR_W_LOW: "weight_low", _lib.SR_W_HIGH: "weight_high", _lib.SR_W_MLP: "weight_mlp", _lib.SR_V_LOW: "att_vec_low",
             _lib.SR_V_HIGH: "att_vec_high", _lib.SR_V_MLP: "att_vec_mlp", _lib.SR_V_STRUC: "att_struc_low",
             _lib.SR_LNW_LOW: "layer_norm_low.weight", _lib.SR_LNW_HIGH: "layer_norm_high.weight", _lib.SR_LNW_MLP: "layer_norm_mlp.weight",
             _lib.SR_LNW_STRUC: "layer_norm_struc_low.weight", _lib.SR_LNB_LOW: "layer_norm_low.bias",
             _lib.SR_LNB_HIGH: "layer_norm_high.bias", _lib.SR_LNB_MLP: "layer_norm_mlp.bias", _lib.SR_LNB_STRUC: "layer_norm_struc_low.bias",
             _lib.SR_MIX: "att_vec", _lib.SR_STRUC: "struc_low"}
    dims = [(f_in, hidden), (hidden, C_)]

    def shape(li, role):
        fi, fo = dims[li]
        if role <= _lib.SR_W_MLP:
            return (fi, fo)
        if role == _lib.SR_MIX:
            return (k, k)
        if role == _lib.SR_STRUC:
            return (n, fo)
        return (fo, 1) if role <= _lib.SR_V_STRUC else (fo,)

    # (view, struct entry, float64 leaf) of every tensor: the roles of the two layers, then the Linear's weight [F, f_in] and bias
    tensors, leaves = [], [{}, {}]
    for li in range(2):
        for role, nm in names.items():
            t = p.t[li][role]
            if not t.param:
                continue
            sh = shape(li, role)
            v = _vec(t.param, int(np.prod(sh)))
            leaf = torch.from_numpy(v.astype(np.float64).reshape(sh)).requires_grad_(train)
            leaves[li][nm] = leaf
            tensors.append((v, t, leaf))
    res = []
    for r, sh in enumerate(((hidden, f_in), (hidden,))):
        t = p.res[r]
        v = _vec(t.param, int(np.prod(sh)))
        leaf = torch.from_numpy(v.astype(np.float64).reshape(sh)).requires_grad_(train)
        res.append(leaf)
        tensors.append((v, t, leaf))
    kw = dict(model_type="acmgcnp", variant=bool(p.relu_before), structure_info=int(k == 4), attn_layernorm=bool(p.layernorm))
    un = raw if k == 4 else None
    fea, att1 = O.layer_forward(leaves[0], xd, low, high, un, return_att=True, **kw)
    fea = torch.relu(fea)
    xx = torch.relu(xd @ res[0].t() + res[1])
    if train:
        fea = fea * torch.from_numpy(dropout_factors(p.drop_hidden, n, hidden))
        xx = xx * torch.from_numpy(dropout_factors(p.drop_res, n, hidden))
    out, att2 = O.layer_forward(leaves[1], fea + xx, low, high, un, return_att=True, **kw)
    _view(p.logits, n, C_, C_)[...] = out.detach().numpy()
    _view(p.att1, n, 4, 4)[:, :k] = att1.detach().numpy()
    _view(p.att2, n, 4, 4)[:, :k] = att2.detach().numpy()
    if not train:
        return 0
    y = torch.from_numpy(_vec(p.labels, n, np.int64).copy())
    w = torch.from_numpy(_vec(p.row_weight, n).astype(np.float64))
    loss = -(w * torch.log_softmax(out, 1).gather(1, y.view(-1, 1)).view(-1)).sum()
    loss.backward()
    _vec(p.loss, 1)[0] = float(loss.detach())
    stepped = set()
    for v, t, leaf in tensors:
        gr = (torch.zeros_like(leaf) if leaf.grad is None else leaf.grad).numpy().reshape(-1).astype(np.float32)
        if t.grad:
            _vec(t.grad, len(v))[...] = gr
        if not p.update:
            continue
        _adam(p, v, t, gr)
        stepped.add(int(t.step))
    if p.update:
        for addr in stepped:
            _vec(addr, 1)[0] += 1.0
        if p.also_advance:
            _vec(p.also_advance, 1, np.int64)[0] += 1
    return 0


def acm_small_step_workspace_bytes_for(self, a, x, xt, shape, bytes_out):
    """The stock double's size, and a recognisable surplus with the residual (the host must size a residual plan with THIS entry)."""
    st = self.acm_small_step_workspace_bytes(a, x, xt, bytes_out)
    if st == 0 and int(shape._obj.residual):
        bytes_out._obj.value += RESIDUAL_EXTRA_BYTES
    return st


RESIDUAL_EXTRA_BYTES = 4096


def install(monkeypatch):
    """fake_lib.install with the residual-reading small step, the capability probes and the shape-taking workspace entry."""
    monkeypatch.setattr(fake_lib.FakeLib, "acm_small_step", acm_small_step)
    monkeypatch.setattr(fake_lib.FakeLib, "acm_small_step_workspace_bytes_for", acm_small_step_workspace_bytes_for, raising=False)
    fake = fake_lib.install(monkeypatch)
    fake.acm_small_step_has_hidden = lambda w: int(w in (0,) + WIDTHS)
    fake.acm_small_step_has_residual = lambda: 1
    return fake
