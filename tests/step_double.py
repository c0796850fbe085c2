"""Shared by the CPU tests that watch a training step or an evaluation pass on the test double: the ``tiny`` problem at the
headline configuration and a recorder of the ``acm_*`` entry points the double receives."""
import torch

_RIDERS = {"acm_conv_agg_fwd": ("out", "next_zlh", "agg_copy", "next_x"), "acm_conv_agg_bwd": ("out", "grad_out", "proj_dz", "next_agg")}
_NO_COMPUTE = ("acm_version", "acm_last_error", "acm_tuning_get", "acm_tuning_set")


class _Calls:
    """A recording wrapper around the double: the ``acm_*`` compute entry points it receives, in order (workspace and info
    queries left out) -- the two gradient-carrying calls of the hidden layer as (name, the optional riders that were non-NULL)
    -- and, apart, the ``proj_f`` of every acm_conv_agg_out_optional question."""

    def __init__(self, monkeypatch, fake):
        self.log, self.asked = [], []
        for name in dir(fake):
            fn = getattr(fake, name)
            if name.startswith("acm_") and callable(fn) and not name.endswith("_bytes") and not name.startswith("acm_csr_") \
                    and name not in _NO_COMPUTE:
                monkeypatch.setattr(fake, name, self._wrap(name, fn))

    def _wrap(self, name, fn):
        def call(*args):
            if name == "acm_conv_agg_out_optional":
                self.asked.append(int(args[2]))
            elif name in _RIDERS:
                self.log.append((name,) + tuple(r for r in _RIDERS[name] if getattr(args[1]._obj, r)))
            else:
                self.log.append(name)
            return fn(*args)
        return call

    def clear(self):
        del self.log[:], self.asked[:]

    def of(self, name):
        return [c for c in self.log if c[0] == name]


def _setup(seed=3, dropout=0.0, model_type="acmgcnp", pattern_only=False, **model_kw):
    from acm_gnn_amd import GCN, data as D
    from acm_gnn_amd.graph import CsrGraph, FilterOperators
    adj, _, y_np, _, _ = D.synthetic_dataset("tiny", seed=seed)
    low, deg = D.build_filters(adj)
    if pattern_only:                             # (the operators the input pipeline takes: the pattern and a row scale)
        from acm_gnn_amd.distributed import make_sharded_operators
        ops = make_sharded_operators(low, deg, torch.device("cpu"))
    else:
        ops = FilterOperators(CsrGraph.from_scipy(low, "cpu"))
    n = adj.shape[0]
    x = torch.randn(n, 7, generator=torch.Generator().manual_seed(seed))
    y = torch.from_numpy(y_np)
    w = torch.full((n,), 1.0 / n)
    torch.manual_seed(0)
    model = GCN(7, 64, int(y.max()) + 1, 2, n, dropout, model_type, 0, **model_kw)
    return model, ops, x, y, w


def _headline_step(model_type="acmgcnp", **step_kw):
    """The headline configuration on ``tiny``: counter-based dropout, the input pipeline on (P = A_low X is given, so the
    row-local stage is a launch of its own), an eager step on the Tape."""
    from acm_gnn_amd import FusedAdamW, functional as AF, train as T
    model, ops, x, y, w = _setup(dropout=0.3, model_type=model_type, pattern_only=True, attn_layernorm=True)
    model.dropout_state = AF.DropoutState("cpu", seed=3)
    step = T.TrainStep(model, FusedAdamW(model.parameters(), lr=0.01), x, ops, y, w, small_step=False, tape=True, **step_kw)
    return step, model, ops, x, y


class _Wrapper(torch.nn.Module):
    """A thin wrapper whose ``forward`` lacks the ``call`` keyword of models.GCN (the drop-in route's model is one): a step or
    pass over it reaches the layers through the calling thread's ambient context.  It hands on the one thing TrainStep's
    snapshot asks a model for, the dropout counter."""

    def __init__(self, gcn):
        super().__init__()
        self.gcn = gcn

    @property
    def dropout_state(self):
        return self.gcn.dropout_state

    def forward(self, x, adj, adj_high=None, adj_un=None):
        return self.gcn(x, adj, adj_high, adj_un)


def _eval_step(model, ops, x, y):
    from acm_gnn_amd import train as T
    return T.EvalStep(model, x, ops, y, [torch.arange(0, x.shape[0], 2)], loss_set=0, small_step=False)
