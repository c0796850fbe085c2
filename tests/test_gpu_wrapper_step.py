"""A model whose ``forward`` lacks the ``call`` keyword under a capture: train.TrainStep / train.EvalStep then reach the layers
through the calling thread's ambient contexts (deferred reductions, loss-tail request), and with ``use_graph`` those contexts are
entered while the stream captures.  Captured equals eager and the wrapper equals the bare GCN, bit for bit."""
import os
import sys

import numpy as np
import pytest
import scipy.sparse as sp
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from step_double import _Wrapper  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
N, F_IN = 40, 7                          # two full sixteen-row groups and a ragged one


@pytest.fixture(scope="module")
def problem():
    from acm_gnn_amd import data as D, train as T
    from acm_gnn_amd.distributed import make_sharded_operators
    rng = np.random.default_rng(5)
    r, c = rng.integers(0, N, 4 * N), rng.integers(0, N, 4 * N)
    adj = sp.csr_matrix((np.ones(4 * N, np.float32), (r, c)), shape=(N, N))
    adj = ((adj + adj.T) > 0).astype(np.float32).tocsr()
    adj.setdiag(0)
    adj.eliminate_zeros()
    low, deg = D.build_filters(adj)
    ops = make_sharded_operators(low, deg, torch.device(DEV))          # pattern-only: the pattern and a row scale
    g = torch.Generator().manual_seed(5)
    x = torch.randn(N, F_IN, generator=g).to(DEV)
    y = torch.randint(0, 2, (N,), generator=g).to(DEV)
    rows = torch.arange(N, device=DEV)
    w = T.row_weights(rows[rows % 10 != 0], N)       # four rows of weight 0: masked rows, below the loss-row attachment's share
    sets = [torch.arange(k, N, 3, device=DEV) for k in range(3)]
    return ops, x, y, w, sets


def _run(problem, wrap, use_graph):
    """Three training steps, then an evaluation pass, of one fresh instance: (losses, parameters, logits, numbers)."""
    from acm_gnn_amd import GCN, FusedAdamW, functional as AF, train as T
    ops, x, y, w, sets = problem
    torch.manual_seed(0)
    gcn = GCN(F_IN, 64, 2, 2, N, 0.3, "acmgcnp", 0, variant=False, attn_layernorm=True).to(DEV)
    gcn.fused_dropout, gcn.dropout_state = True, AF.DropoutState(torch.device(DEV), seed=31)       # counter-based masks
    opt = FusedAdamW(gcn.parameters(), lr=0.01, weight_decay=1e-3)
    opt.also_advance = gcn.dropout_state.step
    model = _Wrapper(gcn) if wrap else gcn
    step = T.TrainStep(model, opt, x, ops, y, w, use_graph=use_graph, small_step=False)
    assert (step.graph is not None) == use_graph and step.small is None and step.pipe is None
    losses = [float(step()) for _ in range(3)]
    assert step._defer is True and int(gcn.dropout_state.step) == 3           # (the capture's warm-up steps were put back)
    ev = T.EvalStep(model, x, ops, y, sets, use_graph=use_graph, small_step=False)
    assert (ev.graph is not None) == use_graph
    if not use_graph:
        ev()                # the first pass over a static input gathers P = A_low X itself and leaves it for the next ones, which
    logits, accs, val_loss = ev()          # take another kernel: a captured pass, behind its warm-up, is always one of those
    return losses, [p.detach().clone() for p in gcn.parameters()], logits.clone(), tuple(accs) + (val_loss,)


@pytest.fixture(scope="module")
def bare_eager(problem):
    return _run(problem, wrap=False, use_graph=False)


@pytest.mark.parametrize("wrap,use_graph", [(True, False), (True, True), (False, True)],
                         ids=["wrapper-eager", "wrapper-captured", "bare-captured"])
def test_step_and_pass_equal_the_bare_eager_ones(problem, bare_eager, wrap, use_graph):
    got = _run(problem, wrap, use_graph)
    assert np.isfinite(bare_eager[0]).all() and got[0] == bare_eager[0]
    assert len(got[1]) == len(bare_eager[1]) and all(torch.equal(a, b) for a, b in zip(got[1], bare_eager[1]))
    assert torch.equal(got[2], bare_eager[2]) and got[3] == bare_eager[3]
