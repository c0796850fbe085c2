"""The baselines of the synthetic study without a GPU: the new entry points exist and refuse bad arguments before any launch,
the ctypes mirrors of their parameter blocks have the C layout, the float64 restatement (tests/baselines_ref.py) reproduces the
values recorded from the study's own model code, and ``baselines.GCN`` draws the reference's initial values."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

import baselines_ref as R
from conftest import GOLDEN, ROOT, load_npz

NEW_SYMBOLS = ("acm_gcn_fwd", "acm_gcn_bwd_workspace_bytes", "acm_gcn_bwd", "acm_gemm_act")
EINVAL, ESHAPE, EUNSUPPORTED = 1, 2, 4


@pytest.fixture(scope="module")
def case():
    return load_npz(os.path.join(GOLDEN, "baseline_cases.npz"))


@pytest.fixture(scope="module")
def a_low(case):
    return R.dense_operator(case["indptr"], case["indices"], case["vals"])


def test_new_symbols_are_exported_and_the_abi_number_stays():
    from acm_gnn_amd import _lib, build
    lib = _lib.load()
    assert lib.acm_version() == 29 == _lib.ABI_VERSION
    for name in NEW_SYMBOLS:
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(lib, name), name
    assert "acm_gcn.hip" in build.SOURCES


def _fwd(**kw):
    from acm_gnn_amd import _lib
    p = _lib.GcnFwd()
    p.width, p.ld_z, p.ld_y = 32, 32, 32
    buf = (C.c_float * 64)()
    p.z = p.y = C.addressof(buf)
    for k, v in kw.items():
        setattr(p, k, v)
    p._keep = buf
    return p


def _bwd(**kw):
    from acm_gnn_amd import _lib
    p = _lib.GcnBwd()
    p.width, p.hidden, p.keep_scale, p.relu = 5, 32, 1.0, 1
    p.ld_dy, p.ld_h, p.ld_w2, p.ld_g, p.ld_dw2 = 5, 32, 5, 32, 5
    buf = (C.c_float * 64)()
    p.dy = p.h = p.w2 = p.g = p.d_w2 = C.addressof(buf)
    for k, v in kw.items():
        setattr(p, k, v)
    p._keep = buf
    return p


def test_entry_points_check_their_arguments_before_any_launch():
    from acm_gnn_amd import _lib
    lib = _lib.load()
    handle = C.c_void_p(C.addressof((C.c_char * 512)()))          # never dereferenced: every case below fails before
    err = lambda: lib.acm_last_error()                            # noqa: E731
    # NULL pointers
    assert lib.acm_gcn_fwd(None, None, None, 0, None) == EINVAL and b"acm_gcn_fwd" in err()
    assert lib.acm_gcn_fwd(None, C.byref(_fwd()), None, 0, None) == EINVAL and b"acm_gcn_fwd" in err()
    assert lib.acm_gcn_fwd(handle, C.byref(_fwd(y=None)), None, 0, None) == EINVAL
    assert lib.acm_gcn_fwd(handle, C.byref(_fwd(f_next=4, ld_w_next=4, ld_z_next=4)), None, 0, None) == EINVAL      # w_next / z_next
    assert lib.acm_gcn_bwd(None, None, None, 0, None) == EINVAL and b"acm_gcn_bwd" in err()
    assert lib.acm_gcn_bwd(None, C.byref(_bwd()), None, 0, None) == EINVAL and b"acm_gcn_bwd" in err()
    assert lib.acm_gcn_bwd(handle, C.byref(_bwd(h=None)), None, 0, None) == EINVAL
    nbytes = C.c_size_t()
    assert lib.acm_gcn_bwd_workspace_bytes(None, 5, 32, C.byref(nbytes)) == EINVAL
    assert lib.acm_gemm_act(4, 4, 4, None, 4, None, 4, 1, None, None, 4, None, 0, None) == EINVAL and b"acm_gemm_act" in err()
    # shapes
    assert lib.acm_gcn_fwd(handle, C.byref(_fwd(f_next=9)), None, 0, None) == EUNSUPPORTED and b"acm_gcn_fwd" in err()
    assert lib.acm_gcn_fwd(handle, C.byref(_fwd(width=300, ld_z=300, ld_y=300, f_next=2, ld_w_next=2, ld_z_next=2)), None, 0, None) == EUNSUPPORTED
    # a post-op on a narrow layer is refused (the narrow gather carries no post-op parameters); hidden bounds the slabs
    assert lib.acm_gcn_fwd(handle, C.byref(_fwd(width=8, ld_z=8, ld_y=8, relu=1)), None, 0, None) == EUNSUPPORTED and b"acm_gcn_fwd" in err()
    assert lib.acm_gcn_fwd(handle, C.byref(_fwd(width=5, ld_z=5, ld_y=5, f_next=2, ld_w_next=2, ld_z_next=2, w_next=1, z_next=1)), None, 0,
                           None) == EUNSUPPORTED
    assert lib.acm_gcn_bwd(handle, C.byref(_bwd(hidden=257, ld_h=257, ld_g=257)), None, 0, None) == EUNSUPPORTED and b"hidden" in err()
    assert lib.acm_gemm_act(4, 4, 4, handle, 3, handle, 4, 1, None, handle, 4, None, 0, None) == ESHAPE and b"acm_gemm_act" in err()
    assert lib.acm_gemm_act(4, 0, 4, handle, 4, handle, 4, 1, None, handle, 4, None, 0, None) == ESHAPE and b"acm_gemm_act" in err()
    assert lib.acm_gcn_fwd(handle, C.byref(_fwd(ld_y=31)), None, 0, None) == ESHAPE and b"acm_gcn_fwd" in err()
    assert lib.acm_gcn_fwd(handle, C.byref(_fwd(ld_z=31)), None, 0, None) == ESHAPE
    assert lib.acm_gcn_fwd(handle, C.byref(_fwd(width=0)), None, 0, None) == ESHAPE
    assert lib.acm_gcn_fwd(handle, C.byref(_fwd(f_next=4, ld_w_next=3, ld_z_next=4)), None, 0, None) == ESHAPE
    assert lib.acm_gcn_bwd(handle, C.byref(_bwd(width=9, ld_dy=9, ld_w2=9, ld_dw2=9)), None, 0, None) == EUNSUPPORTED and b"acm_gcn_bwd" in err()
    assert lib.acm_gcn_bwd_workspace_bytes(handle, 9, 32, C.byref(nbytes)) == EUNSUPPORTED and b"acm_gcn_bwd" in err()
    for field in ("ld_dy", "ld_w2", "ld_dw2"):
        assert lib.acm_gcn_bwd(handle, C.byref(_bwd(**{field: 4})), None, 0, None) == ESHAPE and b"acm_gcn_bwd" in err(), field
    for field in ("ld_h", "ld_g"):
        assert lib.acm_gcn_bwd(handle, C.byref(_bwd(**{field: 31})), None, 0, None) == ESHAPE, field
    assert lib.acm_gcn_bwd(handle, C.byref(_bwd(keep_scale=0.5)), None, 0, None) == ESHAPE


def test_new_parameter_blocks_have_the_c_layout(tmp_path):
    """The gcc offsets program of test_abi_cpu.py, for the structs this feature adds."""
    from acm_gnn_amd import _lib
    structs = {"acm_gcn_fwd_t": _lib.GcnFwd, "acm_gcn_bwd_t": _lib.GcnBwd}
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "acm_hip.h"', "int main(void){"]
    for cname, cls in structs.items():
        lines.append(f'printf("{cname} size %zu\\n", sizeof({cname}));')
        for fname, _ in cls._fields_:
            lines.append(f'printf("{cname} {fname} %zu\\n", offsetof({cname}, {fname}));')
    lines.append("return 0;}")
    src, exe = tmp_path / "layout.c", tmp_path / "layout"
    src.write_text("\n".join(lines))
    subprocess.check_call(["gcc", "-std=c11", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    got = {}
    for ln in subprocess.check_output([str(exe)], text=True).splitlines():
        s, f, v = ln.split()
        got[(s, f)] = int(v)
    for cname, cls in structs.items():
        assert got[(cname, "size")] == C.sizeof(cls), cname
        for fname, _ in cls._fields_:
            assert got[(cname, fname)] == getattr(cls, fname).offset, (cname, fname)


def _close(got, ref, tol):
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got.detach() if isinstance(got, torch.Tensor) else got, np.float64)
    bound = tol * max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(got - ref).max())
    assert err <= bound, (err, bound)


@pytest.mark.parametrize("mt", R.MODEL_TYPES)
def test_float64_restatement_reproduces_the_recorded_reference(case, a_low, mt):
    """Logits, loss, every gradient and the ten-step Adam trajectory the study's own code produced in fp32, at the project's fp32
    parity thresholds (2e-5 forward, 1e-4 gradients, relative to max(1, max |ref|); 5e-5 relative on the losses)."""
    params = R.case_params(case, mt)
    x, labels, idx = case["x"], case["labels"], case["train_idx"]
    _close(R.forward(params, mt, x, a_low), case[f"{mt}/logits"], 2e-5)
    loss, grads = R.loss_and_grads(params, mt, x, a_low, labels, idx)
    _close(loss, case[f"{mt}/loss"], 2e-5)
    recorded = {k[len(f"{mt}/grad/"):] for k in case if k.startswith(f"{mt}/grad/")}
    assert set(grads) == recorded                       # the same parameters are outside the forward
    for name in recorded:
        _close(grads[name], case[f"{mt}/grad/{name}"], 1e-4)
    traj = R.trajectory(params, mt, x, a_low, labels, idx, len(case[f"{mt}/traj"]))
    np.testing.assert_allclose(traj, case[f"{mt}/traj"], rtol=5e-5)


def test_unknown_model_type_and_acm_without_nnodes_are_refused():
    from acm_gnn_amd import baselines
    with pytest.raises(ValueError, match="model_type"):
        baselines.GCN(12, 32, 5, 0.5, "gat")
    with pytest.raises(ValueError, match="model_type"):
        baselines.GraphConvolution(12, 32, "acmgcn")
    for mt in ("acmgcn", "acmsgc"):
        with pytest.raises(ValueError, match="nnodes"):
            baselines.GCN(12, 32, 5, 0.5, mt)


@pytest.mark.parametrize("mt", ("mlp", "gcn", "sgc"))
def test_seeded_construction_draws_the_recorded_initial_values(case, mt, monkeypatch):
    """Same parameter names, in the reference's order, and -- drawn on the CPU generator from the fixture's seed -- the same
    values; the three 1 x 1 parameters the reference never initialises are zero."""
    from acm_gnn_amd import baselines, layers
    monkeypatch.setattr(baselines, "_default_device", lambda: torch.device("cpu"))
    monkeypatch.setattr(layers, "_default_device", lambda: torch.device("cpu"))
    torch.manual_seed(int(case["seed"]))
    model = baselines.GCN(case["x"].shape[1], int(case["hidden"]), int(case["classes"]), 0.0, mt)
    state = model.state_dict()
    recorded = R.case_params(case, mt)
    assert list(state) == list(recorded)
    for name, t in state.items():
        assert np.array_equal(t.numpy(), recorded[name]), name
        if name.endswith(("low_param", "high_param", "mlp_param")):
            assert float(t.abs().sum()) == 0.0


def test_acm_types_come_from_the_package_model():
    from acm_gnn_amd import baselines, layers, models
    assert isinstance(baselines.GCN(12, 32, 5, 0.5, "gcn"), baselines.BaselineGCN)
    model = baselines.GCN(12, 32, 5, 0.5, "acmgcn", nnodes=96)
    assert type(model) is models.GCN and model.model_type == "acmgcn" and model.structure_info == 0
    assert all(isinstance(m, layers.GraphConvolution) and not m.attn_layernorm for m in model.gcns)
    assert len(baselines.GCN(12, 32, 5, 0.5, "acmsgc", nnodes=96).gcns) == 1
