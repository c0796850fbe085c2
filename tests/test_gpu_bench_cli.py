"""bench.py as the driver launches it: the single-GPU command line, and the torch.distributed.run form with one rank
forced through the row-sharded path (RCCL collectives inside the captured step -- the closest a one-GPU box gets to the
N > 1 launch).  Both must exit 0 and print ONE JSON line carrying the contract's keys.  The checks, the roofline and the
side measurements are those of ``--full``; a plain run measures the headline alone."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
        "dtype", "data", "config", "roofline", "cpu_baseline"}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _run(cmd, env):
    res = subprocess.run(cmd, cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    lines = [ln for ln in res.stdout.decode().splitlines() if ln.strip().startswith("{")]
    assert res.returncode == 0, res.stderr.decode()[-3000:]
    assert len(lines) == 1, lines
    return json.loads(lines[0])


def test_single_gpu_command_line():
    env = dict(os.environ)
    d = _run([sys.executable, "bench.py", "--gpus", "1", "--steps", "10", "--warmup", "3", "--no-cpu-baseline",
              "--full"], env)
    assert KEYS <= set(d) and d["n_gpus"] == 1 and d["steps"] == 10 and d["config"]["checked"] is True
    assert d["roofline"]["bound"] == "hbm" and 0 < d["roofline"]["frac"] < 1
    assert d["config"]["launch"].startswith("hipGraph") and d["ms_per_step"] < 1.0
    assert "train_plus_eval_ms_per_epoch" in d["config"] and "literal_ms_per_step" in d["config"]


def test_torchrun_launch_with_collectives_in_the_captured_step():
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    d = _run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
              "--master-port", str(_free_port()), "bench.py", "--gpus", "1", "--steps", "10", "--warmup", "3",
              "--no-cpu-baseline", "--force-sharded", "--full"], env)
    assert KEYS <= set(d) and d["config"]["checked"] is True
    assert d["config"]["launch"].startswith("hipGraph"), d["config"]["launch"]
    assert d["config"]["shard"]["work_max_over_mean"] <= 1.05


def test_bench_starts_its_own_ranks():
    """``python bench.py --gpus N`` without a launcher around it starts one rank per GPU itself
    (bench.self_launch: torch.distributed.run, 127.0.0.1 rendezvous).  On the one-GPU box the same entry is reached with
    ``--gpus 1 --force-sharded``: RCCL initialised, the row-sharded step with its collectives captured, one JSON line."""
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    d = _run([sys.executable, "bench.py", "--gpus", "1", "--steps", "10", "--warmup", "3", "--no-cpu-baseline", "--force-sharded",
              "--full"], env)
    assert KEYS <= set(d) and d["n_gpus"] == 1 and d["config"]["checked"] is True
    assert d["config"]["launch"].startswith("hipGraph"), d["config"]["launch"]
    assert d["config"]["shard"]["work_max_over_mean"] <= 1.05


def test_plain_run_times_the_headline_alone_and_dumps_its_outputs(tmp_path):
    """``bench.py --gpus 1 --steps N --warmup W`` without --full: the headline figure only (no roofline, no CPU baseline, no
    oracle check), and ``--dump-outputs DIR`` writes the loss, parameters and gradients of the last timed step in float32."""
    env = dict(os.environ)
    out = tmp_path / "outputs"
    d = _run([sys.executable, "bench.py", "--gpus", "1", "--steps", "10", "--warmup", "3", "--dump-outputs", str(out)], env)
    assert KEYS <= set(d) and d["n_gpus"] == 1 and d["steps"] == 10 and d["warmup"] == 3
    assert d["roofline"] is None and d["cpu_baseline"] is None and d["config"]["checked"] is False
    assert d["config"]["launch"].startswith("hipGraph") and 0 < d["ms_per_step"] < 1.0
    import re
    import numpy as np
    nnz = int(re.search(r"nnz\(A_low\)=(\d+)", d["config"]["workload"]).group(1))
    assert abs(d["value"] - nnz / (d["ms_per_step"] * 1e-3)) <= 1e-3 * d["value"]
    names = sorted(p.name for p in out.iterdir())
    assert "loss.npy" in names and any(n.startswith("param.") for n in names) and any(n.startswith("grad.") for n in names)
    arrays = {n: np.load(out / n) for n in names}
    assert all(a.dtype == np.float32 and np.isfinite(a).all() for a in arrays.values())
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    assert abs(float(arrays["loss.npy"][0]) - d["config"]["final_loss"]) <= 1e-6 * max(1.0, abs(d["config"]["final_loss"]))
