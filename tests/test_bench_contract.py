"""bench.py driver-contract tests: JSON line schema, and the exact
torchrun multi-rank launch the round-end driver uses (CPU/gloo here;
RCCL on the GPU box)."""

import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

REQUIRED_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup",
                 "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
                 "dtype", "data", "config"}


def _cpu_env():
    """Environment for the CPU/gloo multi-rank launches: the ranks stand
    in for one GPU each, so a machine with fewer GPUs than ranks must not
    hand them its devices (rank r would select GPU r). An out-of-range
    index leaves no device visible and the ranks take the CPU path."""
    env = dict(os.environ)
    env["HIP_VISIBLE_DEVICES"] = "-1"
    env["CUDA_VISIBLE_DEVICES"] = "-1"
    return env


def _parse_last_json(out: str):
    lines = [l for l in out.strip().splitlines() if l.startswith("{")]
    assert lines, f"no JSON line in output:\n{out[-2000:]}"
    return json.loads(lines[-1])


@pytest.mark.timeout(300)
def test_bench_single_process_cpu():
    r = subprocess.run(
        [sys.executable, "bench.py", "--steps", "4", "--warmup", "1",
         "--n_stocks", "24", "--seq_len", "5", "--num_factor", "4",
         "--hidden_size", "16", "--num_portfolio", "8", "--n_days", "2",
         "--engine", "eager"],
        cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _parse_last_json(r.stdout)
    assert REQUIRED_KEYS.issubset(d.keys())
    assert d["n_gpus"] == 1
    assert d["metric"] == "training cross-sections/sec"
    assert d["value"] > 0 and d["higher_is_better"] is True
    assert d["config"]["parallelism"] == "dp1"


_SMALL = ["--n_stocks", "24", "--seq_len", "5", "--num_factor", "4",
          "--hidden_size", "16", "--num_portfolio", "8", "--n_days", "2"]


def _run_dump(out_dir, extra):
    """One `--gpus 1 --steps 4 --warmup 2 --dump-outputs` run; returns
    the result line and the dumped arrays after the generic checks."""
    import numpy as np

    r = subprocess.run(
        [sys.executable, "bench.py", "--gpus", "1", "--steps", "4",
         "--warmup", "2", "--dump-outputs", str(out_dir)] + extra,
        cwd=REPO, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stderr[-2000:]
    d = _parse_last_json(r.stdout)
    assert REQUIRED_KEYS.issubset(d.keys())
    assert d["steps"] == 4 and d["warmup"] == 2
    # ms_per_step is the wall time of one timed step
    assert d["ms_per_step"] > 0
    assert abs(d["ms_per_step"] * d["value"] - 1000.0) < 1e-6 * 1000.0
    files = sorted(f for f in os.listdir(out_dir) if f.endswith(".npy"))
    arrays = {f[:-4]: np.load(os.path.join(out_dir, f)) for f in files}
    assert {"loss", "params"}.issubset(arrays)
    for name, a in arrays.items():
        assert a.dtype in (np.float32, np.float64), name
        assert a.size > 0 and np.isfinite(a).all(), name
    assert sum(a.nbytes for a in arrays.values()) <= 64 << 20
    return d, arrays


@pytest.mark.timeout(600)
def test_bench_dump_outputs_cpu_reproducible(tmp_path):
    """--dump-outputs writes the last timed step's loss and the trained
    parameters; equal arguments give equal inputs, hence equal dumps.
    --full is accepted and keeps the result line's meaning."""
    import numpy as np

    d1, a1 = _run_dump(tmp_path / "a", _SMALL + ["--engine", "eager"])
    d2, a2 = _run_dump(tmp_path / "b",
                       _SMALL + ["--engine", "eager", "--full"])
    assert d1["metric"] == d2["metric"] and d1["dtype"] == d2["dtype"]
    assert a1.keys() == a2.keys()
    for name in a1:
        assert a1[name].shape == a2[name].shape, name
        np.testing.assert_allclose(a1[name], a2[name], rtol=1e-5, atol=1e-6,
                                   err_msg=name)
    assert a1["params"].ndim == 1 and a1["loss"].shape == (1,)


@pytest.mark.gpu
@pytest.mark.timeout(300)
def test_bench_dump_outputs_fused_gpu(tmp_path):
    """The fused engine's dump: loss terms, the last step's
    reconstruction (one value per stock) and the parameter arena, at
    the flagship shapes."""
    d, a = _run_dump(tmp_path / "g", ["--engine", "fused"])
    assert d["config"]["engine"] == "fused"
    assert {"loss", "mse", "kl", "recon", "params"} == set(a)
    assert a["recon"].size == 300
    assert abs(float(a["loss"][0]) - float(a["mse"][0] + a["kl"][0])) \
        <= 1e-4 * max(1.0, abs(float(a["loss"][0])))


@pytest.mark.timeout(600)
def test_bench_torchrun_two_ranks_gloo():
    """Exactly the driver's launch shape (nnodes=1, nproc-per-node N,
    master-addr 127.0.0.1), CPU/gloo standing in for RCCL."""
    env = _cpu_env()
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
         "--master-port", "29571", "bench.py", "--gpus", "2",
         "--steps", "4", "--warmup", "1", "--n_stocks", "24",
         "--seq_len", "5", "--num_factor", "4", "--hidden_size", "16",
         "--num_portfolio", "8", "--n_days", "2", "--engine", "eager"],
        cwd=REPO, capture_output=True, text=True, timeout=540, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2000:])
    d = _parse_last_json(r.stdout)
    assert d["n_gpus"] == 2
    assert d["config"]["parallelism"] == "dp2"
    assert d["config"]["global_batch"] == 48
    assert d["scaling"] == "weak"


@pytest.mark.timeout(300)
def test_bench_forced_dist_world_size_1():
    """FV_FORCE_DIST=1: a single-process run initializes the real
    collective backend at world_size=1 (gloo on CPU; RCCL on a GPU box —
    the hardware smoke for the DP path) and still reports n_gpus=1."""
    env = dict(os.environ)
    env.update({"FV_FORCE_DIST": "1", "MASTER_ADDR": "127.0.0.1",
                "MASTER_PORT": "29572", "WORLD_SIZE": "1", "RANK": "0",
                "LOCAL_RANK": "0"})
    r = subprocess.run(
        [sys.executable, "bench.py", "--steps", "4", "--warmup", "1",
         "--n_stocks", "24", "--seq_len", "5", "--num_factor", "4",
         "--hidden_size", "16", "--num_portfolio", "8", "--n_days", "2",
         "--engine", "eager"],
        cwd=REPO, capture_output=True, text=True, timeout=240, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2000:])
    d = _parse_last_json(r.stdout)
    assert d["n_gpus"] == 1
    assert d["config"]["parallelism"] == "dp1"


@pytest.mark.timeout(600)
def test_bench_torchrun_four_ranks_gloo():
    """4-rank ladder rung of the driver's SCALE launch (CPU/gloo)."""
    env = _cpu_env()
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "4", "--master-addr", "127.0.0.1",
         "--master-port", "29573", "bench.py", "--gpus", "4",
         "--steps", "4", "--warmup", "1", "--n_stocks", "16",
         "--seq_len", "4", "--num_factor", "4", "--hidden_size", "16",
         "--num_portfolio", "8", "--n_days", "2", "--engine", "eager"],
        cwd=REPO, capture_output=True, text=True, timeout=540, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2000:])
    d = _parse_last_json(r.stdout)
    assert d["n_gpus"] == 4
    assert d["config"]["parallelism"] == "dp4"
    assert d["config"]["global_batch"] == 64


@pytest.mark.timeout(600)
def test_bench_torchrun_eight_ranks_gloo():
    """Full-node rung of the driver's SCALE launch (nproc-per-node 8,
    CPU/gloo): the exact width the round-end 8×MI355X run uses, incl.
    n_days(2) < world_size(8) — wrap-padding must keep all 8 ranks in
    lockstep."""
    env = _cpu_env()
    r = subprocess.run(
        [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
         "--nproc-per-node", "8", "--master-addr", "127.0.0.1",
         "--master-port", "29574", "bench.py", "--gpus", "8",
         "--steps", "3", "--warmup", "1", "--n_stocks", "12",
         "--seq_len", "4", "--num_factor", "3", "--hidden_size", "16",
         "--num_portfolio", "6", "--n_days", "2", "--engine", "eager"],
        cwd=REPO, capture_output=True, text=True, timeout=540, env=env)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-2000:])
    d = _parse_last_json(r.stdout)
    assert d["n_gpus"] == 8
    assert d["config"]["parallelism"] == "dp8"
    assert d["config"]["global_batch"] == 96
