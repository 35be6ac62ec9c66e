"""GPU: a plain `bench.py --gpus 1` run -- the headline only, its result line, and what --dump-outputs writes: the residual
history and the iterate x of the timed CG steps (checked against the oracle's CG and against ||b - A x||), the same arrays
for the same arguments in every run, a fixed sample of x where x is long."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_bench(args, out_dir):
    env = dict(os.environ, OMP_NUM_THREADS="1")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT", "BIS_FORCE_DIST", "BIS_BENCH_REHEARSE"):
        env.pop(k, None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", *args, "--dump-outputs", str(out_dir)],
                         capture_output=True, text=True, timeout=300, env=env, cwd=ROOT)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-3000:]
    lines = [ln for ln in out.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, out.stdout[-2000:]
    assert len(lines[0]) < 4096  # (a reader that keeps the last few KB of the output still has the whole line)
    return json.loads(lines[0])


def test_plain_run_and_its_outputs(tmp_path, oracle):
    n1, steps, warmup = 24, 9, 3
    j = run_bench(["--size", str(n1), "--steps", str(steps), "--warmup", str(warmup)], tmp_path)
    assert j["metric"].startswith("CG iterations/sec") and j["unit"] == "CG iterations/s" and j["higher_is_better"] is True
    assert j["dtype"] == "f64" and j["steps"] == steps and j["warmup"] == warmup and j["value"] > 0
    assert abs(j["ms_per_step"] - 1e3 / j["value"]) <= 1e-9 * j["ms_per_step"] and j["roofline"]["launches"] > 0
    # a plain run is the headline only: nothing that takes runs of its own
    for k in ("cpu_baseline", "parity_max_dr_over_r0", "compressed_stream", "crs_arrays_in_place", "target_512", "sweeps",
              "configs", "device_state_after_timed_region"):
        assert k not in j, k
    assert "measured_stream_GBs" not in j["roofline"]
    h, x = np.load(tmp_path / "residual_history.npy"), np.load(tmp_path / "x.npy")
    assert h.dtype == np.float64 and x.dtype == np.float64 and h.shape == (warmup + steps + 1,) and x.shape == (n1 ** 3,)
    assert h[0] == j["residual_r0"] and h[-1] == j["residual_last"]
    # the history is the CG's (the oracle's restatement of the reference), and x is the iterate of the last timed step
    A = oracle.gen_hpcg(n1)
    ref, _ = oracle.cg_run(A, warmup + steps, None)
    assert np.max(np.abs(h - ref[:len(h)])) <= 1e-10 * ref[0]
    true_res = np.linalg.norm(np.ones(A.n_rows) - oracle.spmv(A, x))
    assert abs(true_res - h[-1]) <= 1e-10 * h[0]


def test_outputs_repeat_and_long_x_is_sampled(tmp_path):
    """Above 2^21 rows x is written as x_sample: 2^21 fixed rows; two runs with the same arguments write the same arrays."""
    args = ["--size", "130", "--steps", "5", "--warmup", "1"]
    run_bench(args, tmp_path / "a")
    run_bench(args, tmp_path / "b")
    assert sorted(os.listdir(tmp_path / "a")) == ["residual_history.npy", "x_sample.npy"]
    for name in ("residual_history", "x_sample"):
        a, b = np.load(tmp_path / "a" / f"{name}.npy"), np.load(tmp_path / "b" / f"{name}.npy")
        assert a.dtype == np.float64 and a.shape == b.shape and np.all(np.isfinite(a))
        np.testing.assert_allclose(a, b, rtol=1e-12, atol=0)
    assert np.load(tmp_path / "a" / "x_sample.npy").shape == (1 << 21,)
