"""bench.py command line: a plain run is lean, --full adds the TTFT
measurement, --dump-outputs writes reproducible outputs.  Runs the CPU
shrink (debug model) so it needs no GPU."""

import json
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).parent.parent


def _run_bench(*extra):
    env = {**os.environ, "PYTHONPATH": str(ROOT),
           # force the CPU shrink even on a GPU host
           "HIP_VISIBLE_DEVICES": "", "CUDA_VISIBLE_DEVICES": ""}
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        env.pop(k, None)
    proc = subprocess.run(
        [sys.executable, str(ROOT / "bench.py"), "--gpus", "1",
         "--steps", "3", "--warmup", "1", *extra],
        capture_output=True, text=True, env=env, timeout=300)
    assert proc.returncode == 0, proc.stderr[-2000:]
    lines = [ln for ln in proc.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, proc.stdout
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def bench_runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench")
    plain = _run_bench("--dump-outputs", str(d / "plain"))
    full = _run_bench("--full", "--dump-outputs", str(d / "full"))
    return d, plain, full


def test_result_line_fields(bench_runs):
    _, plain, full = bench_runs
    for res in (plain, full):
        assert res["steps"] == 3 and res["warmup"] == 1
        assert res["unit"] == "tokens/s" and res["higher_is_better"] is True
        assert res["dtype"] == "bf16"
        assert res["ms_per_step"] > 0
        batch = res["config"]["global_batch"]
        # value and ms_per_step describe the same timed region
        assert res["value"] == pytest.approx(
            batch / (res["ms_per_step"] / 1000), rel=1e-2)


def test_ttft_only_with_full(bench_runs):
    _, plain, full = bench_runs
    assert "p50_ttft_ms" not in plain["config"]
    assert full["config"]["p50_ttft_ms"] > 0


def test_dump_outputs_reproducible(bench_runs):
    d, plain, _ = bench_runs
    a = np.load(d / "plain" / "tokens.npy")
    b = np.load(d / "full" / "tokens.npy")
    assert a.dtype == np.float32
    assert a.shape == (plain["config"]["global_batch"],)
    assert (a == np.round(a)).all() and (a >= 0).all()
    # same arguments -> same inputs -> same outputs, with or without the
    # extra measurements
    np.testing.assert_array_equal(a, b)
