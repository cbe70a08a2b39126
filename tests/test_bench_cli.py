"""bench.py's command line: a plain run times the headline steps only, --full adds the
other legs, --dump-outputs writes what the last timed step computed.

CPU: the options exist and a bad step count is refused before anything is imported.
GPU: one plain run in a child process (as the benchmark is run) -- the line's fields,
and the dumped recovery shards against the CPU oracle's encode of the same seeded input.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_bench_help_lists_full_and_dump_outputs():
    r = subprocess.run([sys.executable, BENCH, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs DIR" in r.stdout


def test_bench_refuses_zero_steps():
    r = subprocess.run([sys.executable, BENCH, "--steps", "0"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 2 and "--steps" in r.stderr


@pytest.mark.gpu
def test_bench_full_run_carries_the_other_legs():
    """--full with the slow legs switched off: the decode and roofline blocks are in the line."""
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--full",
                        "--profile-steps", "3", "--no-cpu", "--no-host", "--no-object", "--no-copy",
                        "--no-configs", "--no-sharded", "--batch", "1"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.strip().splitlines()[-1])
    assert line["full"] is True and line["steps"] == 3 and line["ms_per_step"] > 0
    assert line["roofline"]["kernel"] and line["gpu_event_ms_per_step"] > 0
    assert line["decode_GiBps"]["1pct"] > 0 and line["decode_GiBps"]["100pct"] > 0


@pytest.mark.gpu
def test_bench_plain_run_line_and_dump(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import bench
    import oracle_lib as O

    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(tmp_path)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, "a plain run prints the result line and nothing else"
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "GiB/s" and line["dtype"] == "u8"
    assert line["higher_is_better"] is True and line["steps"] == 3 and line["warmup"] == 1
    assert line["full"] is False
    N, M, S = bench.CONFIGS[bench.HEADLINE]
    assert line["value"] == pytest.approx((N + M) * S / (line["ms_per_step"] / 1e3) / 2**30, rel=1e-3)
    # nothing but the headline steps ran
    for key in ("roofline", "decode_GiBps", "batched", "host_e2e", "object_api", "cpu_baseline",
                "device_copy", "sharded", "config3", "config4"):
        assert key not in line
    assert os.listdir(tmp_path) == ["recovery.npy"]
    got = np.load(tmp_path / "recovery.npy")
    assert got.dtype == np.float32 and got.shape == (M, S)
    orig, _ = bench.stripe_inputs(bench.HEADLINE, 0, torch.device("cuda", 0))
    want = O.encode("default", orig.cpu().numpy(), M)
    assert np.array_equal(got, want.astype(np.float32)), "dumped recovery shards differ from the oracle's encode"
