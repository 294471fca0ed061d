"""What a plain `bench.py` run does against `bench.py --full` (``-m gpu``): a plain run is set-up, warm-up, the timed steps
and the result line; only ``--full`` reports the strict-f32 variant and runs the CPU baseline and the secondary workloads.
Small batch: this checks what runs, not how fast."""

import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVED = ("strict_f32_variant", "cpu_baseline", "extra_summary", "extra_file", "extra_file_error")


def _line(*flags):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--batch", "4096", *flags]
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "TFMPC_LQR_MFMA")}
    res = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = [l for l in res.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, res.stdout
    return json.loads(lines[0])


def test_plain_run_measures_the_headline_only():
    line = _line()
    assert line["unit"] == "iterations/s" and line["higher_is_better"] is True and line["dtype"] == "f32"
    assert line["value"] > 0 and line["ms_per_step"] > 0 and line["status_flagged_instances"] == 0
    # the strict variant's 3 + max(1, steps // 2) launches still precede the warm-up, so the timed steps start where they always did
    assert line["untimed_launches_before_timing"] == 3 + 1 + 1
    assert not [k for k in MOVED if k in line] and "strict_f32_variant_frac" not in line["summary"]


def test_full_run_keeps_the_strict_f32_variant():
    line = _line("--full", "--no-extra", "--no-cpu-baseline")
    assert line["strict_f32_variant"]["kernel_ms"] > 0 and line["roofline"]["frac_strict_f32"] > 0
    assert line["untimed_launches_before_timing"] == 3 + 1 + 1
    assert "cpu_baseline" not in line and "extra_summary" not in line
