"""bench.py's two modes: a plain run prints the headline alone; `--full` adds the other measurements and the comparison with the
reference, and times the same steps with the same outputs."""
from __future__ import annotations

import json
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

import bench

ROOT = Path(__file__).resolve().parents[1]
FULL_ONLY = ("cpu_baseline", "drop_in_python", "e2e", "configs")


def test_full_is_off_by_default():
    assert bench.parse_args([]).full is False
    assert bench.parse_args(["--full"]).full is True


def _run(tmp_path: Path, name: str, *extra: str) -> dict:
    cmd = [sys.executable, str(ROOT / "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--size-mb", "8", "--side-mb", "8",
           "--dump-outputs", str(tmp_path / name), *extra]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


@pytest.mark.gpu
def test_plain_run_is_the_headline_and_full_adds_the_rest(tmp_path):
    plain = _run(tmp_path, "plain")
    full = _run(tmp_path, "full", "--full")
    for j in (plain, full):
        assert j["unit"] == "GB/s" and j["higher_is_better"] is True and j["dtype"] == "u8"
        assert j["value"] > 0 and j["ms_per_step"] > 0 and j["steps"] == 3 and j["warmup"] == 2
    assert not any(k in plain for k in FULL_ONLY)
    assert plain["config"]["verified_vs_oracle"] is None
    assert "per_kernel" not in plain["roofline"] and "whole_step" in plain["roofline"]
    assert all(k in full for k in FULL_ONLY)
    assert full["config"]["verified_vs_oracle"]
    assert full["roofline"]["per_kernel"] and full["roofline"]["fixed_overhead_us"]
    assert full["launch_mode"]["ms_per_step_plain_launches"] and full["launch_mode"]["ms_per_step_graph_replay"]
    for key, c in full["configs"].items():
        assert "error" not in c and not str(c["verified_vs_oracle"]).startswith("MISMATCH"), (key, c)
    assert plain["config"]["tokens"] == full["config"]["tokens"]
    for f in sorted(plain["dumped_outputs"]["files"]):
        assert np.array_equal(np.load(tmp_path / "plain" / f), np.load(tmp_path / "full" / f)), f
