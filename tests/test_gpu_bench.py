"""bench.py's result line: a plain run prints the headline (and --dump-outputs' arrays) and runs nothing else after its
timed steps; --full adds the per-kernel breakdown, the roofline and the other legs.  Two short runs in child processes."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")
FULL_ONLY = ("kernel_ms_per_scan", "roofline", "sharded_rccl_one_rank", "sharded", "sharded_config5", "wref", "config5",
             "parity", "parity_checked", "cpu_baseline")


def _bench(*extra):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1"]
                       + list(extra), cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert len(lines) == 1, r.stdout[-3000:]
    return json.loads(lines[0])


def test_plain_run_prints_the_headline_and_nothing_else(tmp_path):
    out = _bench("--dump-outputs", str(tmp_path))
    assert all(k in out for k in HEADLINE), sorted(out)
    assert out["unit"] == "scans/s" and out["higher_is_better"] is True
    assert out["steps"] == 2 and out["warmup"] == 1 and out["n_gpus"] == 1
    assert out["value"] > 0 and out["value"] * out["ms_per_step"] == pytest.approx(1e3)
    assert not set(FULL_ONLY) & set(out), sorted(set(FULL_ONLY) & set(out))
    assert out["config"]["C"] > 0 and out["config"]["N_hi"] == 64 * 1024
    assert sorted(out["dump_outputs"]["arrays"]) == sorted(f[:-len(".npy")] for f in os.listdir(tmp_path))


def test_full_run_adds_the_kernel_breakdown_and_the_roofline():
    out = _bench("--full", "--no-pmc", "--no-wref", "--no-config5", "--no-cpu-baseline")
    assert all(k in out for k in HEADLINE), sorted(out)
    assert sorted(out["kernel_ms_per_scan"]) == ["csm_eval", "insert", "rtcsm_rescore", "rtcsm_score", "rtcsm_select"]
    assert all(v > 0 for k, v in out["kernel_ms_per_scan"].items() if k != "rtcsm_rescore"), out["kernel_ms_per_scan"]
    assert out["roofline"]["kernel"] == "rtcsm_score_box_kernel" and out["roofline"]["launches"] == 2
    assert "sharded_rccl_one_rank" in out
    assert not {"wref", "config5", "parity", "cpu_baseline"} & set(out)
