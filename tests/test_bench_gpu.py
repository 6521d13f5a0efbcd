"""bench.py without --full times the headline and nothing else: one small plain run on cuda:0 (a fresh child process) carries the
contract's keys and its timed regions, none of the legs of a --full run, and --dump-outputs writes the last timed step's logits."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BENCH = os.path.join(ROOT, "bench.py")


def test_plain_run_times_the_headline_only(tmp_path):
    r = subprocess.run([sys.executable, BENCH, "--gpus", "1", "--steps", "3", "--warmup", "1", "--regions", "2",
                        "--dump-outputs", str(tmp_path)],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.strip()]
    line = json.loads(lines[-1])
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "dtype", "config"):
        assert k in line, k
    assert line["n_gpus"] == 1 and line["steps"] == 3 and line["warmup"] == 1 and line["scaling"] == "weak"
    assert line["unit"] == "samples/s" and line["higher_is_better"] is True and line["dtype"] == "bf16"
    assert line["value"] == pytest.approx(256 / (line["ms_per_step"] * 1e-3), rel=1e-3)
    # no leg of a --full run: no roofline, no CPU baseline or parity figure, no variant / one-at-a-time scalars, one scaling
    assert line["roofline"] is None and line["cpu_baseline"] is None
    assert not [k for k in line if k.startswith(("value_", "max_abs_logit_diff", "ms_per_step_"))]
    assert "weak_scaling" not in line and "strong_scaling" not in line
    detail = json.loads(next(ln for ln in lines if ln.startswith("bench_detail "))[len("bench_detail "):])
    for k in ("roofline_all", "variants", "small_batch", "stress", "text_pipeline", "trunks", "serial_replay"):
        assert k not in detail, k
    assert "xcd_map" not in detail["config"]
    regions = detail["timing"]["regions_ms_per_step"]
    assert len(regions) == 2 and line["ms_per_step"] in regions
    logits = np.load(str(tmp_path / "logits.npy"))
    assert os.listdir(str(tmp_path)) == ["logits.npy"]
    assert logits.dtype == np.float32 and logits.shape == (256, 3) and np.isfinite(logits).all()
