"""bench.py without --full: set-up, warm-up, the timed steps and the headline's line -- no other leg.

(What --full adds takes tens of seconds and is run by whoever wants those figures; here only the plain run, the one
every change is measured with several times over.)"""
import json
import os
import subprocess
import sys
import time

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# the line of a plain one-GPU run: the headline and what the timed steps themselves measured
PLAIN_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "prewarm_ms", "ms_per_step", "higher_is_better",
              "scaling", "vs_baseline", "dtype", "data", "config", "roofline", "kernels", "pixel_path"}
# ... whose kernel classes are those of the headline's step
PLAIN_KERNELS = {"iiwt_finest", "iiwt_coarse", "iiwt_3_levels", "obmc", "upsample"}
# the issue's bound for a plain run: seconds from start to exit, less its warm-up and timed steps
OUTSIDE_STEPS_S = 30.0


def test_plain_run_is_the_headline_alone():
    steps, warmup = 3, 1
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    t0 = time.perf_counter()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        str(warmup)], env=env, capture_output=True, text=True, timeout=300)
    wall = time.perf_counter() - t0
    assert p.returncode == 0, p.stdout[-1000:] + p.stderr[-3000:]
    lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1
    out = json.loads(lines[0])
    assert out["metric"] == "Mpix/s IIWT+OBMC decode, 2160p s16" and out["unit"] == "Mpix/s" and out["dtype"] == "s16"
    assert out["higher_is_better"] is True and out["n_gpus"] == 1 and out["steps"] == steps and out["warmup"] == warmup
    assert out["value"] > 0 and out["ms_per_step"] > 0
    # value and ms_per_step are the same measurement: 8 pictures of 3840 x 2160 per step
    assert out["value"] == pytest.approx(8 * 3840 * 2160 / (out["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    assert set(out) == PLAIN_KEYS, sorted(set(out) ^ PLAIN_KEYS)
    assert set(out["kernels"]) <= PLAIN_KERNELS and "obmc" in out["kernels"], sorted(out["kernels"])
    outside = wall - (steps + warmup) * out["ms_per_step"] * 1e-3
    print("plain run: %.2f s from start to exit, %.2f s outside its steps" % (wall, outside))
    assert outside <= OUTSIDE_STEPS_S
