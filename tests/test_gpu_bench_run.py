"""bench.py as the driver runs it: a plain run times exactly --steps steps and prints the headline line only,
--dump-outputs writes what the last timed step computed, and --full still carries the companion figures."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
HEADLINE = ("metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step")


def _bench(*argv):
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "CLIMA_BENCH_FORCE_DIST")}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1"] + list(argv),
                       env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


def test_plain_run_and_dumped_outputs(tmp_path):
    d = tmp_path / "out"
    line = _bench("--steps", "7", "--warmup", "2", "--dump-outputs", str(d))
    for k in HEADLINE:
        assert k in line, k
    assert line["steps"] == 7 and line["warmup"] == 2
    assert line["unit"] == "calls/s" and line["higher_is_better"] is True and line["dtype"] == "f64"
    assert line["ms_per_step"] > 0 and abs(line["value"] * line["ms_per_step"] - 1e3) < 1e-6 * line["value"] * line["ms_per_step"]
    for k in ("roofline", "cpu_baseline", "resident_sync", "rce_jacobian_batch", "repeats_calls_per_s"):
        assert k not in line, k                      # measured with --full only
    nz = 200
    out = {f[:-4]: np.load(str(d / f)) for f in os.listdir(str(d))}
    assert sum(a.nbytes for a in out.values()) <= 64 << 20
    for k in ("ir_fup_n", "ir_fdn_n", "sol_fup_n", "sol_fdn_n", "f_total"):
        assert out[k].shape == (nz + 1,), k
    for k in ("ir_fup_a", "ir_fdn_a", "sol_fup_a", "sol_fdn_a", "sol_amean"):
        assert out[k].shape[0] == nz + 1, k
    for k in ("ir_tau_band", "sol_tau_band"):
        assert out[k].shape[0] == nz, k
    for k, a in out.items():
        assert a.dtype == np.float64 and np.all(np.isfinite(a)), k
    olr = -(out["ir_fdn_n"][nz] - out["ir_fup_n"][nz])
    isr = out["sol_fdn_n"][nz] - out["sol_fup_n"][nz]
    assert olr > 0 and isr > 0
    assert abs(olr / 1e3 - line["olr_W_m2"]) <= 1e-12 * abs(line["olr_W_m2"])
    assert abs(isr / 1e3 - line["isr_W_m2"]) <= 1e-12 * abs(line["isr_W_m2"])


def test_full_run_keeps_the_companion_figures():
    line = _bench("--full", "--steps", "5", "--warmup", "2", "--repeats", "1", "--no-cpu-baseline", "--no-jacobian")
    for k in HEADLINE:
        assert k in line, k
    assert line["steps"] == 5
    for k in ("roofline", "algorithmic", "repeats_calls_per_s", "resident_sync", "sync_api_c", "sync_api"):
        assert k in line, k
