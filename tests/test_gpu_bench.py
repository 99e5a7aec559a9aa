"""GPU: a plain `bench.py` run — warm-up, exactly --steps timed steps, the headline line, and with --dump-outputs what
the last timed step returned: that step starts from the seeded weights, so two runs with the same arguments dump the
same arrays up to rounding."""

import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _plain_run(tmp_path, out):
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2",
                        "--workload", "tiny", "--dump-outputs", str(out)], cwd=str(tmp_path), capture_output=True,
                       text=True, timeout=600)
    assert p.returncode == 0, (p.stdout + p.stderr)[-3000:]
    lines = [line for line in p.stdout.strip().split("\n") if line.startswith("{")]
    assert len(lines) == 1
    return json.loads(lines[0]), {n: np.load(out / f"{n}.npy") for n in ("loss", "oce_loss", "offsets")}


def test_plain_run_prints_the_headline_and_dumps_the_last_step(tmp_path):
    rec, got = _plain_run(tmp_path, tmp_path / "out")
    assert rec["unit"] == "crops/s" and rec["higher_is_better"] is True and rec["dtype"].startswith("f32")
    assert rec["metric"].startswith("train crops/sec") and rec["steps"] == 3 and rec["warmup"] == 2
    # value and ms_per_step describe the same timed steps (batch 2 per step)
    assert rec["value"] > 0 and abs(rec["value"] - 2 * 1e3 / rec["ms_per_step"]) <= 1e-3 * rec["value"] + 0.01
    losses = rec["losses_from_first_step"]
    assert len(losses) == 2 + 3
    np.testing.assert_allclose(losses[-1], losses[0], rtol=1e-6)      # the last step is the first one again
    # nothing beside the headline: those objects come with --full
    for key in ("roofline", "train3d", "train2d_f32_mfma", "infer", "train_e2e", "cpu_baseline", "gpu_library_baseline"):
        assert key not in rec, key
    assert got["loss"].dtype == got["oce_loss"].dtype == np.float64 and got["offsets"].dtype == np.float32
    assert got["loss"].item() == losses[-1]
    assert got["offsets"].shape[0] == 2 and got["offsets"].size == 2 * 2 * 48 * 48 and np.isfinite(got["offsets"]).all()
    assert sum(a.nbytes for a in got.values()) <= 64 * 2 ** 20
    # the same arguments again: the same inputs, the same outputs up to rounding
    _rec2, again = _plain_run(tmp_path, tmp_path / "again")
    for n, a in got.items():
        np.testing.assert_allclose(again[n], a, rtol=1e-6, atol=1e-6 * max(1.0, float(np.abs(a).max())), err_msg=n)
