"""`bench.py --dump-outputs DIR` on the real engine: a plain run writes the
last timed step's logits and box encodings, and two runs with the same
arguments write the same bits (seeded inputs and weights)."""
import glob
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _bench(out_dir):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1",
           "--steps", "2", "--warmup", "1", "--preset", "car", "--frames",
           "3", "--frames-per-step", "2", "--dump-outputs", str(out_dir)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    lines = [json.loads(l) for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1
    return lines[0]


def test_plain_bench_dumps_the_last_step_deterministically(tmp_path):
    a, b = tmp_path / "a", tmp_path / "b"
    r = _bench(a)
    _bench(b)
    # a plain run: one region of exactly --steps steps, headline only
    assert r["steps"] == 2 and r["config"]["repeat_ms_per_step"]["n"] == 1
    assert r["config"]["frames_timed"] == 2 * 2
    assert r["dtype"] == "f32" and r["ms_per_step"] > 0
    for key in ("roofline", "roofline_mfma", "cpu_baseline"):
        assert key not in r
    names = sorted(os.path.basename(p) for p in glob.glob(str(a / "*.npy")))
    assert names == ["frame0_box_encodings.npy", "frame0_logits.npy",
                     "frame1_box_encodings.npy", "frame1_logits.npy"]
    for j in (0, 1):
        lg = np.load(str(a / ("frame%d_logits.npy" % j)))
        bx = np.load(str(a / ("frame%d_box_encodings.npy" % j)))
        assert lg.dtype == np.float32 and bx.dtype == np.float32
        assert lg.ndim == 2 and bx.ndim == 3 and bx.shape[:2] == lg.shape
        assert lg.shape[0] > 0 and np.isfinite(lg).all() and \
            np.isfinite(bx).all()
    for n in names:
        assert np.array_equal(np.load(str(a / n)), np.load(str(b / n))), n
