"""bench.py's contract: a plain run prints one line with the headline figures and nothing that needs runs of its own (those are behind --full),
--steps sets the number of timed steps, and --dump-outputs writes what the last timed step returned to its caller, within 64 MB."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

GRADS = {"grad_xyz": 3, "grad_opacity": 1, "grad_scaling": 3, "grad_rotation": 4, "grad_diffuse": 3, "grad_normal": 3, "grad_roughness": 1, "grad_f0": 3}
FULL_ONLY = ("roofline", "cpu_baseline", "kernel_ms", "primary_only", "team_help_off", "other_variant", "multi_gpu")


def test_dump_sample_is_fixed_and_bounded():
    x = np.arange(5000 * 3, dtype=np.float32).reshape(1, 5000, 3)
    small = bench.dump_sample(x, 5000)
    assert small is x  # within the limit: the array itself
    a, b = bench.dump_sample(x, 100), bench.dump_sample(x, 100)
    assert a.shape == (100, 3) and np.array_equal(a, b)  # the same rows in every run
    rows = a[:, 0] / 3
    assert np.all(np.diff(rows) > 0) and np.array_equal(a, x.reshape(-1, 3)[rows.astype(np.int64)])  # whole rows, ascending, no repeats


def test_largest_dump_fits_64_mb():
    render = bench.DUMP_PIXEL_ROWS * 3 * 4
    grads = bench.DUMP_GAUSSIAN_ROWS * sum(GRADS.values()) * 4
    assert render + grads <= 64 << 20


def _bench(tmp_path, tag, *extra):
    out = tmp_path / tag
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "2", "--width", "480", "--height", "272",
           "--gaussians", "30000", "--dump-outputs", str(out)] + list(extra)
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-4000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0]), {f[:-4]: np.load(out / f) for f in os.listdir(out)}


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_run_is_lean_and_dumps_the_last_step(tmp_path):
    d, arrays = _bench(tmp_path, "a")
    assert d["steps"] == 3 and d["ms_per_step"] > 0 and d["value"] > 0 and d["status"] == 0
    assert d["unit"] == "Mrays/s" and d["higher_is_better"] is True and d["dtype"] == "f32" and d["metric"].startswith("Mrays/s fwd+bwd")
    assert d["full"] is False and not any(k in d for k in FULL_ONLY)
    assert sorted(arrays) == sorted(GRADS) == d["outputs"]["names"]  # a training step hands its caller the gradients
    for k, c in GRADS.items():
        assert arrays[k].shape == (30000, c) and arrays[k].dtype == np.float32 and np.isfinite(arrays[k]).all(), k
    assert np.abs(arrays["grad_opacity"]).max() > 0 and np.abs(arrays["grad_diffuse"]).max() > 0
    # the same arguments give the same inputs: a second process computes the same step (sums of float atomics: equal up to their order)
    _, again = _bench(tmp_path, "b")
    for k in GRADS:
        assert np.abs(arrays[k] - again[k]).max() <= 1e-4 * np.abs(arrays[k]).max() + 1e-30, k
    # a no-grad render hands its caller the image
    d, img = _bench(tmp_path, "c", "--forward-only")
    assert d["metric"].startswith("Mrays/s fwd-only") and sorted(img) == ["render"]
    assert img["render"].shape == (3, 272, 480, 3) and img["render"].dtype == np.float32 and np.isfinite(img["render"]).all()
    assert np.abs(img["render"]).max() > 0
