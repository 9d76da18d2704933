"""The `stats` diagnostic variant (EGR_TRAVERSAL_STATS=1, build/variants/stats/, built by __graft_entry__.build()) against the product: diagnostics
observe and never alter, and what they count is plausible. The variant runs in a fresh child process selected by its build-time setting
(tests/stats_variant_worker.py); the product runs here."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import hip_common as hc
from hip_common import ren  # noqa: F401
import stats_variant_worker as worker

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def parse_stats(text):
    """{launch: {group: {label: value}}} of the "=== <launch>" sections of the child's output ([egr stats <group>] <label> <value>[ wave-cycles], ...)."""
    out, cur = {}, None
    for line in text.splitlines():
        if line.startswith("=== "):
            cur = out.setdefault(line[4:].strip(), {})
        m = re.match(r"\[egr stats ([^\]]+)\] (.*)", line)
        if m and cur is not None:
            for item in m.group(2).split(", "):
                label, value = re.match(r"(.*) (\d+)(?: wave-cycles)?$", item).groups()
                cur.setdefault(m.group(1), {})[label] = int(value)
    return out


@pytest.fixture(scope="module")
def both(ren, tmp_path_factory):
    product = worker.run()
    npz = str(tmp_path_factory.mktemp("stats_variant") / "variant.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stats_variant_worker.py"), npz], cwd=ROOT, env=dict(os.environ, EGR_TRAVERSAL_STATS="1"),
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-4000:]
    info = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    z = np.load(info["npz"])
    variant = {launch: {k.split("/", 1)[1]: z[k] for k in z.files if k.startswith(launch + "/")} for launch in product}
    print(r.stdout[-6000:])
    return product, variant, info, parse_stats(r.stdout)


def test_child_ran_the_variant(both):
    _, _, info, _ = both
    assert info["variant"] == "stats" and info["version"].startswith("egr-hip 0.8 ") and "gfx950" in info["version"] and info["version"].endswith("stats"), info


@pytest.mark.parametrize("launch", ["nograd", "grad"])
def test_diagnostics_do_not_alter_the_launch(both, launch):
    product, variant, _, _ = both
    p, v = product[launch], variant[launch]
    assert sorted(p) == sorted(v)
    for k in hc.OUT_KEYS + ["num_traversed_per_pixel", "num_accumulated_per_pixel", "random_seeds", "counters"]:
        assert p[k].shape == v[k].shape and p[k].tobytes() == v[k].tobytes(), (launch, k, hc.mismatch_list(p[k].view(np.int32) if p[k].dtype == np.float32 else p[k], v[k].view(np.int32) if v[k].dtype == np.float32 else v[k]))
    assert p["counters"][0] == worker.W * worker.H and p["counters"][11] == 0
    for k in hc.GRAD_KEYS:  # float atomics add in varying order: like every help-off pair of launches
        assert np.abs(p[k] - v[k]).max() <= 1e-5 * max(float(np.abs(p[k]).max()), 1e-30), (launch, k)
    if launch == "grad":
        assert all(float(np.abs(p[k]).max()) > 0 for k in hc.GRAD_KEYS)


@pytest.mark.parametrize("launch", ["nograd", "grad"])
def test_what_the_diagnostics_count(both, launch):
    _, _, _, stats = both
    s = stats[launch]
    assert sum(s["primary lists"].values()) == (worker.W // 8) * (worker.H // 8) == 48, s["primary lists"]  # one entry per tile: the words are zeroed per launch
    inner = 0
    for cls in ("primary", "bounce"):
        assert s[cls]["lane node visits"] > 0 and s[cls]["lane leaf-box hits"] > 0 and s[cls]["wave inner iterations"] > 0, (cls, s[cls])
        inner += s[cls]["traversal"] + s[cls]["composite"]
    # exact: every wave's (traversal, composite, epilogue) intervals are disjoint and nested in its chain's, and s_memtime is monotonic
    assert 0 < inner + s["forward chain"]["step epilogues"] <= s["forward chain"]["whole chains (task pull to end)"], s
    rows = s["backward primary"]["hit rows"] + s["backward bounce"]["hit rows"]  # (counted by the row loop of primary tiles; the bounce steps' hits go through their queues)
    assert rows > 0 if launch == "grad" else rows == 0, rows
