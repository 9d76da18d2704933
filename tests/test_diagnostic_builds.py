"""The diagnostic builds (csrc/egr_diag.hpp) and the bookkeeping that keeps them apart from the product (build.py, the package loader). No GPU:
every diagnostic switch must PARSE (hipcc -fsyntax-only with the build's flags), and the build directories are exercised with stub compilers."""
import importlib
import os
import stat
import subprocess
import sys

import pytest

PKG = "editable-gaussian-reflections_amd"
b = importlib.import_module(PKG + ".build")
SWITCHES = ["-DEGR_TRAVERSAL_STATS=1", "-DEGR_TASK_TIMES=1", "-DEGR_TASK_TIMES=8", "-DEGR_TASK_TIMES=9", "-DEGR_DEBUG_LIST=1", "-DEGR_DEBUG_PIXEL=0"]
ALL_TOGETHER = [["-DEGR_TRAVERSAL_STATS=1", "-DEGR_TASK_TIMES=" + n, "-DEGR_DEBUG_LIST=1", "-DEGR_DEBUG_PIXEL=0"] for n in ("1", "8", "9")]


@pytest.mark.parametrize("flags", [[s] for s in SWITCHES] + ALL_TOGETHER, ids=lambda f: "+".join(x[2:] for x in f))
def test_diagnostic_switch_parses(flags):
    """trace.hip (device pass: where the switches live) and api.hip (both passes: the host table and printer) under every switch and under all of them."""
    for src, extra in (("trace.hip", ["--cuda-device-only"]), ("api.hip", ['-DEGR_VARIANT_NAME="x"'])):
        r = subprocess.run([b.HIPCC] + b.HIP_FLAGS + flags + extra + ["-fsyntax-only", os.path.join(b.CSRC, src)], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert r.returncode == 0, (src, flags, r.stdout[-3000:])


def test_variant_name_is_a_pure_function_of_the_five_settings():
    assert b.variant_name({}) == "" and b.variant_dir({}) == b.OUT
    assert b.variant_name({"PATH": "/x", "EGR_TEAM_HELP": "1", "EGR_PRINT_TRAVERSAL_STATS": "1", "EGR_TRAVERSAL_STATS": ""}) == ""  # other settings, empty settings: the product
    assert b.variant_name({"EGR_TRAVERSAL_STATS": "1"}) == "stats"
    assert b.variant_name({"EGR_TASK_TIMES": "9"}) == "task_times_9"
    assert b.variant_name({"EGR_EXTRA_FLAGS": "-DEGR_GPOP=4"}) == "EGR_GPOP_4"
    assert b.variant_name({"EGR_TRAVERSAL_STATS": "1", "EGR_EXTRA_FLAGS": "-DEGR_GPOP=4,-DEGR_FPOP=2"}) == "stats-EGR_GPOP_4-EGR_FPOP_2"
    envs = [{"EGR_TRAVERSAL_STATS": "1"}, {"EGR_TASK_TIMES": "1"}, {"EGR_TASK_TIMES": "8"}, {"EGR_DEBUG_LIST": "1"}, {"EGR_DEBUG_PIXEL": "0"}, {"EGR_DEBUG_PIXEL": "7"},
            {"EGR_EXTRA_FLAGS": "-DEGR_GPOP=4"}, {"EGR_EXTRA_FLAGS": "-DEGR_GPOP=2"}, {"EGR_EXTRA_FLAGS": "-mllvm -amdgpu-sched-strategy=iterative-minreg"},
            {"EGR_EXTRA_FLAGS": "-mllvm -amdgpu-sched-strategy=iterative-minreg -DEGR_GPOP=4 -DEGR_FPOP=2 -DEGR_PSTK=96"},
            {"EGR_EXTRA_FLAGS": "-mllvm -amdgpu-sched-strategy=iterative-minreg -DEGR_GPOP=4 -DEGR_FPOP=2 -DEGR_PSTK=64"}]
    names = [b.variant_name(e) for e in envs]
    assert len(set(names)) == len(names) and all(n and len(n) <= 48 and "/" not in n and " " not in n for n in names), names  # distinct flags, distinct readable directories
    for e in envs:
        assert b.variant_name(dict(e, HOME="/somewhere", EGR_TEAM_HELP="0")) == b.variant_name(e)
        assert b.variant_dir(e) == os.path.join(b.OUT, "variants", b.variant_name(e)) and b.lib_paths(e)[0] == os.path.join(b.variant_dir(e), "libegr_hip.so")
        assert b.variant_flags(e) and not set(b.variant_flags(e)) & set(b.HIP_FLAGS)


@pytest.fixture()
def stub_build(tmp_path, monkeypatch):
    """build.py pointed at an empty output directory, with compilers that only write their output file and log their command line."""
    log = tmp_path / "commands.log"
    stub = tmp_path / "stubcc"
    stub.write_text('#!/bin/sh\necho "$@" >> "%s"\nwhile [ $# -gt 0 ]; do if [ "$1" = "-o" ]; then echo stub > "$2"; fi; shift; done\n' % log)
    stub.chmod(stub.stat().st_mode | stat.S_IXUSR)
    monkeypatch.setattr(b, "HIPCC", str(stub))
    monkeypatch.setattr(b, "CXX", str(stub))
    monkeypatch.setattr(b, "OUT", str(tmp_path / "build"))

    def commands():
        lines = log.read_text().splitlines() if log.exists() else []
        log.write_text("")
        return lines

    return commands


def _tree(root):
    return {os.path.relpath(os.path.join(d, f), root): os.path.getmtime(os.path.join(d, f)) for d, _, fs in os.walk(root) for f in fs if "variants" not in os.path.relpath(d, root).split(os.sep)}


def test_product_directory_is_rebuilt_when_its_recorded_flags_differ(stub_build):
    hip, torch_lib = b.build_all(env={})
    n = len(b.HIP_SOURCES) + 1
    first = stub_build()
    assert hip == os.path.join(b.OUT, "libegr_hip.so") and len(first) == n + 2 and not any("EGR_VARIANT_NAME" in c for c in first)  # n compiles, two links
    b.build_all(env={})
    assert stub_build() == []  # up to date: same flags, nothing newer
    # a leftover diagnostic library where the product belongs (what an in-place EGR_TRAVERSAL_STATS build of the old scheme left behind): newer than every source, other flags
    with open(os.path.join(b.OUT, b.FLAGS_FILE), "a") as f:
        f.write("-DEGR_TRAVERSAL_STATS=1\n")
    b.build_all(env={})
    again = stub_build()
    assert len(again) == n + 2 and not any("EGR_TRAVERSAL_STATS" in c for c in again)
    os.remove(os.path.join(b.OUT, b.FLAGS_FILE))  # a directory without a record (built before builds kept one) is stale too
    b.build_all(env={})
    assert len(stub_build()) == n + 2
    b.build_all(env={})
    assert stub_build() == []


def test_variant_build_never_writes_into_the_product_directory(stub_build):
    b.build_all(env={})
    stub_build()
    before = _tree(b.OUT)
    env = {"EGR_TRAVERSAL_STATS": "1", "EGR_EXTRA_FLAGS": "-DEGR_GPOP=4"}
    hip, torch_lib = b.build_all(env=env)
    cmds = stub_build()
    vdir = os.path.join(b.OUT, "variants", "stats-EGR_GPOP_4")
    assert os.path.dirname(hip) == vdir == os.path.dirname(torch_lib) and os.path.exists(hip) and os.path.exists(torch_lib)
    assert _tree(b.OUT) == before  # nothing of the product added, removed or touched
    compiles = [c for c in cmds if " -c " in c and ".hip" in c]
    assert len(compiles) == len(b.HIP_SOURCES) and all("-DEGR_TRAVERSAL_STATS=1" in c and "-DEGR_GPOP=4" in c and '-DEGR_VARIANT_NAME="stats-EGR_GPOP_4"' in c for c in compiles)
    outputs = [c.split(" -o ")[1].split()[0] for c in cmds]
    assert all(o.startswith(vdir + os.sep) for o in outputs), outputs  # its own objects, its own two libraries
    assert any("-L" + vdir in c and "-legr_hip" in c and "$ORIGIN" in c for c in cmds)  # libraytracer.so linked against the variant's libegr_hip.so
    b.build_all(env=env)
    b.build_all(env={})
    assert stub_build() == []  # both up to date, side by side


def test_loading_a_variant_that_is_not_built_names_it():
    """The settings that select a variant at build time select it at load time; if it is not there the loader says which and how to build it - no fallback to
    the product. (A fresh interpreter: the package reads the settings when it is imported.)"""
    code = ("import importlib, os\n"
            f"p = importlib.import_module({PKG!r})\n"
            "assert p.VARIANT == 'EGR_NO_SUCH_KNOB_1' and p.GAUSS_TRACER_PATH == os.path.join(p.BUILD_DIR, 'libraytracer.so') and p.BUILD_DIR.endswith(os.path.join('build', 'variants', 'EGR_NO_SUCH_KNOB_1'))\n"
            "try:\n    p.load_library()\nexcept RuntimeError as e:\n    print('RAISED', e)\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, "-c", code], cwd=root, env=dict(os.environ, EGR_EXTRA_FLAGS="-DEGR_NO_SUCH_KNOB=1"), stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0 and "RAISED" in r.stdout and "EGR_NO_SUCH_KNOB_1" in r.stdout and "tools/build_variant.sh" in r.stdout, r.stdout[-2000:]
    r = subprocess.run([sys.executable, "-c", f"import importlib; p = importlib.import_module({PKG!r}); print(p.VARIANT == '', p.GAUSS_TRACER_PATH)"], cwd=root,
                       env={k: v for k, v in os.environ.items() if k not in b.VARIANT_SETTINGS}, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.stdout.split() == ["True", os.path.join(os.path.dirname(b.CSRC), "build", "libraytracer.so")], r.stdout  # none set: the product, always
