"""In-tree build of the two native artefacts (no cmake, no JIT cache):

  libegr_hip.so    hipcc --offload-arch=gfx950   csrc/{trace,bvh,api,knn,step,denoise,prune,grow,edit,eval,ssim,frames,initcloud,viewset,priors}.hip   the C-ABI product (include/egr_raytracer.h)
  libraytracer.so  g++ against the installed torch  csrc/torch_binding.cpp                 TORCH_LIBRARY(raytracer) shim

The PRODUCT lives in build/. A build with any of the five build-time settings (VARIANT_SETTINGS: the diagnostic switches of csrc/egr_diag.hpp and
EGR_EXTRA_FLAGS) is a VARIANT with objects and libraries of its own in build/variants/<variant_name>/, selected by the same settings when the package
loads (__init__.py): a diagnostic or sweep build never replaces the product. Every build directory records its flag list (FLAGS_FILE); a target is
stale if a source is newer or the recorded flags differ.

hipcc cross-compiles gfx950 without a GPU; the .so files travel to the GPU box with the repo snapshot.
"""
import hashlib
import os
import re
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OUT = os.path.join(HERE, "build")
ROOT = os.path.dirname(HERE)
HIP_LIB = os.path.join(OUT, "libegr_hip.so")
TORCH_LIB = os.path.join(OUT, "libraytracer.so")
FLAGS_FILE = "flags.txt"

HIPCC = os.environ.get("HIPCC", shutil.which("hipcc") or "/opt/rocm/bin/hipcc")
CXX = os.environ.get("CXX", "g++")
# -fno-slp-vectorize: on gfx950 a v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 takes longer than the two scalar instructions it replaces (tools/ubench/valu_rate.hip:
# 6.9 vs 2 x 3.1 cycles per SIMD), and the SLP vectoriser packs every adjacent pair of fp32 operations it finds (both chains -5 ... -7 % without it)
HIP_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-fno-slp-vectorize", "-Wno-unused-result"]
# (tuning knobs - EGR_GPOP, EGR_FPOP, EGR_PSTK, EGR_TEAM, EGR_BOX, EGR_DONATE_MIN, EGR_FWD_WAVES, EGR_BWD_WAVES, EGR_BWD_TEAM, EGR_GT_SLOTS, EGR_ORDER_BUCKETS, EGR_ORDER_SHIFT:
# numeric constants with an #ifndef default in csrc/ - are set for a sweep through EGR_EXTRA_FLAGS="-DEGR_GPOP=4"; the alternative code paths that rounds 1-5 switched
# between at build time are settled and gone: profiles/HISTORY.md has their measurements)
VARIANT_SETTINGS = ("EGR_TRAVERSAL_STATS", "EGR_TASK_TIMES", "EGR_DEBUG_LIST", "EGR_DEBUG_PIXEL", "EGR_EXTRA_FLAGS")
HIP_SOURCES = ["trace.hip", "bvh.hip", "api.hip", "knn.hip", "step.hip", "denoise.hip", "prune.hip", "grow.hip", "edit.hip", "eval.hip", "ssim.hip", "frames.hip", "initcloud.hip", "viewset.hip", "priors.hip"]
HEADERS = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".hpp", ".inc"))) + [os.path.join(ROOT, "include", "egr_raytracer.h")]  # every object depends on all of them
_POOL = ThreadPoolExecutor(8)  # compilers at once, over all builds of this process (trace.hip alone takes longer than the rest together; not sized by the CPU count)


def variant_flags(env):
    """The compiler flags the five build-time settings of `env` (a mapping) add; [] = the product."""
    f = []
    if env.get("EGR_EXTRA_FLAGS"):  # compiler-flag experiments, e.g. "-mllvm -amdgpu-sched-strategy=iterative-minreg", and tuning knobs ("-DEGR_GPOP=4")
        f += env["EGR_EXTRA_FLAGS"].replace(",", " ").split()
    if env.get("EGR_TASK_TIMES"):  # per-task stamps in the stats images: <step> (tools/task_times.py), 9 = whole forward chain (chain_times.py), 8 = backward chain (bwd_times.py)
        f.append("-DEGR_TASK_TIMES=" + env["EGR_TASK_TIMES"])
    if env.get("EGR_DEBUG_PIXEL"):
        f.append("-DEGR_DEBUG_PIXEL=" + env["EGR_DEBUG_PIXEL"])
    if env.get("EGR_DEBUG_LIST"):
        f.append("-DEGR_DEBUG_LIST=1")
    if env.get("EGR_TRAVERSAL_STATS"):
        f.append("-DEGR_TRAVERSAL_STATS=1")
    return f


def variant_name(env):
    """Readable name of the build the five settings of `env` select: "" = the product, else e.g. "stats", "task_times_9", "EGR_GPOP_4" (long ones hashed).
    The build and the package loader both go through this, so what selects a variant at build time selects the same library at load time."""
    parts = ["stats"] if env.get("EGR_TRAVERSAL_STATS") else []
    if env.get("EGR_TASK_TIMES"):
        parts.append("task_times_" + env["EGR_TASK_TIMES"])
    if env.get("EGR_DEBUG_LIST"):
        parts.append("debug_list")
    if env.get("EGR_DEBUG_PIXEL"):
        parts.append("debug_pixel_" + env["EGR_DEBUG_PIXEL"])
    parts += [f[2:] if f.startswith("-D") else f for f in (env.get("EGR_EXTRA_FLAGS") or "").replace(",", " ").split()]
    name = "-".join(re.sub(r"[^A-Za-z0-9.]+", "_", p).strip("_") for p in parts)
    if len(name) > 48 or (parts and not name):
        name = (name[:32].rstrip("_-") + "-" if name else "") + hashlib.sha1(" ".join(variant_flags(env)).encode()).hexdigest()[:10]
    return name


def variant_dir(env):
    name = variant_name(env)
    return os.path.join(OUT, "variants", name) if name else OUT


def lib_paths(env):
    """(libegr_hip.so, libraytracer.so) of the build `env` selects."""
    d = variant_dir(env)
    return os.path.join(d, "libegr_hip.so"), os.path.join(d, "libraytracer.so")


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def _run(cmd):
    r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if r.returncode != 0:
        sys.stderr.write(" ".join(cmd) + "\n" + r.stdout + "\n")
        raise RuntimeError("native build failed: " + os.path.basename(cmd[0]))
    return r.stdout


def _torch_compile_flags():
    import torch
    from torch.utils import cpp_extension

    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    return ["-O2", "-std=c++17", "-fPIC", "-D__HIP_PLATFORM_AMD__=1", "-DUSE_ROCM=1", f"-D_GLIBCXX_USE_CXX11_ABI={int(torch._C._GLIBCXX_USE_CXX11_ABI)}",
            "-Wno-deprecated-declarations"] + ["-I" + p for p in cpp_extension.include_paths()] + ["-I" + os.path.join(rocm, "include")]


def build_all(force=False, verbose=False, env=None):
    """Build the product (env without any of VARIANT_SETTINGS; default: os.environ) or the variant `env` selects, in its own directory.
    Returns (libegr_hip.so, libraytracer.so)."""
    import torch

    env = os.environ if env is None else env
    out, name = variant_dir(env), variant_name(env)
    hip_lib, torch_lib = lib_paths(env)
    hip_flags = HIP_FLAGS + variant_flags(env) + (['-DEGR_VARIANT_NAME="%s"' % name] if name else [])
    torch_flags = _torch_compile_flags()
    os.makedirs(out, exist_ok=True)
    record = " ".join(hip_flags + ["|"] + torch_flags) + "\n"
    flags_path = os.path.join(out, FLAGS_FILE)
    if not (os.path.exists(flags_path) and open(flags_path).read() == record):
        force = True  # built with other flags (or by a build that kept no record): everything in this directory is stale
        if os.path.exists(flags_path):
            os.remove(flags_path)
    jobs, objs = [], []
    for src in HIP_SOURCES + ["torch_binding.cpp"]:
        s = os.path.join(CSRC, src)
        o = os.path.join(out, os.path.splitext(src)[0] + ".o")
        objs.append(o)
        if force or _newer(o, [s] + HEADERS):
            cmd = [HIPCC] + hip_flags if src.endswith(".hip") else [CXX] + torch_flags
            if verbose:
                print(os.path.basename(cmd[0]), src, ("[" + name + "]") if name else "", flush=True)
            jobs.append(_POOL.submit(_run, cmd + ["-c", s, "-o", o]))
    for j in jobs:
        j.result()
    if jobs or _newer(hip_lib, objs[:-1]):
        _run([HIPCC, "--offload-arch=gfx950", "-shared", "-fPIC"] + objs[:-1] + ["-o", hip_lib])
    if jobs or _newer(torch_lib, [objs[-1], hip_lib]):
        tdir = os.path.dirname(torch.__file__)
        _run([CXX, "-shared", objs[-1], "-o", torch_lib, "-L" + os.path.join(tdir, "lib"), "-L" + out, "-legr_hip", "-lc10", "-lc10_hip", "-ltorch_cpu", "-ltorch_hip",
              "-ltorch", "-Wl,-rpath,$ORIGIN", "-Wl,--no-as-needed"])
    if not os.path.exists(flags_path):
        with open(flags_path, "w") as f:
            f.write(record)
    return hip_lib, torch_lib


if __name__ == "__main__":  # build what the environment selects; the last line printed is its directory (tools/build_variant.sh)
    build_all(force="--force" in sys.argv, verbose=True)
    print(variant_dir(os.environ))
