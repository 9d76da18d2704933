"""ctypes front-end for the reference's own shader code built for the CPU (oracle/ref_driver.cpp -> oracle/_ref/libegr_reference.so).

TEST INFRASTRUCTURE ONLY. `Reference` has the interface of oracle.Oracle, so a test feeds both the same calls; everything it returns is fp32, as the
reference's tensors are. The library exists only where the reference's sources were present when build() ran (`available()`): nothing that has to
run without them - the GPU tests, smoke(), bench.py - may import this module's results except through fixtures under tests/golden/.
"""
import ctypes
import os
import subprocess

import numpy as np

from .oracle import CONFIG_FIELDS, GAUSSIAN_FIELDS, NSTEPS

_HERE = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_HERE, "_ref", "libegr_reference.so")
_lib = None

OUT_KEYS = ["output_rgb", "output_depth", "output_normal", "output_f0", "output_roughness", "output_transmittance", "output_total_transmittance",
            "output_ray_origin", "output_ray_direction", "output_final"]  # order of core/framebuffer.h
_OUT_CH = [3, 1, 3, 3, 1, 1, 1, 3, 3, 3]
GRAD_KEYS = ["dL_drgb", "dL_dnormal", "dL_df0", "dL_droughness", "dL_dopacity", "dL_dscale", "dL_dmean", "dL_drotation", "total_weight"]
_GRAD_CH = [3, 3, 3, 1, 1, 3, 3, 4, 1]
TARGET_KEYS = ["diffuse", "specular", "depth", "normal", "f0", "roughness"]
ACTIVATIONS = {"sigmoid": 0, "relu": 1, "clipped_relu": 2, "exp": 3}


def reference_dir():
    return os.environ.get("EGR_REFERENCE_DIR", "/root/reference")


def build(force=False):
    """Builds the library if the reference's sources are there. Returns its path, or None (one line printed) when they are not."""
    src = os.path.join(reference_dir(), "editable_gauss_refl", "cuda", "csrc", "shaders.cu")
    if not os.path.exists(src):
        print(f"oracle/_ref: no reference sources under {reference_dir()} (EGR_REFERENCE_DIR) - libegr_reference.so not built")
        return None
    cmd = ["make", "-C", _HERE, "EGR_REFERENCE_DIR=" + reference_dir(), "_ref/libegr_reference.so"]
    subprocess.check_call(cmd + (["-B"] if force else []), stdout=subprocess.DEVNULL)
    return _LIB_PATH


def available():
    """Whether the library was built (it is never built on import: build() of __graft_entry__ does that)."""
    return os.path.exists(_LIB_PATH)


def lib():
    global _lib
    if _lib is None:
        if not available():
            raise RuntimeError("oracle/_ref/libegr_reference.so is not built (needs the reference's sources: see oracle/Makefile)")
        L = ctypes.CDLL(_LIB_PATH)
        vp, ci, cf, u32 = ctypes.c_void_p, ctypes.c_int, ctypes.c_float, ctypes.c_uint32
        L.ref_create.restype = vp
        L.ref_create.argtypes = [ci, ci]
        L.ref_destroy.argtypes = [vp]
        L.ref_set_config.argtypes = [vp, vp]
        L.ref_set_camera.argtypes = [vp, vp, vp, cf, cf, cf]
        L.ref_set_gaussians.argtypes = [vp, ci] + [vp] * 8
        L.ref_set_targets.argtypes = [vp] + [vp] * 6
        L.ref_update_bvh.argtypes = [vp]
        L.ref_reset_accumulators.argtypes = [vp]
        L.ref_set_reverse_traversal.argtypes = [vp, ci]
        L.ref_get_total_num_calls.restype = u32
        L.ref_get_total_num_calls.argtypes = [vp]
        L.ref_set_total_num_calls.argtypes = [vp, u32]
        L.ref_get_accumulated_sample_count.restype = ci
        L.ref_get_accumulated_sample_count.argtypes = [vp]
        L.ref_gradients.argtypes = [vp, ci, vp]
        L.ref_raytrace.restype = ci
        L.ref_raytrace.argtypes = [vp, ci]
        L.ref_read_outputs.argtypes = [vp, vp, vp, vp, vp]
        L.ref_get_instances.argtypes = [vp, vp, vp, vp]
        L.ref_tea4.restype = u32
        L.ref_tea4.argtypes = [u32, u32]
        L.ref_lcg.restype = u32
        L.ref_lcg.argtypes = [vp]
        L.ref_rnd.restype = cf
        L.ref_rnd.argtypes = [vp]
        L.ref_primary_ray_direction.argtypes = [vp, cf, ci, ci, ci, ci, ci, vp, vp]
        L.ref_sample_cook_torrance.argtypes = [ci] + [vp] * 5
        L.ref_cook_torrance_weight.argtypes = [ci] + [vp] * 6
        L.ref_compute_scaling_factor.argtypes = [ci] + [vp] * 4
        L.ref_eval_gaussian.argtypes = [ci] + [vp] * 3
        L.ref_activation.argtypes = [ci, ci, vp, vp]
        L.ref_activation_backward.argtypes = [ci, ci, vp, vp, vp]
        L.ref_normalize_act.argtypes = [ci, vp, vp]
        L.ref_backward_normalize_act.argtypes = [ci, vp, vp, vp]
        _lib = L
    return _lib


def _f32(a, shape=None):
    a = np.ascontiguousarray(np.asarray(a, dtype=np.float32))
    return a if shape is None else a.reshape(shape)


def _ptr(a):
    return a.ctypes.data_as(ctypes.c_void_p) if a is not None else None


def _ptr_array(arrays):
    return (ctypes.c_void_p * len(arrays))(*[a.ctypes.data for a in arrays])


class Reference:
    """The reference's `Raytracer` (raytracer.cpp) on the CPU: set_gaussians = the eight copy_ of the caller's parameter export, update_bvh = its
    instance kernel, raytrace = one launch of its raygen program over every pixel. `reverse_traversal` visits the instances last to first."""

    def __init__(self, width, height, reverse_traversal=False):
        self.L = lib()
        self.W, self.H = int(width), int(height)
        self.h = self.L.ref_create(self.W, self.H)
        self.config = {k: v for k, v in CONFIG_FIELDS}
        self.n = 0
        self.L.ref_set_reverse_traversal(self.h, int(reverse_traversal))
        self.set_camera(np.zeros(3), np.eye(3), 1.0, 0.01, 999.9)
        self._push_config()

    def __del__(self):
        try:
            self.L.ref_destroy(self.h)
        except Exception:
            pass

    @property
    def total_num_calls(self):
        return int(self.L.ref_get_total_num_calls(self.h))

    @total_num_calls.setter
    def total_num_calls(self, v):
        self.L.ref_set_total_num_calls(self.h, int(v) & 0xFFFFFFFF)

    @property
    def accumulated_sample_count(self):
        return int(self.L.ref_get_accumulated_sample_count(self.h))

    def set_config(self, **kw):
        for k, v in kw.items():
            if k not in self.config:
                raise KeyError(k)
            self.config[k] = v
        self._push_config()

    def _push_config(self):
        c = np.ascontiguousarray([float(self.config[k]) for k, _ in CONFIG_FIELDS], dtype=np.float64)
        self.L.ref_set_config(self.h, _ptr(c))

    def set_camera(self, origin, c2w, fov, znear=0.01, zfar=999.9):
        self.L.ref_set_camera(self.h, _ptr(_f32(origin, (3,))), _ptr(_f32(c2w, (3, 3))), float(np.float32(fov)), float(np.float32(znear)), float(np.float32(zfar)))

    def set_gaussians(self, g):
        arrs = [_f32(g[k]).reshape(-1, c) for k, c in GAUSSIAN_FIELDS]
        n = arrs[0].shape[0]
        assert all(a.shape[0] == n for a in arrs)
        self.n = n
        self.L.ref_set_gaussians(self.h, n, *[_ptr(a) for a in arrs])

    def update_bvh(self):
        self.L.ref_update_bvh(self.h)

    def reset_accumulators(self):
        self.L.ref_reset_accumulators(self.h)

    def instances(self):
        """(M[n,3,4], Wm[n,3,4], visible[n]): the reference kernel's object-to-world rows, the driver's inverse of them, the visibility mask."""
        M, Wm, vis = np.zeros((self.n, 3, 4), np.float32), np.zeros((self.n, 3, 4), np.float32), np.zeros(self.n, np.int32)
        self.L.ref_get_instances(self.h, _ptr(M), _ptr(Wm), _ptr(vis))
        return M, Wm, vis

    def raytrace(self, grads_enabled=False, targets=None, grads_into=None):
        """One launch (total_num_calls is incremented first). Returns the framebuffer, random_seeds and the two stats as the launch left them - a grad
        launch writes no images, so its output_* are those of the launch before - and, with grads_enabled, the nine gradient tensors: summed onto
        `grads_into` (fp32 arrays by key) where given, onto zeros otherwise."""
        H, W, n = self.H, self.W, self.n
        tg = [None if not targets or targets.get(k) is None else _f32(targets[k]) for k in TARGET_KEYS]
        self.L.ref_set_targets(self.h, *[_ptr(a) for a in tg])
        grads = None
        if grads_enabled:
            grads = []
            for k, c in zip(GRAD_KEYS, _GRAD_CH):
                if grads_into is not None and k in grads_into:
                    assert grads_into[k].dtype == np.float32 and grads_into[k].flags.c_contiguous and grads_into[k].size == n * c
                    grads.append(grads_into[k])
                else:
                    grads.append(np.zeros((n, c), np.float32))
            self.L.ref_gradients(self.h, 1, _ptr_array(grads))
        if self.L.ref_raytrace(self.h, int(bool(grads_enabled))) != 0:
            raise MemoryError("reference driver: hit lists")
        out = {k: np.zeros((1 if k == "output_final" else NSTEPS, H, W, c), np.float32) for k, c in zip(OUT_KEYS, _OUT_CH)}
        out["random_seeds"] = np.zeros((H, W, 1), np.uint32)
        out["num_traversed"] = np.zeros((H, W), np.int32)
        out["num_accumulated"] = np.zeros((H, W), np.int32)
        self.L.ref_read_outputs(self.h, _ptr_array([out[k] for k in OUT_KEYS]), _ptr(out["random_seeds"]), _ptr(out["num_traversed"]), _ptr(out["num_accumulated"]))
        if grads_enabled:
            self.L.ref_gradients(self.h, 0, _ptr_array(grads))
            out.update(zip(GRAD_KEYS, grads))
        return out


# ---------------------------------------------------------------------------------------------- the reference's small functions
def tea4(a, b):
    return int(lib().ref_tea4(a & 0xFFFFFFFF, b & 0xFFFFFFFF))


def lcg_sequence(seed, count):
    st = ctypes.c_uint32(seed & 0xFFFFFFFF)
    return [int(lib().ref_lcg(ctypes.byref(st))) for _ in range(count)], int(st.value)


def rnd_sequence(seed, count):
    st = ctypes.c_uint32(seed & 0xFFFFFFFF)
    return [float(lib().ref_rnd(ctypes.byref(st))) for _ in range(count)], int(st.value)


def primary_ray_direction(c2w, fov, jitter, ix, iy, width, height, seed):
    """(direction[3] fp32, seed after the call) of Camera::compute_primary_ray_direction."""
    st, d = ctypes.c_uint32(seed & 0xFFFFFFFF), np.zeros(3, np.float32)
    lib().ref_primary_ray_direction(_ptr(_f32(c2w, (3, 3))), float(np.float32(fov)), int(jitter), int(ix), int(iy), int(width), int(height), ctypes.byref(st), _ptr(d))
    return d, int(st.value)


def sample_cook_torrance(N, V, roughness, u):
    N, V, r, u = _f32(N).reshape(-1, 3), _f32(V).reshape(-1, 3), _f32(roughness).reshape(-1), _f32(u).reshape(-1, 2)
    L = np.zeros_like(N)
    lib().ref_sample_cook_torrance(len(N), _ptr(N), _ptr(V), _ptr(r), _ptr(u), _ptr(L))
    return L


def cook_torrance_weight(N, V, L, roughness, f0):
    N, V, L, r, f0 = _f32(N).reshape(-1, 3), _f32(V).reshape(-1, 3), _f32(L).reshape(-1, 3), _f32(roughness).reshape(-1), _f32(f0).reshape(-1, 3)
    w = np.zeros_like(N)
    lib().ref_cook_torrance_weight(len(N), _ptr(N), _ptr(V), _ptr(L), _ptr(r), _ptr(f0), _ptr(w))
    return w


def compute_scaling_factor(opacity, alpha_threshold, exp_power):
    o, a, p = np.broadcast_arrays(_f32(opacity), _f32(alpha_threshold), _f32(exp_power))
    o, a, p = _f32(o).reshape(-1), _f32(a).reshape(-1), _f32(p).reshape(-1)
    out = np.zeros_like(o)
    lib().ref_compute_scaling_factor(len(o), _ptr(o), _ptr(a), _ptr(p), _ptr(out))
    return out


def eval_gaussian(local_hit, exp_power):
    x = _f32(local_hit).reshape(-1, 3)
    p = _f32(np.broadcast_to(_f32(exp_power), (len(x),)))
    out = np.zeros(len(x), np.float32)
    lib().ref_eval_gaussian(len(x), _ptr(x), _ptr(p), _ptr(out))
    return out


def activation(name, x):
    x = _f32(x).reshape(-1)
    y = np.zeros_like(x)
    lib().ref_activation(ACTIVATIONS[name], len(x), _ptr(x), _ptr(y))
    return y


def activation_backward(name, dL_dy, y):
    g, y = _f32(dL_dy).reshape(-1), _f32(y).reshape(-1)
    out = np.zeros_like(g)
    lib().ref_activation_backward(ACTIVATIONS[name], len(g), _ptr(g), _ptr(y), _ptr(out))
    return out


def normalize_act(x):
    x = _f32(x).reshape(-1, 4)
    y = np.zeros_like(x)
    lib().ref_normalize_act(len(x), _ptr(x), _ptr(y))
    return y


def backward_normalize_act(dL_dy, x):
    g, x = _f32(dL_dy).reshape(-1, 4), _f32(x).reshape(-1, 4)
    out = np.zeros_like(x)
    lib().ref_backward_normalize_act(len(x), _ptr(g), _ptr(x), _ptr(out))
    return out
