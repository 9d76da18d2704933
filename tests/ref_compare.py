"""The comparison rule between the reference's shader code run on the CPU (oracle/reference.py, or a fixture it wrote) and the CPU oracle, shared by
tests/test_oracle_vs_reference.py and tests/test_reference_fixture.py. A plain module: no fixtures, nothing is collected from here.

Integers (random_seeds, num_accumulated, num_traversed) are compared exactly, at every pixel of every case. Floats are compared three ways with the fp64 oracle: per tensor
    max|ref - o64| <= FACTOR * max|o32 - o64| + FLOOR * max|o64|
- reference and fp32 oracle are two fp32 evaluations of the same formulas in another operation order, so each is as far from the fp64 evaluation as
fp32 rounding puts it on that scene; 8 leaves room for the order, a wrong formula shows at 1e-3 of the tensor or more."""
import numpy as np

FACTOR = 8.0
FLOOR = 1e-6
OUT_KEYS = ["output_rgb", "output_depth", "output_normal", "output_f0", "output_roughness", "output_transmittance", "output_total_transmittance",
            "output_ray_origin", "output_ray_direction", "output_final"]
GRAD_KEYS = ["dL_drgb", "dL_dnormal", "dL_df0", "dL_droughness", "dL_dopacity", "dL_dscale", "dL_dmean", "dL_drotation", "total_weight"]


def report(name, **kv):
    print("REPORT " + name + ": " + ", ".join(f"{k}={v}" for k, v in kv.items()), flush=True)


def three_way(ref, o32, o64, keys):
    """Per key: (passes, max|ref - o64|, max|o32 - o64|, max|o64|, ratio), ratio = (max|ref - o64| - FLOOR max|o64|) / max|o32 - o64| (<= FACTOR passes;
    inf when the fp32 oracle is exact and the reference is off the floor). Non-finite elements must be the same in the reference and the fp32 oracle -
    NaN at the same places, the same infinity at the same places - and are left out of the maxima."""
    res = {}
    for k in keys:
        r, a, b = (np.asarray(x[k], np.float64) for x in (ref, o32, o64))
        a, b = a.reshape(r.shape), b.reshape(r.shape)
        odd = ~np.isfinite(r) | ~np.isfinite(a)
        if not (np.array_equal(np.isnan(r), np.isnan(a)) and np.array_equal(r[odd & ~np.isnan(r)], a[odd & ~np.isnan(a)])):
            res[k] = (False, float("nan"), float("nan"), float("nan"), float("inf"))
            continue
        ok = ~odd & np.isfinite(b)
        if not ok.any():
            res[k] = (True, 0.0, 0.0, 0.0, 0.0)
            continue
        e_ref, e_32, scale = float(np.abs(r - b)[ok].max()), float(np.abs(a - b)[ok].max()), float(np.abs(b)[ok].max())
        excess = max(e_ref - FLOOR * scale, 0.0)
        ratio = 0.0 if excess == 0.0 else (excess / e_32 if e_32 > 0 else float("inf"))
        res[k] = (ratio <= FACTOR, e_ref, e_32, scale, ratio)
    return res


def failing(res):
    return {k: tuple(f"{x:.3g}" for x in v[1:]) for k, v in res.items() if not v[0]}


def worst_ratio(res):
    return max([v[4] for v in res.values()] + [0.0])


def could_be_left_out(o32):
    """The pixels the comparison rule would allow to leave out if a case needed it (none does: a failing case lists them in its message): those the
    fp32 oracle flags - two composited hits within 4 ulps of each other, or within 1e-5 on a bounce step, whose order the last bits of t decide."""
    why = {"depth_tie": np.asarray(o32["num_depth_ties"]) > 0, "bounce_near_tie": np.asarray(o32["num_bounce_near_ties"]) > 0}
    ys, xs = np.nonzero(why["depth_tie"] | why["bounce_near_tie"])
    return [(int(x), int(y), "+".join(k for k in why if why[k][y, x])) for y, x in zip(ys, xs)]


def assert_integers(ref, o32, name):
    """random_seeds, num_traversed and num_accumulated equal at every pixel."""
    assert np.array_equal(np.asarray(ref["random_seeds"]).reshape(-1), np.asarray(o32["random_seeds"]).reshape(-1)), (name, "random_seeds")
    for k in ("num_traversed", "num_accumulated"):
        r, a = np.asarray(ref[k]).reshape(-1), np.asarray(o32[k]).reshape(-1)
        bad = np.flatnonzero(r != a)
        assert bad.size == 0, (name, k, [(int(i), int(r[i]), int(a[i])) for i in bad[:8]], int(bad.size))
