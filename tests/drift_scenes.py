"""Scenes whose Gaussians have drifted out of the BVH's build frame, shared by the CPU test of these inputs (test_drift_scenes.py, oracle only) and
the GPU tests of the refitted tree (test_hip_drifted_tree.py). Training refits the tree every iteration and rebuilds it only at pruning intervals:
in between the means move and the scales grow, and a box that leaves the 16-bit quantisation frame of the last rebuild is stored with sentinel
cells (0 decodes as -inf, 65535 as +inf; csrc/bvh.hip: quant_lo / quant_hi), which switches every forward launch to its sentinel code.
A plain numpy module: no fixtures, nothing is collected from here. `syn` is the package's synthetic module (the conftest fixture)."""
import numpy as np

W, H, N = 64, 48, 3000
SIDES = ("lo_x", "lo_y", "lo_z", "hi_x", "hi_y", "hi_z")
ALL_SIDES = frozenset(SIDES)
# the sentinel kinds every drift is meant to produce (test_drift_scenes.py holds the inputs to it: >= 100 boxes on each of these sides, none on the others)
EXPECTED_SIDES = {"dilate": ALL_SIDES, "two_walls": frozenset({"hi_x", "lo_z"}), "growth": ALL_SIDES,
                  "far_wall": ALL_SIDES - {"lo_x"}}  # (the +x wall times 12 spreads to both sides in y and z, and only outward in x)
KINDS = tuple(EXPECTED_SIDES)
WALLS = tuple((axis, sign) for axis in range(3) for sign in (+1, -1))


def wall_side(axis, sign):
    return ("hi_" if sign > 0 else "lo_") + "xyz"[axis]


def base_scene(syn, seed):
    return syn.make_scene(N, "trained", seed)


def _copy(g):
    return {k: v.copy() for k, v in g.items()}


def _on_wall(syn, g, axis, sign):
    """Rows of the wall at sign * ROOM_HALF[axis] (the walls' means lie exactly on their plane; the few sphere samples within 0.01 of it move along)."""
    return sign * g["mean"][:, axis] > syn.ROOM_HALF[axis] - 0.01


def drift(syn, g, kind):
    """A copy of the raw parameters `g` after the drift `kind` (EXPECTED_SIDES lists the sentinel kinds each one produces)."""
    d = _copy(g)
    f32 = np.float32
    if kind == "dilate":  # the whole room 1.4 times as large: all six sides, the spheres stay inside the frame
        d["mean"] *= f32(1.4)
        d["scale"] += f32(np.log(1.4))
    elif kind == "two_walls":  # two walls move outward, nothing else: two sentinel kinds
        d["mean"][_on_wall(syn, g, 0, +1), 0] += f32(1.0)
        d["mean"][_on_wall(syn, g, 2, -1), 2] -= f32(0.7)
    elif kind == "growth":  # the means stay, every fifth box grows across the frame's border
        d["scale"][::5] += f32(np.log(4.0))
    elif kind == "far_wall":  # coordinates ten times the frame
        w = _on_wall(syn, g, 0, +1)
        d["mean"][w] *= f32(12.0)
        d["scale"][w] += f32(np.log(12.0))
    else:
        raise KeyError(kind)
    return d


def wall(syn, g, axis, sign):
    """One wall moves outward by 1.0: exactly one sentinel kind, wall_side(axis, sign)."""
    d = _copy(g)
    d["mean"][_on_wall(syn, g, axis, sign), axis] += np.float32(sign * 1.0)
    return d


def walk(g, steps, rng):
    """The stand-in for training between two rebuilds: `steps` increments of mean += N(0, 0.03), scale += N(0, 0.05); one state after the other."""
    d = _copy(g)
    states = []
    for _ in range(steps):
        d["mean"] = (d["mean"] + rng.normal(0.0, 0.03, d["mean"].shape)).astype(np.float32)
        d["scale"] = (d["scale"] + rng.normal(0.0, 0.05, d["scale"].shape)).astype(np.float32)
        states.append(_copy(d))
    return states


def oblique_camera(syn, axis, sign):
    """Sees the wall that wall(axis, sign) moves at an angle, never head-on: a ray that leaves the frame straight through a box's truncated face
    still finds the box when a sentinel is decoded as a plain cell; an oblique ray does not."""
    eye = np.array([0.3, -0.2, 0.1])
    target = np.zeros(3)
    target[axis] = sign * syn.ROOM_HALF[axis]
    target[(axis + 1) % 3] = eye[(axis + 1) % 3] + 1.5
    target[(axis + 2) % 3] = eye[(axis + 2) % 3] + 0.4
    return dict(origin=eye.astype(np.float32), c2w=syn.look_at(eye, target).astype(np.float32), fov=np.float32(0.9), znear=np.float32(0.01),
                zfar=np.float32(999.9))


def out_of_frame_mask(aabb, frame):
    """(mask [N], {side: count}) of the usable boxes (lo <= hi) of aabb [N,6] that the refit stores with a sentinel cell in the frame
    (origin xyz, cells per world unit xyz): (lo - o) * s + 2 < 2 or (hi - o) * s + 2 > 65533 on any axis, in fp32 as quant_lo / quant_hi."""
    a = np.asarray(aabb, np.float32)
    fr = np.asarray(frame, np.float32)
    o, s = fr[:3], fr[3:]
    usable = a[:, 0] <= a[:, 3]
    with np.errstate(invalid="ignore", over="ignore"):
        low = ((a[:, :3] - o) * s + np.float32(2.0) < np.float32(2.0)) & usable[:, None]
        high = ((a[:, 3:] - o) * s + np.float32(2.0) > np.float32(65533.0)) & usable[:, None]
    sides = np.concatenate([low, high], axis=1)  # [N,6] in the order of SIDES
    return sides.any(axis=1), {k: int(sides[:, i].sum()) for i, k in enumerate(SIDES)}


def ellipsoid_boxes(o):
    """[N,6] boxes of an oracle's snapshot as the tree bounds them: the ellipsoid's half-extent along axis a is |row a of M|_2 (the tree pads
    them by a part in a thousand); an invisible Gaussian gets an empty box (lo > hi)."""
    M, _, _, vis = o.instances()
    ext = np.sqrt((M[:, :, :3] ** 2).sum(-1))
    ctr = M[:, :, 3]
    box = np.concatenate([ctr - ext, ctr + ext], axis=1)
    box[vis == 0] = np.array([1.0, 1.0, 1.0, -1.0, -1.0, -1.0])
    return box.astype(np.float32)


def frame_restated(aabb):
    """egr_bvh_rebuild's rule restated for the CPU test (the GPU tests read the real frame: Raytracer.debug_bvh_state): the bounds of the usable
    boxes, widened by 5 % of the extent (at least 1e-6) on both sides, mapped onto 65530 cells. Returns (origin xyz, cells per world unit xyz)."""
    a = np.asarray(aabb, np.float32)
    u = a[a[:, 0] <= a[:, 3]]
    lo, hi = (u[:, :3].min(0), u[:, 3:].max(0)) if len(u) else (np.zeros(3, np.float32), np.ones(3, np.float32))
    ext = np.maximum(hi - lo, np.float32(1e-6))
    lo, hi = lo - np.float32(0.05) * ext, hi + np.float32(0.05) * ext
    return np.concatenate([lo, np.float32(65530.0) / (hi - lo)]).astype(np.float32)


def hidden(g, mask):
    """A copy of `g` with the rows of `mask` made invisible (sigmoid(-8) is below the alpha threshold)."""
    d = _copy(g)
    d["opacity"][mask] = np.float32(-8.0)
    return d


def changed_share(a, b, step):
    """Share of the pixels whose output_rgb of `step` differs by more than 1e-3 between two launches."""
    return float((np.abs(a["output_rgb"][step] - b["output_rgb"][step]).max(-1) > 1e-3).mean())
