"""TEST INFRASTRUCTURE ONLY: a shadow trainer in plain numpy - what surrounds the render in one iteration of the reference's loop (train.py:217-260,
scene/gaussian_model.py), restated on host arrays in the project's words; fp64 wherever arithmetic happens, fp32 wherever a value is stored. It holds

  the eight raw parameter groups in trainer.GROUPS' order, both Adam moments of each, ONE step count, the model-side and the raytracer-side gradients,
  total_weight and the caller's per-row extras,

and restates

  update_learning_rate   trainer.expon_lr for xyz (read out of trainer.py without importing it: that module loads the native library)
  step                   g = model-side + raytracer-side gradient (one fp32 add), scale decay, the Adam update and the three clamps through
                         aux_restatement.scale_decay64 / adam_moments64 / adam_update64, both gradients zeroed, the count advanced; total_weight stays
  prune_mask / prune     fp32(total_weight) / fp32(interval) < fp32(min_weight), strict; |xyz - c| < znear in fp64 for any camera; an explicit mask taken as
                         given; compaction = boolean indexing of parameters, moments and extras; gradients and total_weight zero at the new length
  grow                   rows appended, their moments, gradients and total_weight zero, the old rows' kept; extras extended by their fill value
  reset_state            both moments of one group zero, the count untouched

It takes gradients as arguments and contains no tracer. tests/test_schedule_restatement_host.py holds it to torch.optim.Adam with the reference's optimizer
surgery; tests/test_hip_schedule.py holds the product to it, one hand-over at a time (`adopt`). The second half of the file is the one schedule both modules
drive: its sizes, rates and events, and the host-side recipes for its inputs."""
import ast
import math
import os

import numpy as np

import aux_restatement as ar
import grow_restatement as gr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = "editable-gaussian-reflections_amd"
F32, F64 = np.float32, np.float64


def trainer_definitions():
    """(GROUPS, CLAMPS, expon_lr) as trainer.py states them, evaluated from its source: the module itself loads the GPU library on import."""
    tree = ast.parse(open(os.path.join(ROOT, PKG, "trainer.py")).read())
    wanted = [n for n in tree.body if (isinstance(n, ast.FunctionDef) and n.name == "expon_lr")
              or (isinstance(n, ast.Assign) and getattr(n.targets[0], "id", None) in ("GROUPS", "CLAMPS"))]
    ns = {"np": np, "math": math}
    exec(compile(ast.Module(wanted, []), "trainer.py", "exec"), ns)
    return ns["GROUPS"], ns["CLAMPS"], ns["expon_lr"]


GROUPS, CLAMPS, expon_lr = trainer_definitions()
NAMES = tuple(name for name, _, _ in GROUPS)
RT_NAME = {name: rt for name, _, rt in GROUPS}  # the raytracer's (and synthetic.make_scene's, and the oracle's) name of a group
ATTR = {name: attr for name, attr, _ in GROUPS}


def grad_key(name):
    """The native gradient tensor of a group (hip_common.GRAD_KEYS, the oracle's outputs)."""
    return "dL_d" + RT_NAME[name]


def sphere_distances(xyz, centers):
    """[N, C] fp64 distances of fp32 points from fp32 camera centres."""
    d = np.asarray(xyz, F64)[:, None, :] - np.asarray(centers, F64).reshape(-1, 3)[None]
    return np.sqrt((d * d).sum(axis=2))


def near_cameras(xyz, centers, znear):
    """scene.select_points_to_prune_near_cameras restated: inside ANY camera's znear sphere, in fp64. Returns (mask [N], the smallest | dist - znear | / znear)."""
    z = np.broadcast_to(np.asarray(znear, F64).reshape(-1), (np.asarray(centers).reshape(-1, 3).shape[0],))
    dist = sphere_distances(xyz, centers)
    with np.errstate(divide="ignore", invalid="ignore"):
        margin = np.where(z[None] > 0, np.abs(dist - z[None]) / z[None], np.inf)
    return np.any(dist < z[None], axis=1), float(margin.min()) if margin.size else math.inf


class ShadowTrainer:
    def __init__(self, params, lrs, xyz_schedule=None, beta1=0.9, beta2=0.999, eps=1e-15, scale_decay=1.0, extras=()):
        """params: group name -> [N, width] array (copied, stored as fp32). extras: per-row arrays of the caller's model."""
        self.p = {n: np.array(params[n], F32) for n in NAMES}
        self.m = {n: np.zeros_like(self.p[n]) for n in NAMES}
        self.v = {n: np.zeros_like(self.p[n]) for n in NAMES}
        self.g = {n: np.zeros_like(self.p[n]) for n in NAMES}  # model side (.grad of the raw parameters)
        self.rg = {n: np.zeros_like(self.p[n]) for n in NAMES}  # raytracer side (the native holder's gradients)
        self.total_weight = np.zeros((self.n, 1), F32)
        self.extras = [np.array(e) for e in extras]
        self.lrs = {n: float(lrs.get(n, 0.0)) for n in NAMES}
        self.xyz_schedule, self.beta1, self.beta2, self.eps, self.scale_decay = xyz_schedule, beta1, beta2, eps, scale_decay
        self.steps = 0

    @property
    def n(self):
        return self.p[NAMES[0]].shape[0]

    def update_learning_rate(self, iteration):
        if self.xyz_schedule is not None:
            self.lrs["xyz"] = expon_lr(iteration, **self.xyz_schedule)
        return self.lrs["xyz"]

    def receive(self, rt_grads, total_weight):
        """One launch's raytracer-side gradients (group name -> array) and weights are ADDED to what is held: nothing but `step` and `prune` clears them."""
        for n in NAMES:  # (the sum of two fp32 values formed in fp64 and rounded once IS their fp32 sum)
            self.rg[n] = (self.rg[n].astype(F64) + np.asarray(rt_grads[n], F32).astype(F64)).astype(F32)
        self.total_weight = (self.total_weight.astype(F64) + np.asarray(total_weight, F32).astype(F64).reshape(-1, 1)).astype(F32)

    def step(self):
        t = self.steps + 1
        for n in NAMES:
            g32 = self.g[n] + self.rg[n]  # the import: one fp32 add
            assert g32.dtype == F32
            p = self.p[n].astype(F64)
            if n == "scaling" and self.scale_decay != 1.0:
                p = ar.scale_decay64(p, F32(self.scale_decay))
            m, v = ar.adam_moments64(self.m[n], self.v[n], g32, self.beta1, self.beta2)
            self.m[n], self.v[n] = m.astype(F32), v.astype(F32)
            lo, hi = CLAMPS.get(n, (-math.inf, math.inf))
            self.p[n] = np.clip(p - ar.adam_update64(self.m[n], self.v[n], self.lrs[n], t, self.beta1, self.beta2, self.eps), lo, hi).astype(F32)
            self.g[n], self.rg[n] = np.zeros_like(self.p[n]), np.zeros_like(self.p[n])
        self.steps = t

    def prune_mask(self, min_weight=0.0, interval=1, cam_centers=None, cam_znear=None, remove_mask=None):
        """(rows to REMOVE [N] bool, margins): margins["weight"] = the smallest | q - min_weight | / min_weight over the rows (inf for min_weight 0),
        margins["sphere"] = the smallest | dist - znear | / znear over rows and cameras (inf without cameras)."""
        with np.errstate(divide="ignore", invalid="ignore"):
            q = self.total_weight.reshape(-1).astype(F32) / F32(interval)
            assert q.dtype == F32
            remove = q < F32(min_weight)
            margins = dict(weight=float(np.abs(q.astype(F64) - F64(F32(min_weight))).min() / F64(F32(min_weight))) if min_weight > 0 else math.inf, sphere=math.inf)
        if cam_centers is not None:
            inside, margins["sphere"] = near_cameras(self.p["xyz"], cam_centers, cam_znear)
            remove = remove | inside
        if remove_mask is not None:
            remove = remove | (np.asarray(remove_mask).reshape(-1) != 0)
        return remove, margins

    def prune(self, remove):
        keep = ~np.asarray(remove, bool)
        assert keep.shape == (self.n,) and keep.any()
        for n in NAMES:
            self.p[n], self.m[n], self.v[n] = self.p[n][keep], self.m[n][keep], self.v[n][keep]
            self.g[n], self.rg[n] = np.zeros_like(self.p[n]), np.zeros_like(self.p[n])  # the iteration's gradients are dropped on both sides
        self.extras = [e[keep] for e in self.extras]
        self.total_weight = np.zeros((self.n, 1), F32)  # ... and the weights restart

    def grow(self, new, extra_fills=()):
        """new: group name -> [M, width] rows. The old rows keep everything, mid-interval: total_weight is not cleared."""
        m_rows = np.asarray(new[NAMES[0]]).reshape(-1, 3).shape[0]
        assert m_rows > 0 and len(extra_fills) == len(self.extras)
        for n in NAMES:
            add = np.asarray(new[n], F32).reshape(m_rows, self.p[n].shape[1])
            zeros = np.zeros_like(add)
            self.p[n] = np.concatenate([self.p[n], add])
            for held in (self.m, self.v, self.g, self.rg):
                held[n] = np.concatenate([held[n], zeros])
        self.total_weight = np.concatenate([self.total_weight, np.zeros((m_rows, 1), F32)])
        self.extras = [np.concatenate([e, np.full((m_rows,) + e.shape[1:], fill, e.dtype)]) for e, fill in zip(self.extras, extra_fills)]

    def reset_state(self, name):
        self.m[name], self.v[name] = np.zeros_like(self.p[name]), np.zeros_like(self.p[name])

    def adopt(self, p=None, m=None, v=None, g=None, rg=None, total_weight=None, extras=None):
        """Teacher forcing: the held fp32 state takes the other side's bits (dicts by group name; shapes must already agree)."""
        for mine, theirs in ((self.p, p), (self.m, m), (self.v, v), (self.g, g), (self.rg, rg)):
            if theirs is not None:
                for n in NAMES:
                    a = np.array(theirs[n], F32)
                    assert a.shape == mine[n].shape, (n, a.shape, mine[n].shape)
                    mine[n] = a
        if total_weight is not None:
            a = np.array(total_weight, F32).reshape(-1, 1)
            assert a.shape == self.total_weight.shape
            self.total_weight = a
        if extras is not None:
            assert len(extras) == len(self.extras) and all(np.asarray(a).shape == b.shape for a, b in zip(extras, self.extras))
            self.extras = [np.array(a) for a in extras]


# ---- the schedule of tests/test_schedule_restatement_host.py (where its inputs are shown to be comfortable) and tests/test_hip_schedule.py ----
#
# Sizes: the smallest at which every mechanism is live. T iterations; batches of V views from the upstream sampler; iteration SINGLE_VIEW_ITERATION renders the first
# view of its batch alone through the single-view path; odd iterations add a model-side opacity gradient; bounces come on, and the far field is added, after the
# step of iteration GROW_ITERATION; iteration PRUNE_ITERATION prunes between the render and the step; iteration RESET_ITERATION starts with an opacity reset.
W, H, N, NUM_VIEWS, V, T = 48, 32, 800, 4, 2, 10
SCENE_SEED, PERTURB_SEED, PERTURB_SIGMA, SAMPLER_SEED = 7, 1, 2e-3, 11
LRS = dict(xyz=1.6e-4, normal=2e-3, roughness=2e-3, f0=2e-3, f_dc=1e-2, opacity=2.5e-2, scaling=5e-3, rotation=1e-3)  # test_training_loop.py's
XYZ_SCHEDULE = dict(lr_init=1.6e-4, lr_final=1.6e-6, lr_delay_steps=20, lr_delay_mult=0.01, max_steps=30000)  # inside the warm-up: another rate at every iteration
SCALE_DECAY = 0.999
# The model's roughness at the start. The reference samples the bounce direction in fp32 (the shaders' arithmetic, which the fp32 oracle restates), and what that costs
# depends on the roughness: against the same function in fp64 the sampled direction is off by 1.4e-4 at roughness 0.01 and 0.02 (median over 20,000 random normals,
# views and uniforms), 4.5e-6 at 0.1, 1.7e-7 at 0.5. With the true scene's roughness (0.1 on the walls, 0.02 on the spheres) the two oracles then disagree on which
# candidates 20 to 45 of the 1536 bounce rays of a launch composite, and their gradients differ by 2e-3 to 3e-3 of a tensor's max-abs at every iteration with bounces
# (measured on this schedule; 5e-3 on the scene of test_batch_gradients_against_the_oracle). At 0.7 they agree to 6e-6 at every iteration, which is what the host
# module asserts (3e-4). The targets keep the true roughness, so the roughness gradient is live.
START_ROUGHNESS = 0.7
SINGLE_VIEW_ITERATION, GROW_ITERATION, PRUNE_ITERATION, RESET_ITERATION = 5, 3, 7, 9
FARFIELD = dict(num_points=64, radius=1.0, seed=750)
EXTRA_FILL = -5  # the int32 per-row extra: 7 * row - 3 for the first rows, this for grown ones
PRUNE_INTERVAL = 4 * V
MIN_WEIGHT = 0.0207  # inside a 17 % gap of the sorted total_weight / interval of the oracle-driven trajectory (0.0188 .. 0.0227), near its 7 % quantile
REMOVE_EVERY, REMOVE_PHASE = 7, 3  # the explicit mask of the remove_mask-alone run: rows with row % 7 == 3
RESET_OPACITY_CEILING = -0.5  # the reset replaces opacity by min(opacity, this) (exact in any precision)
FIRST_CALL = 0  # total_num_calls of a new tracer


def sampler(num_views, seed, views_per_step):
    """Upstream's viewpoint stack (train.py:218-220) restated: pop(randint(0, len - 1)) from a stack that is refilled when empty, `views_per_step` draws per batch."""
    import random

    rng, stack = random.Random(seed), []
    while True:
        batch = []
        for _ in range(views_per_step):
            if not stack:
                stack = list(range(num_views))
            batch.append(stack.pop(rng.randint(0, len(stack) - 1)))
        yield batch


def bounces_at(iteration):
    return 0 if iteration <= GROW_ITERATION else 2


def model_side_gradient(iteration, n):
    """The model-side opacity gradient of an odd iteration ([n,1] fp32), None on even ones."""
    if iteration % 2 == 0:
        return None
    return (np.random.default_rng(1000 + iteration).normal(size=(n, 1)) * 1e-3).astype(F32)


def extra_rows(n):
    return (np.arange(n, dtype=np.int32).reshape(n, 1) * 7 - 3).astype(np.int32)


def explicit_remove_mask(n):
    return np.arange(n) % REMOVE_EVERY == REMOVE_PHASE


def start_model(truth, dist2):
    """test_training_loop.py's start: the truth's points moved by 2e-3, scales from the mean squared distance to the three nearest neighbours (`dist2` [N]: distCUDA2
    on the GPU, its brute-force checker on the CPU), grey colour, opacity 0. One deviation: every row keeps the truth's own anisotropy (its three log-scales minus their
    mean) on top of the kNN size. With three EQUAL scales the rotation gradient is zero in exact arithmetic, what either side computes for it is rounding noise, and no
    bar relative to the tensor's max-abs can hold. One addition: roughness starts at START_ROUGHNESS everywhere (see there)."""
    g = {k: np.array(v, F32) for k, v in truth.items()}
    d2 = np.maximum(np.asarray(dist2, F32).reshape(-1), F32(1e-7))
    shape = g["scale"] - g["scale"].mean(axis=1, keepdims=True, dtype=F32)
    g["scale"] = (np.log(np.sqrt(d2))[:, None] + shape).astype(F32)
    g["rgb"] = np.full_like(g["rgb"], 0.5)
    g["opacity"] = np.zeros_like(g["opacity"])
    g["roughness"] = np.full_like(g["roughness"], START_ROUGHNESS)
    g["mean"] = g["mean"] + np.random.default_rng(PERTURB_SEED).normal(scale=PERTURB_SIGMA, size=g["mean"].shape).astype(F32)
    return g


def by_group(g):
    """A scene dict under the raytracer's names -> group name -> array."""
    return {n: g[RT_NAME[n]] for n in NAMES}


def by_rt_name(p):
    return {RT_NAME[n]: p[n] for n in NAMES}


def stored_pose(R, T):
    """What dataset.ViewSet keeps of a dataset pose and what the launch makes of it: (R fp32, centre = fp32(-R T in fp64), the blender c2w = -R with column 0
    negated again) - the camera the oracle needs."""
    R64, T64 = np.asarray(R, F64), np.asarray(T, F64)
    R32 = R64.astype(F32)
    c2w = -R32.copy()
    c2w[:, 0] = -c2w[:, 0]
    return R32, (-R64 @ T64).astype(F32), c2w


def farfield_rows(points, dist2, init_scale=0.1, init_opa=0.1, init_diffuse=0.2, init_f0=0.04):
    """The eight raw tensors add_farfield_points makes of the surviving candidates (config.py:43-50), by group name; `dist2` as in start_model."""
    k = points.shape[0]
    const = lambda value, width: np.full((k, width), value, F32)
    spacing = np.sqrt(np.maximum(np.asarray(dist2, F32).reshape(-1), F32(1e-7)))
    p = F32(init_opa)
    rotation = const(0.0, 4)
    rotation[:, 0] = 1.0
    return dict(xyz=np.asarray(points, F32), normal=const(0.0, 3), roughness=const(0.0, 1), f0=const(init_f0, 3), f_dc=const(init_diffuse, 3),
                opacity=np.full((k, 1), np.log(p / (F32(1.0) - p)), F32), scaling=np.repeat(np.log(spacing * F32(init_scale))[:, None], 3, axis=1).astype(F32), rotation=rotation)


def farfield_survivors(centers, znear):
    """(the candidates of FARFIELD outside every camera sphere [K,3], how many were dropped, the smallest relative distance of a candidate from a sphere's surface)."""
    cand = gr.candidates(0, FARFIELD["num_points"], FARFIELD["seed"], FARFIELD["radius"])
    inside, margin = near_cameras(cand, centers, znear)
    return cand[~inside], int(inside.sum()), margin
