"""Shared helpers of the GPU parity tests (HIP path through torch.classes.raytracer -> libraytracer.so -> C ABI vs the CPU oracle)."""
import importlib
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

PKG = "editable-gaussian-reflections_amd"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
OUT_KEYS = ["output_rgb", "output_depth", "output_normal", "output_f0", "output_roughness", "output_transmittance",
            "output_total_transmittance", "output_ray_origin", "output_ray_direction", "output_final"]
GRAD_KEYS = ["dL_drgb", "dL_dnormal", "dL_df0", "dL_droughness", "dL_dopacity", "dL_dscale", "dL_dmean", "dL_drotation", "total_weight"]

# The suite pins team help OFF at creation (conftest.py: many tests assert bit equality between two launches), but the kernels the product ships and bench.py
# times are the TEAM builds (k_forward_chain<.., 16>, k_backward_chain<4>: egr_set_team_help(1), the library default). Every test that compares with the ORACLE
# with a tolerance runs twice: help off (single-wave workgroups) and the product default (teams; help across the CU's waves and, round 6, across the GPU).
BOTH_HELP_MODES = pytest.mark.parametrize("team_help", [False, True], ids=["help_off", "product_default_help_on"])


@pytest.fixture(scope="module")
def ren():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU fallback")
    return importlib.import_module(PKG + ".renderer")


def views(syn, n, step=0.15):
    """n cameras inside the synthetic room: the default one, then moved and turned a little, with other fields of view."""
    base = syn.default_camera()
    cams = []
    for i in range(n):
        eye = base["origin"].astype(np.float64) + np.array([step * i, -step * 2 / 3 * i, step / 3 * i])
        cams.append(dict(origin=eye.astype(np.float32), c2w=syn.look_at(eye, (1.2 - 0.2 * i, 0.5 + 0.1 * i, -0.9)).astype(np.float32),
                         fov=np.float32(0.6911 + 0.07 * i), znear=np.float32(0.01), zfar=np.float32(999.9)))
    return cams


def tracer(ren, syn, W=64, H=48, N=3000, seed=5, variant="trained", fwd=8_000_000, bwd=1_000_000, **kw):
    """A tracer on a synthetic scene of the batch tests' size (the default hit arena is a no-grad render's: grad tests pass their own `bwd`)."""
    g = syn.make_scene(N, variant, seed=seed)
    return ren.GaussianRaytracer(ren.GaussianParams(g), W, H, ppll_forward_size=fwd, ppll_backward_size=bwd, **kw)


def psnr(a, b):
    mse = float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2))
    return 150.0 if mse == 0 else 10.0 * np.log10(1.0 / mse)


def make_pair(ren, orc, g, cam, W, H, cfg=None, fwd=8_000_000, bwd=8_000_000, **kw):
    """Returns (GaussianRaytracer, Oracle) fed the same scene / camera / config."""
    pc = ren.GaussianParams(g)
    rt = ren.GaussianRaytracer(pc, W, H, ppll_forward_size=fwd, ppll_backward_size=bwd, **kw)
    o = orc.Oracle(W, H)
    o.set_camera(cam["origin"], cam["c2w"], cam["fov"], cam.get("znear", 0.01), cam.get("zfar", 999.9))
    o.set_gaussians(g)
    c = dict(loss_weight_diffuse=5.0, loss_weight_specular=3.0, loss_weight_normal=2.5, loss_weight_depth=2.5, loss_weight_f0=1.0,
             loss_weight_roughness=1.0)
    c.update(cfg or {})
    o.set_config(**c)
    mc = rt.cuda_module.get_config()
    for k, v in (cfg or {}).items():
        getattr(mc, k).fill_(v)
    o.update_bvh()
    return rt, o


def cam_obj(ren, cam, targets=None):
    images = {}
    if targets:
        images = {k + "_image": torch.tensor(v).cuda().moveaxis(-1, 0).contiguous() for k, v in targets.items()}
    return ren.camera_from_c2w(cam["origin"], cam["c2w"], cam["fov"], **images)


def hip_outputs(rt):
    fb = rt.cuda_module.get_framebuffer()
    return {k: getattr(fb, k).cpu().numpy() for k in OUT_KEYS}


def hip_grads(rt):
    g = rt.cuda_module.get_gaussians()
    return {k: getattr(g, k).cpu().numpy() for k in GRAD_KEYS}


def run_grad(ren, rt, camera):
    rt.zero_grad()
    rt.cuda_module.get_gaussians().total_weight.zero_()
    ren.render(camera, rt)
    torch.cuda.synchronize()


def report(name, **kv):
    """Measured levels go to stdout (pytest -s / the captured log) so that the asserted bars can be kept at what is achieved."""
    print("REPORT " + name + ": " + ", ".join(f"{k}={v}" for k, v in kv.items()), flush=True)


def mismatch_list(a, b, limit=12):
    idx = np.flatnonzero(np.asarray(a).reshape(-1) != np.asarray(b).reshape(-1))
    return [(int(i), int(np.asarray(a).reshape(-1)[i]), int(np.asarray(b).reshape(-1)[i])) for i in idx[:limit]], int(idx.size)




def generic_targets(syn, W, H):
    """syn.make_targets with roughness / f0 moved off the scene's own wall values (0.1 / 0.04): where a fully opaque wall renders
    exactly its target, sign(output - target) is decided by the last bit of rounding, i.e. by noise in BOTH implementations."""
    tg = syn.make_targets(W, H)
    tg["roughness"] = tg["roughness"] + np.float32(0.23)
    tg["f0"] = tg["f0"] + np.float32(0.17)
    return tg


def grads_vs_oracle_listing_flipped_pixels(ren, rt, o, camera, tg, W, H, name, max_flipped=8, bar=1e-3, loose=5e-3):
    """The north-star gradient bar (max-rel-err < 1e-3 of each tensor's max-abs) with a SHOWN reason for anything above it.

    A bounce ray that differs by an ulp between the two implementations can meet one grazing candidate (alpha = alpha_threshold at
    the clip sphere) more or less; on a small image one such hit is 1-2e-3 of a tensor's maximum. Instead of loosening the bar:
      1. one grad launch on both sides -> nine gradient tensors; if all are < bar, done;
      2. otherwise LIST the pixels whose rays differ: composited hits per bounce step (HIP: egr_debug_get_step_hits, oracle:
         num_hits[step]), total transmittance of a step (a flipped candidate behind the last composited hit only shows there), or two
         consecutive composited hits within 4 ulps of each other in the oracle (their ORDER - hence their two weights - is decided by
         the last bits of t, where this build contracts fmas and the oracle does not; exact ties: by the list order, which is
         unspecified upstream);
      3. assert there are at most `max_flipped` of them, take exactly those PIXELS out ON BOTH SIDES (pixel masks: egr_debug_set_pixel_mask /
         Oracle.set_pixel_mask - the same whole-image launch otherwise) and assert < bar on everything else.
    Whatever is listed, NO tensor may be further than `loose` (5e-3) from the oracle on all pixels.
    Returns (per-tensor errors over all pixels, per-tensor errors without the listed pixels, listed pixels)."""
    m = rt.cuda_module
    run_grad(ren, rt, camera)
    k = int(m.get_metadata().total_num_calls)
    o.total_num_calls = k - 1
    ref = o.raytrace(True, targets=tg)
    gr = hip_grads(rt)
    live = [key for key in GRAD_KEYS if np.abs(ref[key]).max() > 0]
    err_all = {key: float(np.abs(gr[key] - ref[key]).max() / np.abs(ref[key]).max()) for key in live}
    for key in GRAD_KEYS:  # a tensor the configuration switches off stays exactly zero on both sides
        if key not in live:
            assert float(np.abs(gr[key]).max()) == 0.0, key
    worst_all = max(err_all.values())
    assert worst_all < loose, (name, err_all)  # unconditional: a listing never excuses more than this
    if worst_all < bar:
        report(name, worst_grad=f"{worst_all:.1e}", flipped_pixels=0)
        return err_all, err_all, []
    hits_h = m.debug_step_hits().numpy()  # [3,H,W], this grad launch
    hits_o = ref["num_composited_per_step"]
    m.get_metadata().total_num_calls.fill_(k - 1)  # the same rays once more, as images
    with torch.no_grad():
        rt(camera)
    o.total_num_calls = k - 1
    img_o = o.raytrace(False)
    tt_h = hip_outputs(rt)["output_total_transmittance"][..., 0]
    why = {"hits": np.any(hits_h != hits_o, axis=0), "T_total": np.any(np.abs(tt_h - img_o["output_total_transmittance"][..., 0]) > 2e-5, axis=0),
           "near_tie": ref["num_depth_ties"] > 0}
    flipped = why["hits"] | why["T_total"] | why["near_tie"]
    ys, xs = np.nonzero(flipped)
    listing = [(int(x), int(y), "+".join(k for k in why if why[k][y, x]), hits_h[:, y, x].tolist(), hits_o[:, y, x].tolist()) for y, x in zip(ys, xs)]
    assert 0 < len(listing) <= max_flipped, (name, err_all, listing[:20], len(listing))
    keep = ~flipped  # exactly the listed PIXELS are taken out, on both sides
    o.set_pixel_mask(keep)
    o.total_num_calls = k - 1
    ref_rest = o.raytrace(True, targets=tg)
    o.set_pixel_mask(None)
    rt.zero_grad()
    m.get_gaussians().total_weight.zero_()
    m.debug_set_pixel_mask(torch.from_numpy(keep.astype(np.uint8)).cuda())  # (a masked pixel is a pixel outside the image for every kernel of the launch)
    try:
        m.get_metadata().total_num_calls.fill_(k - 1)
        ren.render(camera, rt)
    finally:
        m.debug_set_pixel_mask(torch.empty(0, dtype=torch.uint8))
    torch.cuda.synchronize()
    gr_rest = hip_grads(rt)
    err_rest = {key: float(np.abs(gr_rest[key] - ref_rest[key]).max() / np.abs(ref[key]).max()) for key in live}
    worst_rest = max(err_rest.values())
    report(name, worst_grad_all_pixels=f"{worst_all:.1e}", worst_grad_without_listed=f"{worst_rest:.1e}", flipped_pixels=listing)
    assert worst_rest < bar, (name, err_rest, listing)
    return err_all, err_rest, listing


LOSS_WEIGHTS = dict(loss_weight_diffuse=5.0, loss_weight_specular=3.0, loss_weight_normal=2.5, loss_weight_depth=2.5, loss_weight_f0=1.0, loss_weight_roughness=1.0)  # make_pair's


def set_config_everywhere(rt, oracles, **cfg):
    """The same config scalars on the HIP tracer and on every oracle (loss weights, num_bounces: read on the device at every launch)."""
    mc = rt.cuda_module.get_config()
    for k, v in cfg.items():
        getattr(mc, k).fill_(v)
    for oo in oracles:
        oo.set_config(**cfg)


class SequenceMatched:
    """The two-pass idea of test_config_c_gradient_check_vs_oracle_at_size for small scenes, with THREE sides: HIP, the fp32 oracle `o` and the fp64
    oracle `o64` (Oracle(W, H, double=True), same scene / camera / config).

    pass 1 (`trace(None)`) traces every pixel on all three sides - images of a no-grad launch, gradients and the ordered composited sequences of a
    grad launch - and `masks(p1)` calls a pixel CLEAN when all three sides composite the same gaussians in the same order on every step (equal
    hit_sequence_hash; HIP: debug_hit_sequence_hash), agree on output_total_transmittance within 2e-5 on every step (the backward reads T - Ttot, quirk Q1)
    and on every forward output within 1e-3; pass 2 (`trace(clean)`) traces the clean pixels only, on all sides (debug_set_pixel_mask /
    Oracle.set_pixel_mask) with the same total_num_calls `K`: a masked pixel is a pixel outside the image, the others trace exactly the rays of pass 1.
    `parts`: the (rank, world) launches the HIP side is made of (images tiled, gradients summed)."""

    def __init__(self, ren, rt, o, o64, camera, tg, K=5, parts=((0, 1),)):
        self.ren, self.rt, self.o, self.o64, self.camera, self.tg, self.K, self.parts = ren, rt, o, o64, camera, tg, K, list(parts)
        self.W, self.H = o.W, o.H

    def _hip(self, mask, images):
        m = self.rt.cuda_module
        H, W = self.H, self.W
        if mask is not None:
            m.debug_set_pixel_mask(torch.from_numpy(mask.astype(np.uint8)).cuda())
        try:
            img = None
            if images:
                for name in OUT_KEYS:
                    getattr(m.get_framebuffer(), name).zero_()
                for r, w in self.parts:
                    m.set_partition(r, w)
                    m.get_metadata().total_num_calls.fill_(self.K - 1)
                    with torch.no_grad():
                        self.rt(self.camera)
                img = hip_outputs(self.rt)
            self.rt.zero_grad()
            m.get_gaussians().total_weight.zero_()
            rays, seq = 0, np.zeros((3, H, W), np.uint64)
            for r, w in self.parts:
                m.set_partition(r, w)
                m.get_metadata().total_num_calls.fill_(self.K - 1)
                self.ren.render(self.camera, self.rt)
                assert m.get_counters()[11] == 0  # no capacity overflow
                rays += m.get_counters()[0]
                seq = seq | m.debug_hit_sequence_hash().numpy().view(np.uint64)  # (0 outside the rank's tiles)
            torch.cuda.synchronize()
            assert rays == (H * W if mask is None else int(np.count_nonzero(mask)))
            return img, hip_grads(self.rt), seq
        finally:
            if mask is not None:
                m.debug_set_pixel_mask(torch.empty(0, dtype=torch.uint8))
            m.set_partition(0, 1)

    def _oracle(self, oo, mask, images, abs_sums):
        oo.set_pixel_mask(mask)
        try:
            oo.total_num_calls = self.K - 1
            ref = oo.raytrace(True, targets=self.tg, abs_sums=abs_sums)
            img = None
            if images:
                oo.total_num_calls = self.K - 1
                img = oo.raytrace(False)
            return ref, img
        finally:
            oo.set_pixel_mask(None)

    def trace(self, mask=None):
        """One launch set on all three sides (mask None: every pixel, with images). Returns a dict: img_{h,32,64}, grad_{h,32,64}, abs64 (o64's
        grad_abs), abs32, seq_{h,32,64} ([3,H,W] hashes)."""
        images = mask is None
        img_h, grad_h, seq_h = self._hip(mask, images)
        r32, img32 = self._oracle(self.o, mask, images, True)
        r64, img64 = self._oracle(self.o64, mask, images, True)
        return dict(img_h=img_h, img_32=img32, img_64=img64, grad_h=grad_h, grad_32={k: r32[k] for k in GRAD_KEYS}, grad_64={k: r64[k] for k in GRAD_KEYS},
                    abs64=r64["grad_abs"], abs32=r32["grad_abs"], seq_h=seq_h, seq_32=r32["hit_sequence_hash"], seq_64=r64["hit_sequence_hash"], ref32=r32)

    @staticmethod
    def masks(p1):
        """(same_sequence, clean) [H,W] masks of a pass-1 result: same_sequence = equal hashes on all sides and steps and total transmittances within 2e-5
        (the rays composite and pass the same candidates); clean = that and every forward output within 1e-3 between HIP and both oracles."""
        same = np.all((p1["seq_h"] == p1["seq_32"]) & (p1["seq_h"] == p1["seq_64"]), axis=0)
        for ref in (p1["img_32"], p1["img_64"]):
            same &= np.all(np.abs(p1["img_h"]["output_total_transmittance"] - ref["output_total_transmittance"]) <= 2e-5, axis=(0, -1))
        off = np.zeros_like(same)
        for key in OUT_KEYS:
            if key in ("output_ray_origin", "output_ray_direction"):
                continue  # (the next ray of a step: follows from the outputs, and has no loss of its own)
            for ref in (p1["img_32"], p1["img_64"]):
                off |= np.any(np.abs(p1["img_h"][key] - ref[key]) > 1e-3, axis=(0, -1))
        return same, same & ~off

    def run(self, max_unclean, name):
        """pass 1, the asserted cap on the pixels that are not clean, pass 2. Returns (pass 1, pass 2, clean mask)."""
        p1 = self.trace(None)
        same, clean = self.masks(p1)
        unclean = int(clean.size - np.count_nonzero(clean))
        report(name + "_pass1", pixels=int(clean.size), not_clean=unclean, other_sequence_or_T_total=int(clean.size - np.count_nonzero(same)), cap=max_unclean)
        assert unclean <= max_unclean, (name, unclean, max_unclean)
        p2 = self.trace(clean)
        reordered = int(np.count_nonzero(np.any(p2["seq_h"] != p2["seq_64"], axis=0) & clean))
        report(name + "_pass2", clean_pixels_with_another_sequence=reordered)
        return p1, p2, clean


def per_component_ratio(x, ref64, abs64, floor=1e-7):
    """The worst |x - ref| - floor * max|ref| over the components, in units of the reference's sum of absolute contributions of the component
    (grad_abs): the per-gaussian bar |x - ref| <= kappa * abs + floor * max|ref| holds iff the returned ratio is <= kappa. A component no hit feeds
    (abs == 0) must be within the floor (inf otherwise)."""
    worst = 0.0
    for k in GRAD_KEYS:
        if k == "total_weight":
            continue
        excess = np.abs(np.asarray(x[k], np.float64) - ref64[k]) - floor * float(np.abs(ref64[k]).max())
        fed = abs64[k] > 0
        if np.any(excess[~fed] > 0):
            return float("inf")
        if np.any(fed):
            worst = max(worst, float((np.maximum(excess[fed], 0.0) / abs64[k][fed]).max()))
    return worst
