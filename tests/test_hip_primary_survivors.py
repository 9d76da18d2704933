"""Primary tiles (8 x 8 tasks, step 0): the tile's frustum walk buffers leaves in rounds of up to 192, and every lane then tests its own ray against the
buffered leaves and appends what it accepts to its own list (csrc/forward_task.inc, the loop over `lbuf` inside `if (packet)`): in chunks of 64 leaves
a lane first tests its ray against every leaf's padded bounding sphere and then walks only the leaves it kept (csrc/trace.hip: staged_sphere,
ray_misses_sphere). A pair the pre-test drops must be one the candidate test would neither have counted nor appended, so per ray nothing may change:
the same candidates counted, the same list in the same order.

Scenes are built for what such a loop can get wrong - known leaf counts per tile at the 32- and 64-leaf boundaries, at the 192-leaf round boundary and
over several rounds, lanes with very different numbers of leaves to meet, lanes without a pixel, Gaussians whose bounding sphere is a poor or an
ill-conditioned bound (tiny and far, 1:100 discs, grazing rays of a jittered cloud), the segments in front of the near and behind the far plane - and
every scene is held against the CPU oracle and against the SAME binary's pair walk (4 x 4 tasks test every (ray, leaf) pair the tree yields).
Oracle results are computed once per scene and shared (`_ref`)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

from hip_common import BOTH_HELP_MODES, OUT_KEYS, cam_obj, generic_targets, grads_vs_oracle_listing_flipped_pixels, hip_outputs, make_pair, mismatch_list, psnr, ren, report  # noqa: F401

MAX_FLIPPED = 8  # grads_vs_oracle_listing_flipped_pixels' cap on the pixels two implementations may disagree on by an ulp
STRING_PIXEL = (4, 4)  # the ray the known-answer strings lie on: a central pixel of tile (0, 0)
STRING_KS = (1, 63, 64, 65, 191, 192, 193, 400)  # the 64-leaf batch boundary, the 192-leaf round boundary, several rounds


def _pixel_dir(cam, W, H, px, py):
    """Direction of pixel (px, py) without jitter (trace.hip: primary_direction; core/camera.h:17-36), fp64."""
    vs = np.tan(float(cam["fov"]) / 2.0)
    x = (W / H) * vs * (2.0 * (px + 0.5) / W - 1.0)
    y = vs * (1.0 - 2.0 * (py + 0.5) / H)
    c2w = np.asarray(cam["c2w"], np.float64)
    d = c2w[:, 0] * x + c2w[:, 1] * y - c2w[:, 2]
    return d / np.linalg.norm(d)


def _cloud(mean, scale, rotation=None, opacity=-3.0, seed=0):
    """Raw parameters of Gaussians at `mean` [n,3] with activated scales `scale` x (1, 0.7, 1.3), rotated at random; appearance from a seeded generator."""
    rng = np.random.default_rng(seed)
    mean = np.asarray(mean, np.float64).reshape(-1, 3)
    n = mean.shape[0]
    scale = np.broadcast_to(np.asarray(scale, np.float64), (n, 3)) * np.array([1.0, 0.7, 1.3])  # (isotropic: the rotation gradient would be rounding noise)
    if rotation is None:
        rotation = rng.normal(size=(n, 4))
    nrm = rng.normal(size=(n, 3))
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    g = dict(rgb=rng.uniform(0.05, 0.95, (n, 3)), normal=nrm, f0=rng.uniform(0.05, 0.95, (n, 3)), roughness=rng.uniform(0.05, 0.95, (n, 1)),
             opacity=np.broadcast_to(np.asarray(opacity, np.float64), (n, 1)), scale=np.log(scale), mean=mean, rotation=rotation)
    return {k: np.ascontiguousarray(np.asarray(v, np.float32)) for k, v in g.items()}


def _on_rays(cam, W, H, pixels, ts, offset=0.0):
    """Points on the rays of `pixels` at distances `ts` (one per pixel entry), moved sideways by `offset`."""
    o = np.asarray(cam["origin"], np.float64)
    pts = []
    for (px, py), t in zip(pixels, ts):
        d = _pixel_dir(cam, W, H, px, py)
        side = np.cross(d, [0.0, 0.0, 1.0])
        pts.append(o + t * d + offset * side / np.linalg.norm(side))
    return np.array(pts)


def _join(*clouds):
    return {k: np.ascontiguousarray(np.concatenate([c[k] for c in clouds], 0)) for k in clouds[0]}


def _scene(syn, name):
    """(gaussians, camera, W, H, config, pixel mask or None). num_bounces = 0 and jitter off unless the scene is about jitter."""
    cfg = dict(jitter_primary_rays=0, num_bounces=0)
    cam = syn.plus_x_camera()
    W, H, mask = 16, 16, None
    if name.startswith("string_") and name != "string_grad_193":  # K small Gaussians on ONE ray: all K reach that tile's buffer, the ray runs through every centre
        K = int(name.split("_")[1])
        g = _cloud(_on_rays(cam, W, H, [STRING_PIXEL] * K, 1.0 + 4.0 * np.arange(K) / K), 0.002)
    elif name == "string_grad_193":  # 193 leaves on one ray for the GRAD launch: larger and off the ray by a third of a radius (a ray through a centre has u = 0,
        K = 193                      # where the gradients of mean and scale are the rounding noise of u on both sides)
        g = _cloud(_on_rays(cam, W, H, [STRING_PIXEL] * K, 1.0 + 4.0 * np.arange(K) / K, offset=0.006), 0.02)
    elif name == "one_big_many_small":  # one Gaussian over the whole tile among 192 that each touch one pixel: every lane meets 3 or 4 of the tile's 193 leaves
        px = [(x, y) for y in range(8) for x in range(8)] * 3
        ts = np.repeat([2.0, 2.6, 3.4], 64)
        g = _join(_cloud(_on_rays(cam, W, H, [(4, 4)], [3.0], offset=0.03), 0.35, opacity=-2.0), _cloud(_on_rays(cam, W, H, px, ts), 0.004, seed=1))
    elif name == "half_idle":  # only the left half of tile (0, 0) meets anything: 32 lanes keep nothing
        px = [(x, y) for y in range(8) for x in range(4)] * 4
        g = _cloud(_on_rays(cam, W, H, px, np.repeat([1.5, 2.0, 2.5, 3.0], 32)), 0.004, seed=2)
    elif name == "ragged_20x12":  # lanes without a pixel in the right column and the bottom row of tiles
        W, H = 20, 12
        g = syn.random_blob_scene(400, seed=21)
    elif name == "masked_columns":  # every second column masked: lanes without a ray next to lanes with one
        g = syn.random_blob_scene(400, seed=22)
        mask = np.zeros((H, W), bool)
        mask[:, ::2] = True
    elif name == "tiny_far":  # scale 1e-4 at distance 50: |lo| = 5e5 object units, where the fp32 |u| is good to a few per cent of the unit sphere only
        px = [(x, y) for y in range(2, 6) for x in range(8)] * 3
        ts = np.repeat([49.0, 50.0, 51.0], 32)
        g = _join(_cloud(_on_rays(cam, W, H, px, ts), 1e-4, opacity=0.0, seed=3), _cloud(_on_rays(cam, W, H, px, ts + 0.3, offset=1.5e-4), 1e-4, opacity=0.0, seed=4))
    elif name == "discs":  # axis ratio 1:100, rotated at random, two of them exactly face-on and edge-on
        W, H = 32, 16
        g = syn.random_blob_scene(300, seed=23)
        g["scale"][:] = np.log(np.array([0.2, 0.2, 0.002], np.float32))
        g["rotation"][0] = [np.sqrt(0.5), 0, np.sqrt(0.5), 0]  # thin axis along the view direction: face-on
        g["rotation"][1] = [1, 0, 0, 0]                         # thin axis along z, seen from +x: edge-on
        g["mean"][0], g["mean"][1] = [2.0, 0.1, 0.1], [2.5, -0.2, 0.0]
    elif name == "blob_jitter":  # a dense random cloud, jitter on: hundreds of rays graze ellipsoid boundaries
        W, H = 48, 32
        g = syn.random_blob_scene(1500, seed=24)
        cfg["jitter_primary_rays"] = 1
    elif name == "near_far":  # test_near_plane_cut_and_far_plane's planes, with far more than 64 leaves in every tile
        W, H = 32, 16
        cam = dict(syn.default_camera())
        cam["znear"], cam["zfar"] = np.float32(1.5), np.float32(3.0)
        g = syn.make_scene(8000, "init", seed=6)
    else:
        raise KeyError(name)
    return g, cam, W, H, cfg, mask


UNEVEN = ["one_big_many_small", "half_idle", "ragged_20x12", "masked_columns"]
PAD = ["tiny_far", "discs", "blob_jitter"]
ALL_SCENES = ["string_%d" % k for k in STRING_KS] + UNEVEN + PAD + ["near_far"]
_REF = {}


def _ref(orc, syn, name):
    """The oracle's no-grad result of a scene: computed once, shared, never modified."""
    if name not in _REF:
        g, cam, W, H, cfg, mask = _scene(syn, name)
        o = orc.Oracle(W, H)
        o.set_camera(cam["origin"], cam["c2w"], cam["fov"], cam.get("znear", 0.01), cam.get("zfar", 999.9))
        o.set_gaussians(g)
        o.set_config(**dict(dict(loss_weight_diffuse=5.0, loss_weight_specular=3.0, loss_weight_normal=2.5, loss_weight_depth=2.5, loss_weight_f0=1.0, loss_weight_roughness=1.0), **cfg))
        o.update_bvh()
        o.set_pixel_mask(mask)
        o.total_num_calls = 0  # (the first launch of a fresh tracer sees 1)
        ref = o.raytrace(False)
        for v in ref.values():
            if isinstance(v, np.ndarray):
                v.setflags(write=False)
        _REF[name] = ref
    return _REF[name]


def _hip(ren, orc, syn, name, **kw):
    """One no-grad launch of a fresh tracer on a scene: (outputs, num_traversed_per_pixel, num_accumulated_per_pixel, counters)."""
    g, cam, W, H, cfg, mask = _scene(syn, name)
    rt, _ = make_pair(ren, orc, g, cam, W, H, cfg=cfg, **kw)
    m = rt.cuda_module
    if mask is not None:
        m.debug_set_pixel_mask(torch.from_numpy(mask.astype(np.uint8)).cuda())
    try:
        with torch.no_grad():
            rt(cam_obj(ren, cam), znear=float(cam["znear"]), zfar=float(cam["zfar"]))
        torch.cuda.synchronize()
    finally:
        if mask is not None:
            m.debug_set_pixel_mask(torch.empty(0, dtype=torch.uint8))
    st = m.get_stats()
    return hip_outputs(rt), st.num_traversed_per_pixel.cpu().numpy().reshape(H, W), st.num_accumulated_per_pixel.cpu().numpy().reshape(H, W), m.get_counters()


def _strict(name, out, ht, ha, ref, W, H, max_acc):
    """test_forward_strict_parity_primary's bars: hit counts exact (at most `max_acc` listed pixels), images within 2e-4 except at most two pixels whose
    hits composite in the other order, and the default statistic (candidates inside their ellipsoid) a subset of the reference's invocations."""
    bad_acc, n_acc = mismatch_list(ha, ref["num_accumulated"])
    flipped = (ha != ref["num_accumulated"].reshape(H, W)).reshape(-1)
    worst = {}
    for k in OUT_KEYS:
        err = np.abs(out[k] - ref[k]).reshape(3, H * W, -1).max(-1)[0]
        err = np.where(flipped, 0.0, np.nan_to_num(err, nan=np.inf))  # (a listed pixel is listed, not compared)
        worst[k] = (int((err >= 2e-4).sum()), float(err.max()))
    report("survivors_" + name, acc_mismatch=n_acc, acc_first=bad_acc, swapped_and_worst=worst, traversed_sum=int(ht.sum()), oracle_invocations=int(ref["num_traversed"].sum()))
    assert n_acc <= max_acc, bad_acc
    for k in OUT_KEYS:
        assert worst[k][0] <= 2 and worst[k][1] < 1e-2, (k, worst[k])
    assert (ht > ref["num_traversed"].reshape(H, W)).sum() <= 2 and (ht >= ha).all()


@pytest.mark.parametrize("K", STRING_KS)
def test_known_leaf_counts_on_one_ray(ren, orc, syn, K):
    """K Gaussians on the ray of one pixel: that ray is inside every one of them (it runs through the centres), so its default statistic is K - the
    oracle's invocation count of that pixel as well, since the ray also meets every cube - whatever word of the mask or round a leaf falls into."""
    name = "string_%d" % K
    _, _, W, H, _, _ = _scene(syn, name)
    ref = _ref(orc, syn, name)
    out, ht, ha, c = _hip(ren, orc, syn, name)
    px, py = STRING_PIXEL
    assert c[11] == 0
    assert int(ht[py, px]) == K and int(ref["num_traversed"].reshape(H, W)[py, px]) == K, (int(ht[py, px]), int(ref["num_traversed"].reshape(H, W)[py, px]))
    _strict(name, out, ht, ha, ref, W, H, max_acc=1)


@pytest.mark.parametrize("name", UNEVEN + ["near_far"])
def test_uneven_lanes_and_outer_segments_match_oracle(ren, orc, syn, name):
    _, _, W, H, _, mask = _scene(syn, name)
    ref = _ref(orc, syn, name)
    out, ht, ha, c = _hip(ren, orc, syn, name)
    assert c[11] == 0 and c[0] == (W * H if mask is None else int(mask.sum()))
    if name == "half_idle":
        assert int(ht[:8, 4:8].sum()) == 0 and int(ht[:8, :4].min()) == 4  # the right half of the tile meets nothing, every ray of the left half its four
    if name == "one_big_many_small":
        assert int(ht[:8, :8].min()) >= 3 and int(ht[:8, :8].max()) == 4  # its own three, and the big one where the ray is inside it
    _strict(name, out, ht, ha, ref, W, H, max_acc=1)


@pytest.mark.parametrize("name", PAD)
def test_ill_conditioned_and_grazing_candidates_are_all_kept(ren, orc, syn, name):
    """Where the fp32 candidate test is least exact (tiny far Gaussians, thin discs) and where most rays graze (jitter): the integer statistics are the
    oracle's, except pixels listed as flipped by an ulp (at most MAX_FLIPPED; the fp32 and the fp64 oracle differ on no pixel of these seeds)."""
    _, _, W, H, _, _ = _scene(syn, name)
    ref = _ref(orc, syn, name)
    out, ht, ha, c = _hip(ren, orc, syn, name)
    bad, nbad = mismatch_list(ha, ref["num_accumulated"])
    report("survivors_pad_" + name, acc_mismatch=nbad, first=bad, traversed_sum=int(ht.sum()), accumulated_sum=int(ha.sum()), psnr_final=round(psnr(out["output_final"], ref["output_final"]), 1))
    assert c[11] == 0 and int(ha.sum()) > 0
    assert nbad <= MAX_FLIPPED, bad
    assert (ht > ref["num_traversed"].reshape(H, W)).sum() <= 2 and (ht >= ha).all()


@pytest.mark.parametrize("name", ALL_SCENES)
def test_packet_walk_and_pair_walk_of_one_binary_agree(ren, orc, syn, monkeypatch, name):
    """8 x 8 tasks (frustum walk, lane = ray over the buffered leaves) against 4 x 4 tasks (pair walk: every pair the tree yields is tested), team help
    off: what a ray counts and composites is a property of the ray, equal pixel for pixel; the image to test_tile_partition_sums_to_full_image's 1e-6
    (measured on these scenes: no pixel differs in either count, output_final is equal to the bit)."""
    res = {}
    for rpt in (64, 16):
        monkeypatch.setenv("EGR_RAYS_PER_TASK", str(rpt))
        res[rpt] = _hip(ren, orc, syn, name, team_help=False)
    (o64, t64, a64, _), (o16, t16, a16, _) = res[64], res[16]
    bt, nt = mismatch_list(t64, t16)
    ba, na = mismatch_list(a64, a16)
    d = float(np.nanmax(np.abs(o64["output_final"] - o16["output_final"])))
    report("survivors_two_walks_" + name, traversed_mismatch=nt, accumulated_mismatch=na, final_max_abs_diff=d)
    assert nt == 0 and na == 0, (bt, ba)
    np.testing.assert_allclose(o64["output_final"], o16["output_final"], atol=1e-6)


@BOTH_HELP_MODES
@pytest.mark.parametrize("name", ["string_grad_193", "one_big_many_small"])
def test_grad_launch_matches_oracle(ren, orc, syn, name, team_help):
    g, cam, W, H, cfg, _ = _scene(syn, name)
    tg = generic_targets(syn, W, H)
    rt, o = make_pair(ren, orc, g, cam, W, H, cfg=dict(cfg, num_bounces=2), team_help=team_help)
    grads_vs_oracle_listing_flipped_pixels(ren, rt, o, cam_obj(ren, cam, tg), tg, W, H, "survivors_grads_%s_%s" % (name, "help" if team_help else "nohelp"), max_flipped=MAX_FLIPPED)
    assert rt.cuda_module.get_counters()[11] == 0


def test_a_list_longer_than_its_run_continues_in_an_extension_block(ren, orc, syn, monkeypatch):
    """193 accepted candidates on one ray of a packet tile whose own run holds 64 (the capacity test_candidate_lists_longer_than_capacity... sets)."""
    monkeypatch.setenv("EGR_RAYS_PER_TASK", "64")
    name = "string_193"
    _, _, W, H, _, _ = _scene(syn, name)
    ref = _ref(orc, syn, name)
    out, ht, ha, c = _hip(ren, orc, syn, name, fwd=1000)
    px, py = STRING_PIXEL
    assert c[11] == 0, "no overflow: the list continues in an extension block"
    assert int(ht[py, px]) == 193
    _strict(name + "_ext", out, ht, ha, ref, W, H, max_acc=1)
