"""The row sum of the backward chain's primary step (trace.hip: primary_table_add): the lanes of a hit row that hold the SAME gaussian link up through their
table slot's claim word, are summed in registers by pointer jumping (ds_bpermute pulls), and one lane per gaussian, the group's leader, takes the sum to the
wave's LDS table in a single pass. +x camera, jitter off, two bounces, both help modes.

  * known group sizes: an 8x8 image (one tile, lane = 8 y + x) with one faint, wide gaussian over the whole tile and a second one behind it - two hit rows in which
    every active lane holds the same record - under a pixel mask of m = 1 ... 64 active pixels drawn as a seeded permutation of the lanes, so that ranks and
    predecessors are no neighbours (m = 64: six pointer-jumping steps; m = 1: a leader with nobody before it);
  * several groups in a row: the scene of test_hip_presum_neighbours (40 wide + 300 small gaussians) at 16x16, at 20x12 (ragged tiles) and at 16x16 with every
    second column masked;
  * more distinct gaussians in one tile than the table holds: 200 sub-tile gaussians at many depths and three wide ones in one 8x8 tile - a full table is flushed
    while lanes wait, the second probe and the record path of a hit without a slot run; more records leave than two per distinct gaussian;
  * each of the last two also as the four ranks of a partition in 8x4-pixel tasks (lanes 32-63 of every wave idle), summed against the whole-image launch within
    1e-5 of each tensor's maximum - the suite's bar for two launches whose float atomics arrive in another order;
  * train_views over two 16x16 views against the two single launches, same bar (the batch kernel shares the functions).

Every comparison with the oracle uses hip_common.grads_vs_oracle_listing_flipped_pixels with its own bars and must list NO pixel: scenes, seeds and the second
view are chosen so that the fp32 and the fp64 oracle agree on every pixel's integer statistics and ordered hit sequences (asserted here, on the CPU), i.e. no ray
of these scenes is decided by the last bits."""
import numpy as np
import pytest

from hip_common import BOTH_HELP_MODES, GRAD_KEYS, cam_obj, generic_targets, grads_vs_oracle_listing_flipped_pixels, hip_grads, make_pair, ren, report, run_grad, torch  # noqa: F401
from test_hip_presum_neighbours import CFG, column_mask, neighbour_scene
from test_hip_train_views import assert_grads_close, batched, sequential, view_targets

pytestmark = pytest.mark.gpu

GROUP_SIZES = [1, 2, 3, 4, 5, 7, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64]
GROUP_SEED, LANE_SEED, CROWDED_SEED = 1, 7, 2
WORLD = 4
INT_STATS = ["num_traversed", "num_accumulated", "num_composited_all_steps", "effective_steps", "num_composited_per_step", "num_depth_ties", "hit_sequence_hash"]
SEVERAL = {  # name: (W, H, every second column masked)
    "whole_tiles_16x16": (16, 16, False),
    "ragged_tiles_20x12": (20, 12, False),
    "every_second_column_off_16x16": (16, 16, True),
}
_PAIRS = {}


def group_scene(syn, seed=GROUP_SEED):
    """Two faint gaussians wider than the 8x8 image (semi-axes about 2 at depths 2.6 and 3.7; the image is 1.8 wide at depth 2.5), one behind the other."""
    g = syn.random_blob_scene(2, seed=seed)
    g["mean"] = np.array([[2.6, 0.05, -0.03], [3.7, -0.04, 0.06]], np.float32)
    g["scale"] = np.log(np.array([[1.2, 1.3, 1.25], [1.3, 1.2, 1.35]], np.float32))
    g["opacity"] = np.array([[-1.5], [-1.2]], np.float32)
    return g


def crowded_scene(syn, seed=CROWDED_SEED):
    """200 faint gaussians one to four pixels wide at many depths and three wide ones, all in the one tile of an 8x8 image: far more than the table's 80 slots."""
    small = syn.random_blob_scene(200, seed=seed, extent=0.85, depth_range=(1.5, 4.5), scale_range=(0.1, 0.25))
    small["opacity"] = np.random.default_rng(seed + 100).uniform(-2.5, -1.0, (200, 1)).astype(np.float32)
    wide = syn.random_blob_scene(3, seed=seed + 1)
    wide["mean"] = np.array([[2.2, 0.1, 0.0], [3.2, -0.1, 0.1], [4.8, 0.0, -0.1]], np.float32)
    wide["scale"] = np.log(np.array([[1.0, 1.1, 1.05], [1.4, 1.3, 1.35], [1.9, 2.0, 1.95]], np.float32))
    wide["opacity"] = np.array([[-2.0], [-1.8], [-1.6]], np.float32)
    return {k: np.ascontiguousarray(np.concatenate([small[k], wide[k]])) for k in small}


def lane_mask(m):
    """m active pixels of the 8x8 tile: the first m lanes of a seeded permutation (lane = 8 y + x)."""
    mask = np.zeros(64, bool)
    mask[np.random.default_rng(LANE_SEED).permutation(64)[:m]] = True
    return mask.reshape(8, 8)


def two_views(syn):
    eye = np.array([0.0, 0.12, 0.06])
    second = dict(origin=eye.astype(np.float32), c2w=syn.look_at(eye, (1.0, 0.03, -0.02)).astype(np.float32), fov=np.float32(0.75), znear=np.float32(0.01), zfar=np.float32(999.9))
    return [syn.plus_x_camera(), second]


def assert_oracles_agree(orc, syn, g, cam, W, H, name):
    """The fp32 and the fp64 oracle trace every pixel alike: integer statistics and ordered hit sequences (CPU)."""
    outs = []
    for double in (False, True):
        o = orc.Oracle(W, H, double=double)
        o.set_camera(cam["origin"], cam["c2w"], cam["fov"], cam.get("znear", 0.01), cam.get("zfar", 999.9))
        o.set_gaussians(g)
        o.set_config(**CFG)
        o.update_bvh()
        outs.append(o.raytrace(False))
    for k in INT_STATS:
        assert np.array_equal(outs[0][k], outs[1][k]), (name, k, int(np.count_nonzero(outs[0][k] != outs[1][k])))


def pair(ren, orc, syn, key, g, cam, W, H, team_help):
    """(tracer, oracle, camera object, targets) of a scene, made once per help mode; the oracles' agreement is checked when it is made."""
    k = (key, W, H, team_help)
    if k not in _PAIRS:
        assert_oracles_agree(orc, syn, g, cam, W, H, key)
        tg = generic_targets(syn, W, H)
        rt, o = make_pair(ren, orc, g, cam, W, H, cfg=CFG, team_help=team_help)
        _PAIRS[k] = (rt, o, cam_obj(ren, cam, tg), tg)
    return _PAIRS[k]


def set_masks(m, o, mask):
    if mask is None:
        m.debug_set_pixel_mask(torch.empty(0, dtype=torch.uint8))
        o.set_pixel_mask(None)
    else:
        m.debug_set_pixel_mask(torch.from_numpy(mask.astype(np.uint8)).cuda())
        o.set_pixel_mask(mask)


def against_oracle_without_listing(ren, rt, o, camera, tg, W, H, name):
    err, _, listing = grads_vs_oracle_listing_flipped_pixels(ren, rt, o, camera, tg, W, H, name)
    assert listing == [], (name, err, listing)
    return err


def ranks_summed_against_whole(ren, rt, camera, mask, W, H, name):
    """The launch once more as a whole, then as the four ranks of a partition in 8x4 tasks: summed gradients within 1e-5. Returns (whole gradients, counters, step hits)."""
    m = rt.cuda_module
    K = int(m.get_metadata().total_num_calls)
    m.get_metadata().total_num_calls.fill_(K - 1)
    run_grad(ren, rt, camera)
    whole, counters, hits = hip_grads(rt), list(m.get_counters()), m.debug_step_hits().numpy().copy()
    assert counters[0] == (int(mask.sum()) if mask is not None else W * H) and counters[11] == 0
    m.set_rays_per_task(32)
    try:
        rt.zero_grad()
        m.get_gaussians().total_weight.zero_()
        rays = 0
        for r in range(WORLD):
            m.set_partition(r, WORLD)
            m.get_metadata().total_num_calls.fill_(K - 1)
            ren.render(camera, rt)
            assert m.get_counters()[11] == 0
            rays += m.get_counters()[0]
        torch.cuda.synchronize()
        summed = hip_grads(rt)
    finally:
        m.set_partition(0, 1)
        m.set_rays_per_task(0)
    assert rays == counters[0]
    err = {k: float(np.abs(summed[k] - whole[k]).max() / np.abs(whole[k]).max()) for k in GRAD_KEYS if np.abs(whole[k]).max() > 0}
    report(name + "_ranks_summed_vs_whole", **{k: f"{v:.1e}" for k, v in err.items()})
    assert len(err) == len(GRAD_KEYS), sorted(err)
    for k, v in err.items():
        assert v < 1e-5, (name, k, v)
    return whole, counters, hits


@BOTH_HELP_MODES
@pytest.mark.parametrize("m_active", GROUP_SIZES)
def test_known_group_sizes(ren, orc, syn, m_active, team_help):
    rt, o, camera, tg = pair(ren, orc, syn, "group", group_scene(syn), syn.plus_x_camera(), 8, 8, team_help)
    m = rt.cuda_module
    mask = lane_mask(m_active)
    assert int(mask.sum()) == m_active
    set_masks(m, o, mask)
    try:
        against_oracle_without_listing(ren, rt, o, camera, tg, 8, 8, f"row_groups_m{m_active}_{'help_on' if team_help else 'help_off'}")
        assert m.get_counters()[0] == m_active
        hits = m.debug_step_hits().numpy()
        assert (hits[0][mask] == 2).all() and (hits[0][~mask] == 0).all(), hits[0]  # two rows, every active lane holds the row's one record
        weight = hip_grads(rt)["total_weight"]
        assert (weight[:, 0] > 0).all()  # both gaussians were summed
    finally:
        set_masks(m, o, None)


@BOTH_HELP_MODES
@pytest.mark.parametrize("case", sorted(SEVERAL))
def test_several_groups_in_a_row(ren, orc, syn, case, team_help):
    W, H, masked = SEVERAL[case]
    rt, o, camera, tg = pair(ren, orc, syn, "several", neighbour_scene(syn), syn.plus_x_camera(), W, H, team_help)
    m = rt.cuda_module
    mask = column_mask(W, H) if masked else None
    name = f"row_groups_{case}_{'help_on' if team_help else 'help_off'}"
    set_masks(m, o, mask)
    try:
        against_oracle_without_listing(ren, rt, o, camera, tg, W, H, name)
        _, _, hits = ranks_summed_against_whole(ren, rt, camera, mask, W, H, name)
        assert hits[0].max() >= 4 and hits[1:].sum() > 0, hits.sum(axis=(1, 2))  # rows of several hits on the primary step, and the bounce steps ran
    finally:
        set_masks(m, o, None)


@BOTH_HELP_MODES
def test_more_gaussians_in_a_tile_than_the_table_holds(ren, orc, syn, team_help):
    rt, o, camera, tg = pair(ren, orc, syn, "crowded", crowded_scene(syn), syn.plus_x_camera(), 8, 8, team_help)
    name = f"row_groups_crowded_{'help_on' if team_help else 'help_off'}"
    against_oracle_without_listing(ren, rt, o, camera, tg, 8, 8, name)
    whole, counters, hits = ranks_summed_against_whole(ren, rt, camera, None, 8, 8, name)
    distinct = int(np.count_nonzero(whole["total_weight"][:, 0] > 0))  # every gaussian some ray composited, on any step: no fewer than the tile's primary step met
    bounce_hits = int(hits[1:].sum())  # a bounce hit is one record
    primary_records = int(counters[13]) - bounce_hits
    report(name, distinct=distinct, primary_records=primary_records, bounce_hits=bounce_hits, rows=int(hits[0].max()))
    assert distinct > 80  # more than the table's slots
    assert primary_records > 2 * distinct, (primary_records, distinct)  # the table was emptied while the tile was under way: a gaussian left more than once


def test_two_views_in_one_launch(ren, orc, syn):
    g, W, H = neighbour_scene(syn), 16, 16
    cams = two_views(syn)
    for i, c in enumerate(cams):
        assert_oracles_agree(orc, syn, g, c, W, H, f"view{i}")
    rt, _ = make_pair(ren, orc, g, cams[0], W, H, cfg=CFG)
    objs = [cam_obj(ren, c, t) for c, t in zip(cams, view_targets(syn, W, H, 2))]
    seq, work_s, st_s = sequential(ren, rt, objs, 40)
    bat, work_b, st_b = batched(ren, rt, objs, 40)
    assert st_s == 0 and st_b == 0 and np.array_equal(work_b, work_s) and work_b[0] == 2 * W * H and work_b[1] > 0
    assert_grads_close(bat, seq, "row_groups_train_views_vs_sequential")
