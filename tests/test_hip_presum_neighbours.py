"""The neighbour pre-sum of a primary hit row (trace.hip: primary_presum - lane ^ 1, then lane ^ 8, as DPP adds followed by a select) on scenes made for it:
about 40 gaussians several pixels wide, so that neighbouring pixels composite the SAME gaussian at the same hit index and their contributions are summed in
registers, among about 300 small ones that break the runs. Two bounces, jitter off, both help modes.

Images: 16x16 (whole 8x8 tiles), 20x12 (ragged tiles: the lane ^ 1 / lane ^ 8 partner of an edge pixel lies outside the image) and 16x16 with a pixel mask
that switches every second column off (EVERY lane ^ 1 partner is inactive). Each is held against the oracle with the suite's helper and bars
(hip_common.grads_vs_oracle_listing_flipped_pixels: 1e-3 of each tensor's maximum on sequence-matched pixels), and traced once more as the four ranks of a
partition in 8x4-pixel tasks (lanes 32-63 of every wave idle: no lane ^ 8 partner in the lower half of a tile's rows), whose summed gradients must equal the
whole-image launch within 1e-5 of each tensor's maximum - the suite's bar for two launches whose float atomics arrive in another order."""
import numpy as np
import pytest

from hip_common import BOTH_HELP_MODES, GRAD_KEYS, cam_obj, generic_targets, grads_vs_oracle_listing_flipped_pixels, hip_grads, make_pair, ren, report, run_grad, torch  # noqa: F401

pytestmark = pytest.mark.gpu

CFG = dict(jitter_primary_rays=0, num_bounces=2)
CASES = {  # name: (W, H, every second column masked)
    "whole_tiles_16x16": (16, 16, False),
    "ragged_tiles_20x12": (20, 12, False),
    "every_second_column_off_16x16": (16, 16, True),
}
WORLD = 4  # ranks of the partition run (a 16x16 image is ONE macro tile: three of the ranks have nothing to trace, the fourth is under-filled)


def neighbour_scene(syn):
    """40 gaussians two to five pixels wide (a pixel at depth 2.5 is 0.11 wide at these image sizes) + 300 smaller than a pixel, in front of the +x camera."""
    wide = syn.random_blob_scene(40, seed=21, extent=0.8, depth_range=(2.0, 3.5), scale_range=(0.12, 0.3))
    small = syn.random_blob_scene(300, seed=22, extent=0.9, depth_range=(1.5, 4.0), scale_range=(0.01, 0.04))
    return {k: np.ascontiguousarray(np.concatenate([wide[k], small[k]])) for k in wide}


def column_mask(W, H):
    mask = np.zeros((H, W), bool)
    mask[:, 0::2] = True
    return mask


@BOTH_HELP_MODES
@pytest.mark.parametrize("case", sorted(CASES))
def test_presum_neighbours_against_the_oracle_and_as_partition_ranks(ren, orc, syn, case, team_help):
    W, H, masked = CASES[case]
    g, cam, tg = neighbour_scene(syn), syn.plus_x_camera(), generic_targets(syn, W, H)
    rt, o = make_pair(ren, orc, g, cam, W, H, cfg=CFG, team_help=team_help)
    m = rt.cuda_module
    camera = cam_obj(ren, cam, tg)
    name = f"presum_{case}_{'help_on' if team_help else 'help_off'}"
    mask = column_mask(W, H) if masked else None
    if masked:
        m.debug_set_pixel_mask(torch.from_numpy(mask.astype(np.uint8)).cuda())
        o.set_pixel_mask(mask)
    try:
        # ---- the whole image in one launch, against the oracle
        grads_vs_oracle_listing_flipped_pixels(ren, rt, o, camera, tg, W, H, name)
        if masked:  # (the helper's second pass, if it ran one, left no mask behind)
            m.debug_set_pixel_mask(torch.from_numpy(mask.astype(np.uint8)).cuda())
        K = int(m.get_metadata().total_num_calls)
        m.get_metadata().total_num_calls.fill_(K - 1)
        run_grad(ren, rt, camera)
        whole = hip_grads(rt)
        rays_whole = m.get_counters()[0]
        assert rays_whole == (int(mask.sum()) if masked else W * H)
        hits = m.debug_step_hits().numpy()
        assert hits[0].max() >= 4 and hits[1:].sum() > 0, hits.sum(axis=(1, 2))  # rows of several hits on the primary step, and the bounce steps ran
        # ---- the same rays as the ranks of a partition, 8x4 tasks, gradients summed
        m.set_rays_per_task(32)
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
        assert rays == rays_whole
        summed = hip_grads(rt)
    finally:
        m.set_partition(0, 1)
        m.set_rays_per_task(0)
        m.debug_set_pixel_mask(torch.empty(0, dtype=torch.uint8))
        o.set_pixel_mask(None)
    err = {k: float(np.abs(summed[k] - whole[k]).max() / np.abs(whole[k]).max()) for k in GRAD_KEYS if np.abs(whole[k]).max() > 0}
    report(name + "_ranks_summed_vs_whole", **{k: f"{v:.1e}" for k, v in err.items()})
    assert len(err) == len(GRAD_KEYS), sorted(err)  # every gradient tensor is fed
    for k, v in err.items():
        assert v < 1e-5, (name, k, v)
