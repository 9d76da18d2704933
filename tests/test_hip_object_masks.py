"""Per-object coverage on the GPU (csrc/trace.hip: k_forward_objects; Raytracer.object_masks; editing.selection_masks / pick) against the reference's loop restated on
this tracer - one full render per object with the object's 0/1 indicator as the diffuse colour (gaussian_viewer.py:292-321) - BIT FOR BIT, against the CPU oracle at
the strict-parity bar of an output buffer, and as a query that leaves no trace. The scene is test_hip_edit.py's room at 64 x 64 (objects = the sphere boxes), tracers
without team help.

The camera was checked on the CPU oracle (indicator renders, jitter off) before the first GPU run, and every run asserts the same three facts (`facts`): every
sphere's mask is non-zero somewhere (1314 / 1127 / 981 pixels), pixels stop short of the total transmittance (T - full_T > 0: all 4096, so rem != 0 in R4), and
pixels composite more than 16 hits (92; the longest ray 23) - more than one reference batch and three of this kernel's batches of eight."""
import importlib

import numpy as np
import pytest

import hip_common as hc
from hip_common import ren  # noqa: F401
from test_hip_edit import bits, ed, pin_seed, room, tracer  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
PKG = "editable-gaussian-reflections_amd"
W = H = 64
SPHERES = ["sphere0", "sphere1", "sphere2"]


def editable(ren, ed, syn, jitter=False, **kw):
    g, boxes, cam = room(ren, syn)
    e = ed.EditableGaussians(ren.GaussianParams(g), boxes, **kw)
    rt = tracer(ren, e)
    rt.cuda_module.get_config().jitter_primary_rays.fill_(bool(jitter))
    return g, boxes, cam, e, rt


def loop_masks(ren, rt, cam, names):
    """The reference's loop on this tracer: per name the indicator into _diffuse, the pinned seed, render(force_update_bvh=True), rgb[0]'s first channel (the three are
    the same sums: asserted), then _diffuse restored."""
    e = rt.pc
    keep = e._diffuse.clone()
    out = []
    try:
        for name in names:
            e._diffuse.copy_(e.selection(name).to(torch.float32)[:, None].expand(-1, 3))
            pin_seed(rt)
            with torch.no_grad():
                r = ren.render(cam, rt, targets_available=False, force_update_bvh=True)
            assert torch.equal(bits(r.rgb[0][0]), bits(r.rgb[0][1])) and torch.equal(bits(r.rgb[0][0]), bits(r.rgb[0][2])), name
            out.append(r.rgb[0][0].clone())
    finally:
        e._diffuse.copy_(keep)
    with torch.no_grad():  # the model's own colours are back in the tracer
        pin_seed(rt)
        ren.render(cam, rt, targets_available=False, force_update_bvh=True)
    return torch.stack(out)


def query(ed, rt, cam, names=None):
    pin_seed(rt)
    return ed.selection_masks(cam, rt, names=names)


def numpy_hit_top(masks):
    """The definitions of the header on a [K,H,W] array: hit bit j = masks[j] != 0; top = the first index of the largest mask under a strict '>' from -inf (a NaN
    never wins), -1 where hit == 0."""
    K = masks.shape[0]
    hit = np.zeros(masks.shape[1:], np.uint32)
    top = np.full(masks.shape[1:], -1, np.int32)
    best = np.full(masks.shape[1:], -np.inf, np.float32)
    for j in range(K):
        hit |= (masks[j] != 0).astype(np.uint32) << np.uint32(j)
        better = masks[j] > best
        best = np.where(better, masks[j], best)
        top = np.where(better, np.int32(j), top)
    return hit, np.where(hit != 0, top, np.int32(-1)).astype(np.int32)


def assert_equals_loop(res, want, names):
    assert res.names == list(names) and res.masks.shape == (len(names), H, W) and res.masks.dtype == torch.float32
    assert res.hit.shape == (H, W) and res.hit.dtype == torch.int32 and res.top.shape == (H, W) and res.top.dtype == torch.int32
    for j, name in enumerate(names):
        diff = int((bits(res.masks[j]) != bits(want[j])).sum())
        assert diff == 0, (name, diff, float((res.masks[j] - want[j]).abs().max()))
    hit, top = numpy_hit_top(res.masks.cpu().numpy())
    assert np.array_equal(res.hit.cpu().numpy().view(np.uint32), hit)
    assert np.array_equal(res.top.cpu().numpy(), top)


def facts(ren, rt, cam, masks):
    """What keeps the comparisons from passing vacuously (module docstring), on the GPU's own primary step."""
    cfg = rt.cuda_module.get_config()
    nb = int(cfg.num_bounces)
    cfg.num_bounces.fill_(0)  # (the per-pixel hit count is the last step's)
    pin_seed(rt)
    with torch.no_grad():
        ren.render(cam, rt, targets_available=False)
    cfg.num_bounces.fill_(nb)
    fb, st = rt.cuda_module.get_framebuffer(), rt.cuda_module.get_stats()
    rem = fb.output_transmittance[0] - fb.output_total_transmittance[0]
    assert all(int((masks[j] != 0).sum()) > 100 for j in range(masks.shape[0])), [int((m != 0).sum()) for m in masks]
    assert int((rem > 0).sum()) > 100
    assert int((st.num_accumulated_per_pixel > 16).sum()) >= 8, int(st.num_accumulated_per_pixel.max())


# ---------------------------------------------------------------- 1: bit equality with the loop

@pytest.mark.parametrize("jitter", [False, True], ids=["jitter_off", "jitter_on"])
def test_masks_equal_the_reference_loop_bit_for_bit(ren, ed, syn, jitter):
    g, boxes, cam, e, rt = editable(ren, ed, syn, jitter=jitter)
    want = loop_masks(ren, rt, cam, SPHERES)
    res = query(ed, rt, cam)
    assert res.names == SPHERES  # every object but "everything", in pc.names order
    assert_equals_loop(res, want, SPHERES)
    facts(ren, rt, cam, res.masks)
    both = (res.hit & (res.hit - 1)) != 0
    assert int(both.sum()) > 0  # pixels under two objects: the pick rules differ there
    y, x = [int(v) for v in torch.nonzero(both)[0]]
    h = int(res.hit[y, x])
    assert ed.pick(res, x, y) == SPHERES[h.bit_length() - 1] and ed.pick(res, x, y, rule="top") == SPHERES[int(res.top[y, x])]
    none = torch.nonzero(res.hit == 0)
    if len(none):
        assert ed.pick(res, int(none[0][1]), int(none[0][0])) is None and ed.pick(res, int(none[0][1]), int(none[0][0]), rule="top") is None


# ---------------------------------------------------------------- 2: the query leaves no trace

def snapshot(rt):
    cabi = importlib.import_module(PKG + ".c_abi")
    m = rt.cuda_module
    fb, st, md, cfg, gs = m.get_framebuffer(), m.get_stats(), m.get_metadata(), m.get_config(), m.get_gaussians()
    snap = {"fb." + k: getattr(fb, k).clone() for k in cabi.FRAMEBUFFER_FIELDS}
    snap.update({"stats." + k: getattr(st, k).clone() for k in cabi.STATS_FIELDS})
    snap.update({"meta." + k: getattr(md, k).clone() for k in cabi.METADATA_FIELDS})
    snap.update({"cfg." + k: getattr(cfg, k).clone() for k in cabi.CONFIG_FIELDS})
    snap["grad_flat"] = gs.grad_flat.clone()
    snap.update({"g." + k: getattr(gs, k).clone() for k in cabi.GAUSSIAN_PARAMS})
    return snap


def same_bits(a, b):
    raw = lambda t: t.contiguous().view(torch.uint8) if t.dtype == torch.bool else t.contiguous().view(torch.int32)
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(raw(a), raw(b))


def history(ren, ed, syn, with_query):
    """A grad launch (gradients, total_weight and the hit arena hold something), two accumulating jittered renders (the accumulators too), [the query], one more render."""
    g, boxes, cam, e, rt = editable(ren, ed, syn, jitter=True)
    m = rt.cuda_module
    pin_seed(rt)
    rt.zero_grad()
    ren.render(cam, rt, targets_available=False)  # forward + backward
    m.get_config().accumulate_samples.fill_(True)
    with torch.no_grad():
        ren.render(cam, rt, targets_available=False)
        ren.render(cam, rt, targets_available=False)
    before, arena = snapshot(rt), m.debug_hit_sequence_hash().clone()
    res = None
    if with_query:
        res = ed.selection_masks(cam, rt)
        torch.cuda.synchronize()
        after = snapshot(rt)
        changed = [k for k in before if not same_bits(before[k], after[k])]
        assert changed == [], changed
        assert torch.equal(m.debug_hit_sequence_hash(), arena)  # the hit arena of the last grad launch
        assert float(before["fb.accumulated_rgb"].abs().max()) > 0 and int(before["fb.accumulated_sample_count"]) == 2 and float(before["grad_flat"].abs().max()) > 0
        assert int(before["meta.total_num_calls"]) == 7 and int(before["cfg.num_bounces"]) == int(m.get_config().num_bounces) > 0
        assert m.get_counters()[11] == 0  # (no capacity overflow in the query's own launch)
    with torch.no_grad():
        ren.render(cam, rt, targets_available=False)
    return snapshot(rt), res


def test_query_leaves_no_trace_and_the_next_render_is_unchanged(ren, ed, syn):
    with_q, res = history(ren, ed, syn, True)
    without, _ = history(ren, ed, syn, False)
    assert float(res.masks.abs().max()) > 0
    skip = ("grad_flat",)  # (float atomics of the grad launch: equal up to the order of the additions, and no input of a render)
    changed = [k for k in without if k not in skip and not same_bits(without[k], with_q[k])]
    assert changed == [], changed
    assert int(with_q["meta.total_num_calls"]) == 8


# ---------------------------------------------------------------- 3: membership cases

def test_k1_reordered_subset_and_everything(ren, ed, syn):
    g, boxes, cam, e, rt = editable(ren, ed, syn)
    for names in (["sphere1"], ["sphere2", "sphere0"], ["everything"], ["everything", "sphere1", "sphere0", "sphere2"]):
        want = loop_masks(ren, rt, cam, names)
        assert_equals_loop(query(ed, rt, cam, names), want, names)
    # "everything" is rgb[0] of an all-ones model: every row counts, so hit has its bit wherever anything is composited
    res = query(ed, rt, cam, ["everything"])
    assert bool(e.selection("everything").all()) and int((res.hit == 1).sum()) > H * W // 2 and set(res.top.unique().tolist()) <= {-1, 0}
    assert torch.equal(res.top == 0, res.hit == 1)


def test_k32_hand_made_membership(ren, ed, syn):
    """32 objects through a hand-made selection_mask: bit 31 (the sign bit) in use, rows in several objects, rows in none, and one object (bit 17) without rows - an
    all-zero mask and a clear hit bit."""
    g, boxes3, cam = room(ren, syn)
    n = g["mean"].shape[0]
    rng = np.random.default_rng(32)
    word = np.zeros(n, np.uint32)
    for b in range(32):
        if b != 17:
            word |= (rng.random(n) < (0.5 if b == 31 else 0.04 + 0.002 * b)).astype(np.uint32) << np.uint32(b)
    word[rng.random(n) < 0.2] = 0
    count = np.array([bin(int(w)).count("1") for w in word])
    assert (count == 0).sum() > 100 and (count >= 2).sum() > 100 and (count == 1).sum() > 100 and (word >> 31).sum() > 100 and not ((word >> 17) & 1).any()
    names = ["o%d" % b for b in range(32)]
    boxes = {name: dict(min=[-1.0, -1.0, -1.0], max=[1.0, 1.0, 1.0]) for name in names}
    e = ed.EditableGaussians(ren.GaussianParams(g), boxes, selection_mask=torch.from_numpy(word.view(np.int32)).cuda())
    rt = tracer(ren, e)
    want = loop_masks(ren, rt, cam, names)
    res = query(ed, rt, cam)
    assert_equals_loop(res, want, names)
    hit = res.hit.cpu().numpy().view(np.uint32)
    assert not res.masks[17].any() and not ((hit >> 17) & 1).any()
    assert all(bool(res.masks[b].any()) for b in range(32) if b != 17) and int((hit >> 31).sum()) > 100 and int((res.top == 31).sum()) > 0
    y, x = [int(v) for v in np.argwhere((hit >> 31) == 1)[0]]
    assert ed.pick(res, x, y) == "o31"
    # the same objects asked for in reverse: output index j is selection bit 31 - j
    rev = query(ed, rt, cam, names[::-1])
    assert torch.equal(bits(rev.masks), bits(res.masks.flip(0)))
    assert_equals_loop(rev, want.flip(0), names[::-1])


# ---------------------------------------------------------------- 4: geometry edits act, colour edits do not

def test_geometry_edits_act_and_colour_edits_do_not(ren, ed, syn):
    g, boxes, cam, e, rt = editable(ren, ed, syn)
    plain = query(ed, rt, cam)
    assert_equals_loop(plain, loop_masks(ren, rt, cam, SPHERES), SPHERES)
    # a transform edit: the masks are the loop's on the edited tracer, and not the unedited ones
    e.edits["sphere0"] = ed.Edit(translate_x=-0.2, translate_y=0.15, scale=1.2, rotate_z=35.0)
    assert e.dirty_check() is True
    moved = query(ed, rt, cam)  # (exports and refits: dirty)
    assert e.dirty_check() is False and rt.cuda_module.check_bvh() == 0, rt.cuda_module.last_error()
    assert_equals_loop(moved, loop_masks(ren, rt, cam, SPHERES), SPHERES)
    assert not torch.equal(bits(moved.masks[0]), bits(plain.masks[0]))
    # removed: a zero mask; cleared: back bit for bit
    e.edits["sphere2"].removed = True
    gone = query(ed, rt, cam)
    assert not gone.masks[2].any() and not ((gone.hit >> 2) & 1).any() and bool(gone.masks[1].any())
    assert_equals_loop(gone, loop_masks(ren, rt, cam, SPHERES), SPHERES)
    e.edits["sphere2"].removed = False
    back = query(ed, rt, cam)
    assert torch.equal(bits(back.masks), bits(moved.masks))
    # a diffuse-colour edit on top: dirty, exported, and no mask bit changes (upstream the loop's indicator goes through this edit and every mask is tinted:
    # the loop is not the yardstick here - the masks without the colour edit are)
    e.edits["sphere1"] = ed.Edit(diffuse_override=(0.9, 0.1, 0.1, 1.0), diffuse_value_mult=0.5)
    assert e.dirty_check() is True
    tinted = query(ed, rt, cam)
    assert torch.equal(bits(tinted.masks), bits(moved.masks)) and torch.equal(tinted.hit, moved.hit) and torch.equal(tinted.top, moved.top)


def test_duplicate_has_a_mask_of_its_own(ren, ed, syn):
    g, boxes, cam, e, rt = editable(ren, ed, syn)
    before = query(ed, rt, cam)
    e.edits["sphere1"] = ed.Edit(translate_x=-0.3, translate_y=0.5, translate_z=0.2)
    k = e.duplicate_object("sphere1", 0.3)  # the copy lands in the middle of the view (test_hip_edit.py)
    rt.rebuild_bvh()
    e.edits["sphere1"] = ed.Edit()  # the source back where it was; the copy stays (its rows hold the shifted positions)
    names = SPHERES + ["sphere1_copy"]
    res = query(ed, rt, cam)
    assert res.names == names and k > 50
    assert_equals_loop(res, loop_masks(ren, rt, cam, names), names)
    assert bool(res.masks[3].any()) and not torch.equal(bits(res.masks[3]), bits(res.masks[1]))
    assert int(e.selection("sphere1").sum()) == k == int(e.selection("sphere1_copy").sum())
    # the copy is an object of its own: taken out alone (no row of it is accepted any more), every other object's mask is what it was before the copy existed
    e.edits["sphere1_copy"].removed = True
    alone = query(ed, rt, cam)
    assert not alone.masks[3].any() and not ((alone.hit >> 3) & 1).any()
    assert torch.equal(bits(alone.masks[:3]), bits(before.masks))


# ---------------------------------------------------------------- 5: against the CPU oracle

def test_masks_against_the_cpu_oracle(ren, ed, syn, orc):
    """The oracle renders each indicator (jitter off, primary step only); the masks are held to the strict-parity bar of an output buffer (> 90 dB and at
    most 2 pixels at or over 2e-4)."""
    g, boxes, cam, e, rt = editable(ren, ed, syn)
    camd = syn.default_camera()
    o = orc.Oracle(W, H)
    o.set_camera(camd["origin"], camd["c2w"], camd["fov"], camd.get("znear", 0.01), camd.get("zfar", 999.9))
    o.set_config(jitter_primary_rays=0, num_bounces=0, **hc.LOSS_WEIGHTS)
    res = query(ed, rt, cam)
    got = res.masks.cpu().numpy()
    worst = {}
    for j, name in enumerate(SPHERES):
        ind = e.selection(name).cpu().numpy().astype(np.float32)
        o.set_gaussians(dict(g, rgb=np.repeat(ind[:, None], 3, axis=1)))
        o.update_bvh()
        ref = o.raytrace(False)["output_rgb"][0][..., 0]
        err = np.abs(got[j] - ref)
        worst[name] = (int((err >= 2e-4).sum()), round(hc.psnr(got[j], ref), 1), float(err.max()))
        assert float(np.abs(ref).max()) > 0.5
    hc.report("object_masks_vs_oracle", **{k: v for k, v in worst.items()})
    for name, (over, db, _) in worst.items():
        assert over <= 2 and db > 90.0, (name, worst[name])


# ---------------------------------------------------------------- 6, 7: the C ABI through ctypes on raw device pointers; refusals

def raw_twin(rt, cam):
    """A RawRaytracer (ctypes, no shim) on plain device buffers that hold what the shim tracer `rt` holds: the native gaussian tensors, the config, the framebuffer,
    metadata and statistics; its bound camera is set to `cam`."""
    cabi = importlib.import_module(PKG + ".c_abi")
    m = rt.cuda_module
    gs, cfg, fb, md, st = m.get_gaussians(), m.get_config(), m.get_framebuffer(), m.get_metadata(), m.get_stats()
    T = {k: getattr(gs, k).detach().clone().contiguous() for k in cabi.GAUSSIAN_PARAMS}
    n = T["mean"].shape[0]
    widths = dict(dL_drgb=3, dL_dnormal=3, dL_df0=3, dL_droughness=1, dL_dopacity=1, dL_dscale=3, dL_dmean=3, dL_drotation=4, total_weight=1)
    T.update({k: torch.zeros((n, c), dtype=torch.float32, device="cuda") for k, c in widths.items()})
    for names, holder in ((cabi.CONFIG_FIELDS, cfg), (cabi.FRAMEBUFFER_FIELDS, fb), (cabi.METADATA_FIELDS, md), (cabi.STATS_FIELDS, st)):
        T.update({k: getattr(holder, k).detach().clone().contiguous() for k in names})
    T.update(origin=torch.zeros(3, device="cuda"), rotation_c2w=torch.eye(3, device="cuda"), rotation_w2c=torch.eye(3, device="cuda"),
             vertical_fov_radians=torch.zeros(1, device="cuda"), znear=torch.zeros(1, device="cuda"), zfar=torch.zeros(1, device="cuda"))
    torch.cuda.synchronize()
    raw = cabi.RawRaytracer(W, H, n, {k: v.data_ptr() for k, v in T.items()}, ppll_forward_size=8_000_000, ppll_backward_size=1_000_000,
                            device=torch.cuda.current_device(), stream=torch.cuda.current_stream().cuda_stream)
    R, centre = cam.R.to("cuda", torch.float32).contiguous(), cam.camera_center.to("cuda", torch.float32).contiguous()
    raw._check(raw.L.egr_set_camera_from_dataset(raw.ctx, R.data_ptr(), centre.data_ptr(), float(cam.FoVy), 0.01, 999.9, raw.stream))
    torch.cuda.synchronize()
    return raw, T


def raw_query(raw, cam, row_bits, bit_list, masks, hit, top):
    R = cam.R.to("cuda", torch.float32).contiguous()
    centre = cam.camera_center.to("cuda", torch.float32).contiguous()
    fov = torch.tensor([float(cam.FoVy)], dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    raw.object_masks(R.data_ptr(), centre.data_ptr(), fov.data_ptr(), row_bits.data_ptr(), bit_list, masks.data_ptr(), None if hit is None else hit.data_ptr(),
                     None if top is None else top.data_ptr())
    torch.cuda.synchronize()


def test_c_abi_through_ctypes_equals_the_shim_bit_for_bit(ren, ed, syn):
    g, boxes, cam, e, rt = editable(ren, ed, syn, jitter=True)
    names = ["sphere2", "everything", "sphere0"]
    res = query(ed, rt, cam, names)
    raw, T = raw_twin(rt, cam)
    try:
        assert raw.L.egr_debug_check_bvh(raw.ctx, raw.stream) == 0
        T["total_num_calls"].fill_(4)
        masks = torch.full((3, H, W), 7.0, dtype=torch.float32, device="cuda")
        hit, top = torch.full((H, W), 7, dtype=torch.int32, device="cuda"), torch.full((H, W), 7, dtype=torch.int32, device="cuda")
        raw_query(raw, cam, e.selection_mask, [e.bits[nm] for nm in names], masks, hit, top)
        assert torch.equal(bits(masks), bits(res.masks)) and torch.equal(hit, res.hit) and torch.equal(top, res.top)
        assert int(T["total_num_calls"]) == 4 and raw.counters().status == 0 and raw.counters().rays[0] == W * H and raw.counters().rays[1] == 0
        # hit and top are optional
        only = torch.zeros((3, H, W), dtype=torch.float32, device="cuda")
        raw_query(raw, cam, e.selection_mask, [e.bits[nm] for nm in names], only, None, None)
        assert torch.equal(bits(only), bits(res.masks))
    finally:
        raw.close()


def test_refusals_touch_nothing(ren, ed, syn):
    g, boxes, cam, e, rt = editable(ren, ed, syn)
    m = rt.cuda_module
    # through the shim: a bit given twice, a bit >= 32, no bits, too many bits
    R, centre = cam.R, cam.camera_center
    for bad in ([1, 1], [0, 32], [], list(range(32)) + [0]):
        with pytest.raises(RuntimeError) as err:
            m.object_masks(R, centre, float(cam.FoVy), 0.01, 999.9, e.selection_mask, bad)
        assert len(str(err.value)) > 20, bad
    want = loop_masks(ren, rt, cam, SPHERES)
    assert_equals_loop(query(ed, rt, cam), want, SPHERES)  # the tracer still answers
    # through ctypes, with pre-filled outputs
    raw, T = raw_twin(rt, cam)
    try:
        masks = torch.full((2, H, W), 7.0, dtype=torch.float32, device="cuda")
        hit, top = torch.full((H, W), 7, dtype=torch.int32, device="cuda"), torch.full((H, W), 7, dtype=torch.int32, device="cuda")
        before = {k: v.clone() for k, v in T.items()}

        def refused(bit_list, needle):
            with pytest.raises(RuntimeError) as err:
                raw_query(raw, cam, e.selection_mask, bit_list, masks, hit, top)
            assert needle in str(err.value) and "egr_object_masks" in str(err.value), str(err.value)
            assert bool((masks == 7.0).all()) and bool((hit == 7).all()) and bool((top == 7).all())
            assert all(same_bits(before[k], T[k]) for k in T)

        refused([2, 2], "twice")
        refused([0, 40], "< 32")
        refused([], "num_bits")
        assert raw.L.egr_set_exact_stats(raw.ctx, 1) == 0
        refused([0, 1], "exact-statistics")
        raw.update_bvh()  # (the exact-statistics tree)
        refused([0, 1], "exact-statistics")
        raw.raytrace(False)  # the tracer still renders afterwards
        torch.cuda.synchronize()
        assert float(T["output_rgb"].abs().max()) > 0 and raw.counters().status == 0
        assert raw.L.egr_set_exact_stats(raw.ctx, 0) == 0
        raw.update_bvh()
        T["total_num_calls"].fill_(4)
        raw_query(raw, cam, e.selection_mask, [0, 1], masks, hit, top)  # back on the product tree: answered
        assert torch.equal(bits(masks), bits(want[:2]))
    finally:
        raw.close()
    # the shim says the same about an exact-statistics tracer, and the tracer still renders
    m.set_exact_stats(True)
    with pytest.raises(RuntimeError) as err:
        ed.selection_masks(cam, rt)
    assert "exact-statistics" in str(err.value)
    with torch.no_grad():
        out = ren.render(cam, rt, targets_available=False, force_update_bvh=True)
    assert float(out.final.abs().max()) > 0
