"""The tree builder (csrc/bvh.hip) held to its CPU restatement (bvh_restatement.py, itself checked by test_bvh_restatement_host.py), stage by stage, through
the read-only export Raytracer.debug_tree() (egr_debug_get_tree): sorted Morton keys, the sort's permutation and its stability, Karras' links, the rows of
the SAH programme, the collapse (a cut of the binary tree per wide node, optimal within 3 delta), the 16-bit slot boxes (at most one cell beyond the
rounding) and the bounding spheres. check_bvh() asserts validity only - any conservative tree passes it and the image parity tests; these tests assert that
the tree is the RIGHT one. No ray is launched: every test builds (or refits) and reads."""
import math

import numpy as np
import pytest

import bvh_restatement as br
import drift_scenes as ds
from hip_common import ren, report  # noqa: F401

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

SIZES = [1, 2, 3, 8, 9, 64, 65, 255, 256, 257, 4096]  # the builder's block is 256 threads; 4096 leaves are 16 blocks, enough to land on every XCD
EPS = 2.0 ** -24


# ------------------------------------------------------------------------------------------------ clouds
def cloud_blob(syn, n):
    return syn.random_blob_scene(n, seed=n)


def cloud_room(syn, n):  # planar walls: long shared key prefixes
    return syn.make_scene(n, "trained", seed=n)


def cloud_same_mean(syn, n):  # every key equal, the boxes differ
    g = syn.random_blob_scene(n, seed=n + 1)
    g["mean"][:] = np.array([2.5, 0.25, -0.5], np.float32)
    return g


def cloud_two_clusters(syn, n):
    """Two clusters of 1e-4 extent, 100 apart on every axis: distinct positions with equal keys. The frame is ~112 wide on every axis, a key cell
    112 / 2^21 = 5.3e-5, so a cluster covers at most 3 cells per axis - at most 54 distinct keys however many gaussians."""
    g = syn.random_blob_scene(n, seed=n + 2)
    rng = np.random.default_rng(n)
    g["mean"] = (np.array([2.0, 0.0, 0.0]) + rng.uniform(-0.5e-4, 0.5e-4, (n, 3)) + 100.0 * (np.arange(n)[:, None] % 2)).astype(np.float32)
    return g


def cloud_unusable(syn, n):  # invisible gaussians and non-finite means keep their leaves
    g = syn.random_blob_scene(n, seed=n + 3)
    g["opacity"][::7] = -8.0
    for i, (axis, v) in zip(sorted({1 % n, n // 2, n - 1}), ((0, np.nan), (1, np.inf), (2, -np.inf))):
        g["mean"][i, axis] = v
    return g


CLOUDS = dict(blob=cloud_blob, room=cloud_room, same_mean=cloud_same_mean, two_clusters=cloud_two_clusters, unusable=cloud_unusable)


def identical_cloud(syn, n):
    g = syn.random_blob_scene(n, seed=3)
    return {k: np.ascontiguousarray(np.repeat(v[:1], n, axis=0)) for k, v in g.items()}


def make_tracer(ren, g):
    return ren.GaussianRaytracer(ren.GaussianParams(g), 16, 16, ppll_forward_size=1_000_000, ppll_backward_size=1_000_000)


# ------------------------------------------------------------------------------------------------ the export
def export(rt):
    m = rt.cuda_module
    frame, info = m.debug_bvh_state()
    keys, gop, pog, left, right, dp, wn, bsph, ls = m.debug_tree()
    u32 = lambda t: t.numpy().view(np.uint32).astype(np.int64)
    return dict(frame=frame.numpy().copy(), info=[int(x) for x in info], keys=keys.numpy().view(np.uint64).copy(), gop=u32(gop), pog=u32(pog),
                left=left.numpy().astype(np.int64), right=right.numpy().astype(np.int64), dp=dp.numpy().copy(), wnodes=wn.numpy().view(np.uint32).copy(),
                bsph=bsph.numpy().copy(), level_start=u32(ls), aabb=m.debug_instances()[2].numpy().copy(),
                mean=m.get_gaussians().mean.cpu().numpy().copy())


def same_tree(a, b, links=True):
    """The parts of two exports a refit must leave alone: bit-identical. (`links` off: two builds number the nodes inside a level in arrival order.)"""
    for k in ("keys", "gop", "pog", "left", "right", "level_start", "frame"):
        assert np.array_equal(a[k], b[k]), k
    assert not links or np.array_equal(a["wnodes"][..., 3], b["wnodes"][..., 3])
    assert a["info"][1:] == b["info"][1:]


# ------------------------------------------------------------------------------------------------ checks 1 - 4
def check_order(e, name):
    """1. The exported keys are the sorted restated keys bit for bit; gid_of_pos is a permutation that sorts them, ascending by gaussian id among equal keys
    (a stable sort: what makes a rebuild reproducible); pos_of_gid is its inverse."""
    n = e["info"][3]
    ref = br.morton_keys(e["mean"], e["frame"])
    assert e["keys"].shape == (n,) and ref.shape == (n,)
    wrong = int(np.count_nonzero(e["keys"] != np.sort(ref)))
    report(name + "_order", n=n, key_mismatches=wrong, distinct_keys=len(np.unique(ref)))
    assert wrong == 0
    assert np.array_equal(np.sort(e["gop"]), np.arange(n))
    assert np.array_equal(ref[e["gop"]], e["keys"])
    assert np.all((e["keys"][1:] != e["keys"][:-1]) | (e["gop"][1:] > e["gop"][:-1]))
    assert np.array_equal(e["pog"][e["gop"]], np.arange(n))


def check_topology(e):
    """2. The exported links are Karras' over the exported keys, exactly. Returns (first, last) of the binary nodes."""
    left, right, first, last = br.karras(e["keys"])
    assert np.array_equal(e["left"], left) and np.array_equal(e["right"], right)
    return first, last


def check_rows(e, name):
    """3. Boxes: min and max are exact in fp32, so every exported node box equals the fp64 union of the GPU's own leaf boxes. Rows: every T is a sum of
    non-negative areas; an area carries at most 5 roundings (three differences, three products and two sums, of which a sum of non-negative terms keeps the
    larger relative error of its terms and adds one), every level of the tree adds two (T(left, k) + T(right, j - k), then area + D), a minimum of
    approximations approximates the minimum as well as they do, and a contracted multiply-add only removes a rounding:
        |T^ - T| <= delta * T,  delta = (5 + 2 h) * 2^-24,  h = height of the binary tree.
    Returns (area, T, delta)."""
    nb = len(e["left"])
    box, area, T, h = br.sah_rows(e["left"], e["right"], e["aabb"][e["gop"]])
    delta = (5 + 2 * h) * EPS
    assert e["dp"].shape == (nb, 16)
    assert np.array_equal(e["dp"][:, :6].astype(np.float64), box)
    That, Tref = e["dp"][:, 6:13].astype(np.float64), T[:, 1:]
    assert np.all(That[Tref == 0] == 0)
    pos = Tref > 0
    ratio = float((np.abs(That - Tref)[pos] / (delta * Tref[pos])).max()) if pos.any() else 0.0
    report(name + "_rows", height=h, delta=f"{delta:.2e}", worst_T_error_over_bound=f"{ratio:.3f}")
    assert ratio <= 1.0
    return area, T, delta


def check_collapse(e, first, last, area, T, delta, name):
    """4. Every wide node stands for a binary node and its used slots are a cut below it: they partition the node's leaf range, in ascending order, into
    ranges of binary nodes or single leaves. Levels and counts agree with the export. Optimality: the cost C of the exported tree (fp64 areas of its
    nodes) against the programme's optimum T(root, 1): the tree's fp32-evaluated cost IS T^(root, 1) (the replay reuses the stored rows), which is within
    delta of both C and T(root, 1), so C <= T (1 + delta) / (1 - delta) <= T (1 + 3 delta); and no tree costs less than the optimum (C and T are
    fp64 sums of the same <= 4095 areas in two orders: 1e-12 covers their own rounding)."""
    n, nw = e["info"][3], e["info"][1]
    ls = e["level_start"]
    nodes = br.wide_tree_from_links(e["wnodes"], n)
    assert e["wnodes"].shape == (nw, 8, 4) and len(nodes) == nw
    assert ls[0] == 0 and ls[-1] == nw and np.all(np.diff(ls) > 0) and e["info"][2] == len(ls) - 1 == max(nd["depth"] for nd in nodes.values()) + 1
    binary = {(int(a), int(b)): i for i, (a, b) in enumerate(zip(first, last))} if n > 1 else {}
    assert nodes[0]["range"] == (0, n - 1) and nodes[0]["leaves"] == n
    cost = 0.0
    for w, nd in nodes.items():
        assert ls[nd["depth"]] <= w < ls[nd["depth"] + 1], (w, nd["depth"])
        assert [s[0] for s in nd["slots"]] == list(range(len(nd["slots"])))  # no used slot after an empty one
        at = nd["range"][0]
        for _, a, b, leaves, link in nd["slots"]:
            assert a == at and leaves == b - a + 1, (w, a, b, leaves)
            assert (a == b) if link & br.LEAF_FLAG else ((a, b) in binary), (w, a, b)
            at = b + 1
        assert at == nd["range"][1] + 1
        if n > 1:
            assert nd["range"] in binary and len(nd["slots"]) >= 2, (w, nd["range"])
            cost += area[binary[nd["range"]]]
    if n > 1:
        opt = float(T[0, 1])
        report(name + "_collapse", wide_nodes=nw, levels=np.diff(ls).tolist(), C_over_T_minus_1=f"{(cost / opt - 1.0) if opt > 0 else 0.0:.2e}",
               three_delta=f"{3 * delta:.2e}")
        assert opt * (1.0 - 1e-12) <= cost <= opt * (1.0 + 3.0 * delta), (cost, opt)
    else:
        report(name + "_collapse", wide_nodes=nw, levels=np.diff(ls).tolist())
        assert nw == 1 and [s[4] for s in nodes[0]["slots"]] == [br.LEAF_FLAG]
    return nodes


def check_build(e, name):
    check_order(e, name)
    if e["info"][3] > 1:
        first, last = check_topology(e)
        area, T, delta = check_rows(e, name)
    else:
        assert e["left"].size == 0 and e["right"].size == 0 and e["dp"].size == 0
        first = last = area = T = delta = None
    return check_collapse(e, first, last, area, T, delta, name)


# ------------------------------------------------------------------------------------------------ check 6
def leaf_cells(e):
    """(low cells [m,3], high cells [m,3], boxes [m,6] fp32) of the leaf slots whose box is usable and inside the frame, after the assertions every tree
    owes: an unusable gaussian keeps the empty slot box (lo 65535, hi 0). Also returns the mask `all usable boxes are inside`."""
    lo, hi, link = br.unpack_slots(e["wnodes"])
    w, k = np.nonzero((link != br.EMPTY_SLOT) & ((link & br.LEAF_FLAG) != 0))
    box = e["aabb"][e["gop"][link[w, k] & ~br.LEAF_FLAG]]
    usable = box[:, 0] <= box[:, 3]
    assert len(w) == e["info"][3]
    assert np.all(lo[w, k][~usable] == 65535) and np.all(hi[w, k][~usable] == 0)
    inside = usable & ~ds.out_of_frame_mask(box, e["frame"])[0]
    return lo[w, k][inside], hi[w, k][inside], box[inside], bool(np.array_equal(inside, usable))


def cell_offsets(e):
    """6, the figures: low cell - floor(u) and high cell - ceil(u) per leaf slot and axis, u = (x - o) * s + 2 in fp64 for the low (high) side x of the box."""
    lo, hi, box, _ = leaf_cells(e)
    o, s = e["frame"][:3].astype(np.float64), e["frame"][3:].astype(np.float64)
    b = box.astype(np.float64)
    return lo - np.floor((b[:, :3] - o) * s + 2.0).astype(np.int64), hi - np.ceil((b[:, 3:] - o) * s + 2.0).astype(np.int64)


def histogram(d):
    return {int(v): int((d == v).sum()) for v in np.unique(d)}


def check_cells(e, name, fresh):
    """6. u = (x - o) * s + 2 in fp64 for the low (high) side x of a leaf's box: the stored low cell is floor(u) - 1 or floor(u) - 2, the high cell
    ceil(u) + 1 or ceil(u) + 2 - one cell beyond the rounding, and at most one more for the rounding of the kernel's own fp32 u (three roundings of half
    an ulp at 65535, 1.5 * 2^-8 cells). quant_lo / quant_hi take their floor (ceiling) 2^-6 cells further out for that reason: every integer is an fp32
    number, so an fp32 u just below one rounds ONTO it, and a plain floorf(u) - 1 gave floor(u) for 0.15 % of the low cells (measured on the kernel as it
    was: 8 - 22 of 12288 at n = 4096), one cell
    inside this bound. `fresh` (a build): no box carries a sentinel, and the root's box lies within cells [1, 65534]; after a refit only the boxes still
    inside the frame are held to the cells."""
    _, _, _, all_inside = leaf_cells(e)
    if fresh:
        assert e["info"][0] == 0 and all_inside
    d_lo, d_hi = cell_offsets(e)
    report(name + "_cells", leaf_slots=len(d_lo), low_cell_minus_floor=histogram(d_lo), high_cell_minus_ceil=histogram(d_hi))
    assert np.all((d_lo == -1) | (d_lo == -2)), histogram(d_lo)
    assert np.all((d_hi == 1) | (d_hi == 2)), histogram(d_hi)
    if fresh and len(d_lo):
        l3, h3, link = br.unpack_slots(e["wnodes"][:1])
        filled = (link[0] != br.EMPTY_SLOT) & (l3[0, :, 0] <= h3[0, :, 0])
        assert l3[0][filled].min() >= 1 and h3[0][filled].max() <= 65534


# ------------------------------------------------------------------------------------------------ check 8
def oracle_instances(orc, g):
    """(M [n,3,4], cube boxes [n,6], visible [n]) of an fp64 oracle fed the cloud; non-finite means (never usable) are fed as zeros."""
    o = orc.Oracle(16, 16, double=True)
    o.set_gaussians(dict(g, mean=np.where(np.isfinite(g["mean"]), g["mean"], np.float32(0.0)).astype(np.float32)))
    o.update_bvh()
    M, _, Ao, vis = o.instances()
    return M.astype(np.float64), Ao, vis.astype(bool) & np.all(np.isfinite(g["mean"]), axis=1)


def check_spheres(e, orc, g, name, exact=False):
    """8. bsph in record order: the centre is the mean bit for bit and r^2 <= w <= (1.0001 r + 4e-7 (|m|_1 + r))^2 (1 + 8 * 2^-24), r the ellipsoid's largest
    semi-axis (the largest column norm of the oracle's fp64 M), in exact-statistics mode the cube's half diagonal; an unusable gaussian has w < 0."""
    M, Ao, vis = oracle_instances(orc, g)
    usable = e["aabb"][:, 0] <= e["aabb"][:, 3]
    assert np.array_equal(usable, vis)
    sph = e["bsph"][e["pog"]]  # by gaussian id
    assert np.all(sph[~usable, 3] < 0)
    col = np.sqrt((M[:, :, :3] ** 2).sum(axis=1))  # [n,3] column norms
    r = np.sqrt((col ** 2).sum(axis=1)) if exact else col.max(axis=1)
    mean = e["mean"]
    assert np.array_equal(sph[usable, :3].view(np.uint32), mean[usable].view(np.uint32))
    w = sph[:, 3].astype(np.float64)
    r = np.where(usable, r, 1.0)
    upper = (1.0001 * r + 4e-7 * (np.abs(np.where(usable[:, None], mean, 0.0).astype(np.float64)).sum(axis=1) + r)) ** 2 * (1.0 + 8 * EPS)
    if usable.any():
        report(name + "_spheres", usable=int(usable.sum()), least_w_over_r2=f"{(w / r ** 2)[usable].min():.8f}", worst_w_over_upper=f"{(w / upper)[usable].max():.8f}",
               above_upper=int((w > upper)[usable].sum()))
    assert np.all(r[usable] ** 2 <= w[usable])
    assert np.all(w[usable] <= upper[usable])
    return M, Ao, usable


# ------------------------------------------------------------------------------------------------ the tests
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("cloud", list(CLOUDS))
def test_build_equals_the_restatement(ren, syn, cloud, n):
    """Checks 1 - 4 and 6."""
    g = CLOUDS[cloud](syn, n)
    rt = make_tracer(ren, g)
    assert rt.cuda_module.check_bvh() == 0, rt.cuda_module.last_error()
    e = export(rt)
    assert e["info"][3] == n and np.array_equal(e["mean"].view(np.uint32), g["mean"].view(np.uint32))
    name = f"{cloud}_{n}"
    check_build(e, name)
    check_cells(e, name, fresh=True)
    if cloud == "same_mean":  # the clouds are what they are meant to be
        assert len(np.unique(e["keys"])) == 1
    if cloud == "two_clusters":
        assert len(np.unique(e["keys"])) <= min(n, 54) and len(np.unique(g["mean"][::2], axis=0)) == (n + 1) // 2  # (the cluster at the origin's side)
    if cloud == "unusable":
        assert int((e["aabb"][:, 0] > e["aabb"][:, 3]).sum()) >= (n + 6) // 7


@pytest.mark.parametrize("cloud", list(CLOUDS))
def test_bounding_spheres(ren, orc, syn, cloud):
    for n in SIZES:
        g = CLOUDS[cloud](syn, n)
        check_spheres(export(make_tracer(ren, g)), orc, g, f"{cloud}_{n}")


@pytest.mark.parametrize("n", [64, 100, 512])
def test_identical_gaussians_give_the_flattest_tree(ren, syn, n):
    """Equal keys and equal boxes: every wide node costs the same, so the optimum has the fewest nodes, ceil((n - 1) / 7)."""
    rt = make_tracer(ren, identical_cloud(syn, n))
    e = export(rt)
    assert len(np.unique(e["keys"])) == 1 and np.all(e["aabb"] == e["aabb"][0]) and e["aabb"][0, 0] < e["aabb"][0, 3]
    check_build(e, f"identical_{n}")
    report(f"identical_{n}", wide_nodes=e["info"][1], levels=np.diff(e["level_start"]).tolist())
    assert e["info"][1] == math.ceil((n - 1) / 7)
    assert np.array_equal(e["gop"], np.arange(n))  # stable: the order of coincident gaussians is their id order


def test_rebuild_reads_no_stale_rows(ren, syn):
    """5. The programme's rows are never cleared between builds, and the second arrival at a node reads rows another XCD wrote: a stale read would pick up
    the previous cloud's values, here smaller by 9 times and more."""
    n = 4096
    rt = make_tracer(ren, cloud_blob(syn, n))
    first_rows = export(rt)["dp"][:, 6:13].copy()
    with torch.no_grad():
        rt.pc._xyz.mul_(3.0)
        rt.pc._scaling.add_(1.0)
    rt.rebuild_bvh()
    assert rt.cuda_module.check_bvh() == 0
    e = export(rt)
    nodes = check_build(e, "second_build")
    ratio = float(e["dp"][0, 6]) / float(first_rows[0, 0])
    report("second_build_vs_first", root_row_ratio=f"{ratio:.2f}")
    assert ratio > 5.0  # the two builds' rows really differ
    rt.rebuild_bvh()
    e3 = export(rt)
    same_tree(e, e3, links=False)
    assert np.array_equal(e3["dp"][:, :13], e["dp"][:, :13])
    assert br.canonical_form(br.wide_tree_from_links(e3["wnodes"], n)) == br.canonical_form(nodes)  # node numbering inside a level may differ


def refitted(rt, n):
    """Moves every mean by N(0, 0.01) and refits; returns the export."""
    with torch.no_grad():
        rt.pc._xyz.add_(0.01 * torch.randn(rt.pc._xyz.shape, generator=torch.Generator().manual_seed(n)).to(rt.pc._xyz.device))
        rt._export_param_values()
    rt.cuda_module.update_bvh()
    torch.cuda.synchronize()
    assert rt.cuda_module.check_bvh() == 0, rt.cuda_module.last_error()
    return export(rt)


@pytest.mark.parametrize("n", [65, 4096])
@pytest.mark.parametrize("cloud", list(CLOUDS))
def test_refit_keeps_the_topology(ren, syn, cloud, n):
    """7. update_bvh() after the means moved: keys, permutation, links and levels stay bit for bit, the boxes follow."""
    rt = make_tracer(ren, CLOUDS[cloud](syn, n))
    e = export(rt)
    e2 = refitted(rt, n)
    same_tree(e, e2)
    assert not np.array_equal(e2["aabb"], e["aabb"])
    check_cells(e2, f"refit_{cloud}_{n}", fresh=False)


def test_exact_statistics_spheres_and_boxes(ren, orc, syn):
    """8, exact-statistics mode (set_exact_stats(True), then a rebuild): the sphere's r is the cube's half diagonal, and the exported box contains the
    oracle's cube box and is wider on each side by at most the kernel's padding, 1e-4 ext + 4e-7 (|m| + ext), plus four ulps of the coordinate."""
    n = 500
    g = cloud_unusable(syn, n)
    rt = make_tracer(ren, g)
    rt.cuda_module.set_exact_stats(True)
    rt.rebuild_bvh()
    assert rt.cuda_module.check_bvh() == 0
    e = export(rt)
    check_build(e, "exact_stats")
    check_cells(e, "exact_stats", fresh=True)
    M, Ao, usable = oracle_instances(orc, g)
    assert np.array_equal(usable, e["aabb"][:, 0] <= e["aabb"][:, 3])
    A = e["aabb"].astype(np.float64)[usable]
    Ao, m = Ao[usable], e["mean"].astype(np.float64)[usable]
    ext = np.abs(M[usable][:, :, :3]).sum(axis=2)  # the cube's half extent per axis: |row of M|_1
    pad = 1e-4 * ext + 4e-7 * (np.abs(m) + ext) + 4 * np.spacing(np.abs(e["aabb"][usable]).reshape(-1, 2, 3).max(axis=1)).astype(np.float64)
    over = np.maximum((Ao[:, :3] - A[:, :3]) / pad, (A[:, 3:] - Ao[:, 3:]) / pad)
    report("exact_stats_boxes", usable=int(usable.sum()), worst_width_over_padding=f"{over.max():.4f}", least=f"{over.min():.4f}")
    assert np.all(A[:, :3] <= Ao[:, :3]) and np.all(A[:, 3:] >= Ao[:, 3:])
    assert over.max() <= 1.0
    check_spheres(e, orc, g, "exact_stats", exact=True)
