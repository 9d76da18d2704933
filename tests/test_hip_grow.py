"""Growing the cloud on the GPU (csrc/grow.hip; torch.ops.egr.grow_sample / grow_append; trainer.farfield_candidates, FusedTrainStep.grow_and_rebuild and
add_farfield_points): the candidates against the numpy restatement of their generator (grow_restatement.py), the camera filter on them against a restatement of
scene.select_points_to_prune_near_cameras, the append against torch.cat bit for bit, and the one-call growth step against today's three-call sequence."""
import ctypes as C
import importlib

import numpy as np
import pytest

import grow_restatement as gr
import hip_common as hc
from hip_common import ren  # noqa: F401

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu
PKG = "editable-gaussian-reflections_amd"
SIZES = (1, 63, 64, 65, 255, 256, 257, 4097)
SEEDS = (0, 750, 2 ** 63 + 5)  # (the last one uses the high key word)
RADII = (1.0, 2.5)


@pytest.fixture(scope="module")
def tr():
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU fallback")
    return importlib.import_module(PKG + ".trainer")


def ordered(x):
    """fp32 array -> int64 whose differences count representable values between two floats (both zeros map to 0)."""
    i = np.ascontiguousarray(x, np.float32).view(np.int32).astype(np.int64)
    return np.where(i < 0, -(i & 0x7FFFFFFF), i)


def bits(t):
    return t.contiguous().view(torch.int32)


def test_candidates_match_the_restatement_to_one_ulp(tr):
    """Both sides evaluate Box-Muller in fp64 and round to fp32 once. The smallest non-zero |cos| or |sin| on the 2^-23 grid of u is about 3.7e-7, so fp64
    library differences stay near 1e-9 relative: they can move a result across ONE fp32 rounding boundary at the most. The bound is this derivation, not a
    measurement; the number of coordinates that are not bit-equal is printed."""
    unequal = total = 0
    for seed in SEEDS:
        for radius in RADII:
            for n in SIZES:
                got = tr.farfield_candidates(n, seed, radius)
                assert got.dtype == torch.float32 and got.shape == (n, 3) and got.is_cuda and got.is_contiguous()
                got, want = got.cpu().numpy(), gr.candidates(0, n, seed, radius)
                distance = np.abs(ordered(got) - ordered(want))
                assert distance.max() <= 1, (seed, radius, n, int(distance.max()), got[distance > 1][:4], want[distance > 1][:4])
                unequal += int((distance != 0).sum())
                total += distance.size
    print(f"grow_sample vs numpy restatement: {unequal} of {total} coordinates not bit-equal (all within 1 ulp)")


def test_candidates_clamp_chunking_word_boundary_and_repeatability(tr):
    n, seed = 4097, 750
    z = gr.normals(0, n, seed)
    clamped = np.abs(z) > 3.0
    assert int(clamped.sum()) == 27  # (the restatement clamps 27 coordinates of this draw)
    for radius in RADII:
        got = tr.farfield_candidates(n, seed, radius).cpu().numpy()
        limit = np.float32(3.0) * np.float32(radius)
        assert clamped.any() and np.array_equal(got[clamped], np.sign(z[clamped]) * limit)  # exactly +-3 * radius
        assert float(np.abs(got).max()) == float(limit) and int((np.abs(got) == limit).sum()) >= 27
    narrow = tr.farfield_candidates(n, seed, 1.0, clamp=0.5).cpu().numpy()
    assert float(np.abs(narrow).max()) == 0.5 and np.abs(ordered(narrow) - ordered(gr.candidates(0, n, seed, 1.0, 0.5))).max() <= 1  # (another clamp)
    # a call split at any row gives the same rows
    whole = tr.farfield_candidates(257, seed, 2.5)
    parts = torch.cat([tr.farfield_candidates(100, seed, 2.5, first=0), tr.farfield_candidates(157, seed, 2.5, first=100)])
    assert torch.equal(bits(whole), bits(parts))
    # across the word boundary of the counter, and with the high counter word in use
    for first in (2 ** 32 - 3, 2 ** 63 + 2 ** 32 - 3):
        got = tr.farfield_candidates(8, seed, 1.0, first=first).cpu().numpy()
        assert np.abs(ordered(got) - ordered(gr.candidates(first, 8, seed, 1.0))).max() <= 1
    assert not torch.equal(tr.farfield_candidates(8, seed, 1.0, first=2 ** 32), tr.farfield_candidates(8, seed, 1.0, first=0))  # (the high counter word counts)
    # other seeds and other rows are other points; the same arguments are the same bits
    assert not torch.equal(tr.farfield_candidates(64, 1, 1.0), tr.farfield_candidates(64, 2, 1.0))
    assert not torch.equal(tr.farfield_candidates(64, 1, 1.0), tr.farfield_candidates(64, 1 + 2 ** 32, 1.0))
    assert torch.equal(bits(tr.farfield_candidates(n, 2 ** 63 + 5, 2.5)), bits(tr.farfield_candidates(n, 2 ** 63 + 5, 2.5)))
    # empty, and what the op refuses
    assert tr.farfield_candidates(0, seed, 1.0).shape == (0, 3)
    for bad in (dict(n=-1), dict(n=2 ** 26 + 1), dict(radius=float("nan")), dict(radius=-1.0), dict(clamp=-1.0), dict(clamp=float("inf")), dict(first=2 ** 64 - 1, n=2),
                dict(device="cpu")):
        kw = dict(n=16, seed=1, radius=1.0)
        kw.update(bad)
        with pytest.raises(RuntimeError):
            tr.farfield_candidates(**kw)


def near_cameras_torch(points, centers, znear):
    """scene/scene.py:88-105 select_points_to_prune_near_cameras with stock torch calls, one camera at a time."""
    prune = torch.zeros(points.shape[0], dtype=torch.bool, device=points.device)
    for c in range(centers.shape[0]):
        prune |= (points - centers[c]).norm(dim=1) < znear[c]
    return prune


FILTER_N = 4097


@pytest.fixture(scope="module")
def recipe(tr):
    """The filter test's recipe, computed once: 7 cameras of default_rng(41), and the first seed of 750 .. 757 whose 4097 device candidates (radius 1) keep a
    distance of 1e-5 * znear from the surface of every sphere (fp64 on the read-back) - the band test_hip_prune.py uses, inside which an fp32 norm may decide
    either way."""
    rng = np.random.default_rng(41)
    centers = rng.uniform(-1.0, 1.0, (7, 3)).astype(np.float32)
    znear = rng.uniform(0.3, 0.8, 7).astype(np.float32)
    found = None
    for seed in range(750, 758):
        cand = tr.farfield_candidates(FILTER_N, seed, 1.0)
        dist = np.linalg.norm(cand.cpu().numpy().astype(np.float64)[:, None, :] - centers.astype(np.float64)[None], axis=2)
        if not np.any(np.abs(dist - znear[None]) < 1e-5 * znear[None]):
            found = seed
            break
    assert found is not None, "every seed of 750 .. 757 puts a candidate within 1e-5 * znear of a sphere"
    inside = np.any(dist < znear[None], axis=1)
    return dict(seed=found, cand=cand, centers=torch.from_numpy(centers).cuda(), znear=torch.from_numpy(znear).cuda(), inside=inside, kept=cand[torch.from_numpy(~inside).cuda()])


def test_filter_on_the_candidates_equals_the_restated_predicate(tr, recipe):
    cand, centers, znear = recipe["cand"], recipe["centers"], recipe["znear"]
    remove = near_cameras_torch(cand, centers, znear)
    share = float(remove.sum()) / FILTER_N
    print(f"far-field filter: seed {recipe['seed']} removes {int(remove.sum())} of {FILTER_N} ({100 * share:.1f} %)")
    assert 0.05 <= share <= 0.60
    assert np.array_equal(remove.cpu().numpy(), recipe["inside"])  # (fp32 torch and fp64 numpy agree outside the band)
    kept = tr.filter_points_near_cameras(cand, centers, znear)
    assert torch.equal(bits(kept), bits(cand[~remove])) and kept.shape[0] == FILTER_N - int(remove.sum())


SPECIAL_BITS = (0x7FC00001, 0x7FA5A5A5, 0xFFC12345, 0x7F800001, 0x7F800000, 0xFF800000, 0x80000000, 0x00000001, 0x807FFFFF, 0x00400000, 0x3F800000, 0x00000000)


def special_rows(width, rows=12):
    """[rows <= 12, width] fp32 rows whose bits a float move could lose: NaNs with payloads (quiet and signalling patterns), +/-inf, -0.0, denormals."""
    b = np.array(SPECIAL_BITS[:rows], np.uint32).view(np.int32)
    return torch.from_numpy(np.repeat(b[:, None], width, axis=1)).cuda().view(torch.float32)


def with_specials(t):
    k = min(12, t.shape[0])
    if k:
        t[:k] = special_rows(t.shape[1], k)
        t[t.shape[0] - k:] = special_rows(t.shape[1], k)
    return t


def as_i32(word):
    return word - (1 << 32) if word >= 1 << 31 else word


APPEND_SHAPES = [(1, 1), (1000, 64), (1025, 1023), (3 * 1024 + 17, 4097), (0, 65)]


@pytest.mark.parametrize("n,m", APPEND_SHAPES)
def test_append_equals_torch_cat_bit_for_bit(tr, n, m):
    gen = torch.Generator(device="cuda").manual_seed(100 + n)
    src, tail, fill = [], [], []
    for width in (1, 3, 4):  # rows appended, with the special patterns at both ends of the old rows and of the tail
        src.append(with_specials(torch.randn((n, width), device="cuda", generator=gen)))
        tail.append(with_specials(torch.randn((m, width), device="cuda", generator=gen)))
        fill.append(0x12345678)  # (ignored where a tail is given)
    src.append(torch.randint(-2 ** 31, 2 ** 31 - 1, (n, 2), device="cuda", generator=gen, dtype=torch.int32))
    tail.append(torch.randint(-2 ** 31, 2 ** 31 - 1, (m, 2), device="cuda", generator=gen, dtype=torch.int32))
    fill.append(0)
    for word in (0, 0x80000000, 0x7FC00001):  # filled: zeros, -0.0, a NaN with a payload
        src.append(with_specials(torch.randn((n, 3), device="cuda", generator=gen)))
        tail.append(None)
        fill.append(word)
    src.append(torch.randint(-2 ** 31, 2 ** 31 - 1, (n,), device="cuda", generator=gen, dtype=torch.int32))  # 1-D int32, filled with -7
    tail.append(None)
    fill.append(-7)
    before = [t.clone() for t in src] + [t.clone() for t in tail if t is not None]
    out = torch.ops.egr.grow_append(src, tail, fill, m)
    assert len(out) == len(src)
    for t, a, f, o in zip(src, tail, fill, out):
        new = a if a is not None else torch.full((m,) + tuple(t.shape[1:]), as_i32(f & 0xFFFFFFFF), dtype=torch.int32, device="cuda").view(t.dtype)
        want = torch.cat([t, new], 0)
        assert o.dtype == t.dtype and o.shape == want.shape and o.is_contiguous()
        assert torch.equal(bits(o), bits(want)), (n, m, tuple(t.shape), f)
    after = src + [t for t in tail if t is not None]
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(after, before))  # the sources are unchanged
    if n:  # m == 0: a copy
        copy = torch.ops.egr.grow_append(src[:2], [None, None], [0, 0], 0)
        assert all(torch.equal(bits(o), bits(t)) and o.data_ptr() != t.data_ptr() for o, t in zip(copy, src))


def test_append_of_33_tensors_and_what_the_op_refuses(tr):
    n, m = 1025, 1023
    gen = torch.Generator(device="cuda").manual_seed(6)
    # 33 arrays: one more than a table of the C ABI holds (the shim splits the list)
    many = [torch.randn((n, 1 + k % 4), device="cuda", generator=gen) for k in range(33)]
    tails = [torch.randn((m, 1 + k % 4), device="cuda", generator=gen) if k % 3 else None for k in range(33)]
    words = [0x3F800000 + k for k in range(33)]
    out = torch.ops.egr.grow_append(many, tails, words, m)
    assert len(out) == 33
    for t, a, f, o in zip(many, tails, words, out):
        new = a if a is not None else torch.full((m, t.shape[1]), f, dtype=torch.int32, device="cuda").view(torch.float32)
        assert torch.equal(bits(o), bits(torch.cat([t, new], 0)))
    t3, a3 = many[2], tails[2]  # width 3, with a tail
    assert a3 is not None
    refused = [
        ([t3, many[1][: n - 1]], [a3, tails[1]], [0, 0], m),  # another leading size
        ([t3.double()], [a3.double()], [0], m),  # 8-byte elements
        ([many[3][:, :2]], [None], [0], m),  # not contiguous
        ([t3], [a3[: m - 1]], [0], m),  # a tail with other rows
        ([t3], [a3.to(torch.int32)], [0], m),  # a tail of another dtype
        ([t3], [many[3][:m]], [0], m),  # a tail of another width
        ([t3], [a3.cpu()], [0], m),  # a tail on the host
        ([t3], [a3, None], [0], m),  # lists of different lengths
        ([t3], [a3], [0, 0], m),
        ([t3], [None], [1 << 32], m),  # not a 32-bit word
        ([t3], [None], [0], -1),
        ([t3], [None], [0], 2 ** 26),  # n + m beyond the tree's limit
    ]
    for args in refused:
        with pytest.raises(RuntimeError, match="grow_append"):
            torch.ops.egr.grow_append(*args)


def test_overlapping_ranges_are_refused(tr):
    """The torch op allocates its outputs, so an overlap can only be asked for through the C ABI: refused with an error before anything is launched. (What the
    library refuses of an op's own arguments raises through the op: the radius, clamp and range cases of the candidate test.)"""
    cabi = importlib.import_module(PKG + ".c_abi")
    L = cabi.lib()
    n, m, w = 300, 100, 3
    buf = torch.arange(3 * (n + m) * w, dtype=torch.float32, device="cuda")
    before = buf.clone()
    torch.cuda.synchronize()
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    base, word = buf.data_ptr(), 4
    src, tail, free = base, base + n * w * word, base + (n + m) * w * word  # [src | tail | room for a dst and more]

    def call(dst, kind=cabi.EGR_GROW_TAIL_ROWS):
        table = (cabi.egr_grow_array * 1)(cabi.egr_grow_array(src=src, dst=dst, tail=tail, width=w, tail_kind=kind, fill_bits=0))
        return L.egr_grow_append(buf.get_device(), table, 1, n, m, stream)

    for dst in (src, src + word, src + (n * w - 1) * word):  # src == dst, shifted by one word, dst starting in the last word of src
        assert call(dst) != 0 and b"out of place" in L.egr_grow_last_error()
    assert call(tail) != 0 and b"overlaps a tail" in L.egr_grow_last_error()  # dst == tail (src ends where it starts)
    assert call(src - (n + m) * w * word + word) != 0 and b"out of place" in L.egr_grow_last_error()  # dst ending in the first word of src
    torch.cuda.synchronize()
    assert torch.equal(buf, before)
    # the adjacent range after the tail is fine, and equals the torch op
    assert call(free) == 0, L.egr_grow_last_error()
    torch.cuda.synchronize()
    old, new = before[: n * w].reshape(n, w), before[n * w : (n + m) * w].reshape(m, w)
    want = torch.ops.egr.grow_append([old], [new], [0], m)[0]
    assert torch.equal(buf[(n + m) * w : 2 * (n + m) * w].reshape(n + m, w), want) and torch.equal(buf[: (n + m) * w], before[: (n + m) * w])
    assert torch.equal(bits(want), bits(torch.cat([old, new])))
    # a dst that is not 16-byte aligned (the kernel then moves every word on its own): one word further on
    middle = buf.clone()
    assert free % 16 == 0 and call(free + word) == 0, L.egr_grow_last_error()
    torch.cuda.synchronize()
    assert torch.equal(buf[(n + m) * w + 1 : 2 * (n + m) * w + 1].reshape(n + m, w), want)
    assert torch.equal(buf[: (n + m) * w + 1], middle[: (n + m) * w + 1]) and torch.equal(buf[2 * (n + m) * w + 1 :], middle[2 * (n + m) * w + 1 :])  # nothing before it or past its end


def test_append_of_arrays_that_are_not_16_byte_aligned(tr):
    """The old rows go as 16-byte vectors only where src and dst are both 16-byte aligned: sources one, two and three words off such an address (and an aligned one
    for the vector path with 1, 2, 3 and 0 words left over) give torch.cat's bits all the same."""
    gen = torch.Generator(device="cuda").manual_seed(9)
    m = 77
    for n in (1025, 1026, 1027, 1028):
        for width in (1, 3):
            for off in (0, 1, 2, 3):
                room = torch.randn(off + n * width + 8, device="cuda", generator=gen)
                src = with_specials(room[off : off + n * width].view(n, width))
                assert src.is_contiguous() and src.data_ptr() % 16 == 4 * off
                tail_room = torch.randn(off + m * width, device="cuda", generator=gen)
                tail = tail_room[off:].view(m, width)
                filled, rows = torch.ops.egr.grow_append([src, src], [None, tail], [0x7FC00001, 0], m)
                assert torch.equal(bits(rows), bits(torch.cat([src, tail]))), (n, width, off)
                assert torch.equal(bits(filled[:n]), bits(src)) and bool((bits(filled[n:]) == 0x7FC00001).all()), (n, width, off)


LRS = dict(xyz=1.6e-4, normal=1e-3, roughness=2e-3, f0=2e-3, f_dc=2.5e-3, opacity=2.5e-2, scaling=5e-3, rotation=1e-3)
EYES = ((-1.7, -1.2, 0.4), (1.6, -1.3, 0.2), (0.0, 1.5, -0.5))  # the three views of test_hip_prune.py
LOOKS = ((1.2, 0.5, -0.9), (-1.5, 1.0, -0.5), (0.3, -1.8, 0.6))
GRAD_WIDTHS = (3, 3, 3, 1, 1, 3, 3, 4, 1)  # the tensor-major layout of grad_flat: eight gradients, then total_weight
N, W, H = 20000, 32, 32


def same_sums(a, b):
    """Two [22N] buffers of atomically summed gradients and weights of the same launches: equal to 1e-4 of the largest entry of each of the nine tensors (see
    test_hip_prune.py)."""
    n = a.numel() // 22
    lo = 0
    for width in GRAD_WIDTHS:
        x, y = a[lo * n : (lo + width) * n], b[lo * n : (lo + width) * n]
        assert float((x - y).abs().max()) <= 1e-4 * float(x.abs().max()), (lo, float((x - y).abs().max()), float(x.abs().max()))
        lo += width


def scene_cameras(ren, syn):
    tg = syn.make_targets(W, H)
    fov = syn.default_camera()["fov"]
    return [hc.cam_obj(ren, dict(origin=np.array(e, np.float32), c2w=syn.look_at(np.array(e, np.float64), l).astype(np.float32), fov=fov), tg) for e, l in zip(EYES, LOOKS)]


def make_side(ren, tr, g):
    pc = ren.GaussianParams(g)
    rt = ren.GaussianRaytracer(pc, W, H, team_help=False)
    rt.cuda_module.get_config().jitter_primary_rays.fill_(False)
    return pc, rt, tr.FusedTrainStep(pc, rt, LRS)


def state_of(tr, pc, step):
    return [getattr(pc, a) for _, a, _ in tr.GROUPS] + [step.exp_avg[n] for n, _, _ in tr.GROUPS] + [step.exp_avg_sq[n] for n, _, _ in tr.GROUPS]


def test_grow_and_rebuild_equals_todays_sequence(tr, ren, syn):
    ini = importlib.import_module(PKG + ".initialization")
    g = syn.make_scene(N, "trained", seed=4)
    cameras = scene_cameras(ren, syn)
    sides = [make_side(ren, tr, g) for _ in range(2)]
    for pc, rt, step in sides:  # moments, native gradients and total_weight are real
        for cam in cameras:
            ren.render(cam, rt)
            step.step()
        ren.render(cameras[0], rt)  # one more grad launch without a step: the native gradients are not zero when the cloud grows
    (pa, ra, sa), (pb, rb, sb) = sides
    ga, gb = ra.cuda_module.get_gaussians(), rb.cuda_module.get_gaussians()
    attrs = [attr for _, attr, _ in tr.GROUPS]
    # the two sides agree to the level of their float atomics; side B then takes side A's state bit for bit, so that what follows compares the two GROWTH paths
    same_sums(ga.grad_flat, gb.grad_flat)
    gb.grad_flat.copy_(ga.grad_flat)
    for name, attr, _ in tr.GROUPS:
        getattr(pb, attr).copy_(getattr(pa, attr))
        sb.exp_avg[name].copy_(sa.exp_avg[name]), sb.exp_avg_sq[name].copy_(sa.exp_avg_sq[name])
    assert sa.steps == sb.steps == 3
    assert float(ga.total_weight.max()) > 0.0 and float(ga.grad_flat[: 21 * N].abs().max()) > 0.0 and float(sa.exp_avg["xyz"].abs().max()) > 0.0
    old_flat = ga.grad_flat.clone()

    m = 1500
    points = tr.farfield_candidates(m, 7, 1.0)
    new = ini.gaussians_from_cloud(points, torch.full((m, 3), 0.2, device="cuda"), init_scale=0.1, init_opa=0.1, init_roughness=0.0, init_f0=0.04)
    new_host = {k: v.cpu().numpy() for k, v in new.items()}
    counter = torch.arange(N, dtype=torch.int32, device="cuda").reshape(N, 1) * 7 - 3
    weight = torch.rand((N,), device="cuda")

    # what is refused: ValueError, and nothing was touched
    objects = state_of(tr, pa, sa)
    copies = [t.clone() for t in objects] + [ga.grad_flat.clone()]
    edt = importlib.import_module(PKG + ".editing")
    edited = tr.FusedTrainStep.__new__(tr.FusedTrainStep)
    edited.__dict__.update(sa.__dict__)
    edited.pc = edt.EditableGaussians(pa, {}, selection_mask=torch.zeros(N, dtype=torch.int32, device="cuda"))
    assert hasattr(edited.pc, "export_edited")
    ragged = dict(new, scale=new["scale"][: m - 1])
    empty = {k: v[:0] for k, v in new.items()}
    for step, rows, extra in ((sa, empty, ()), (sa, ragged, ()), (sa, dict(new, rgb=new["rgb"].reshape(-1)[:-1]), ()), (edited, new, ()), (sa, new, [(counter[: N - 1], 0)]),
                              (sa, new, [(counter.double(), 0)])):
        with pytest.raises(ValueError):
            step.grow_and_rebuild(rows, extra=extra)
    with pytest.raises(ValueError):
        edited.add_farfield_points(100, 1.0, 1)
    now = state_of(tr, pa, sa)
    assert all(x is y for x, y in zip(objects, now)) and all(torch.equal(bits(x), bits(y)) for x, y in zip(now + [ga.grad_flat], copies))
    assert ra.cuda_module.get_gaussians().mean.shape[0] == N and sa.steps == 3

    # side A: the one call (GPU tensors); side B: today's sequence (host arrays, as append_points takes them)
    n_total, (counter_a, weight_a) = sa.grow_and_rebuild(new, extra=[(counter, 0), (weight, -0.0)])
    pb.append_points(new_host)
    sb.extend(m)
    rb.rebuild_bvh()
    counter_b = torch.cat([counter, torch.zeros((m, 1), dtype=torch.int32, device="cuda")])
    weight_b = torch.cat([weight, torch.full((m,), -0.0, device="cuda")])

    assert n_total == N + m and sa.steps == sb.steps == 3
    ga, gb = ra.cuda_module.get_gaussians(), rb.cuda_module.get_gaussians()
    for x, y in zip(state_of(tr, pa, sa), state_of(tr, pb, sb)):  # the 8 parameters and the 16 moments
        assert x.shape[0] == N + m and x.shape == y.shape and torch.equal(bits(x), bits(y))
    for name, _, _ in tr.GROUPS:
        assert float(sa.exp_avg[name][N:].abs().max()) == 0.0 and float(sa.exp_avg_sq[name][N:].abs().max()) == 0.0
    assert torch.equal(bits(pa._xyz[N:]), bits(points)) and torch.equal(bits(pa._scaling[N:]), bits(new["scale"]))
    assert counter_a.dtype == torch.int32 and torch.equal(counter_a, counter_b) and torch.equal(bits(weight_a), bits(weight_b)) and weight_a.shape == (N + m,)
    for attr in attrs:
        p = getattr(pa, attr)
        assert p.grad is not None and p.grad.shape == p.shape and p.grad.shape[0] == N + m and float(p.grad.abs().max()) == 0.0
    # the native gradients and total_weight: the whole buffer equal on both sides, old rows with their bits, new rows zero
    assert ga.grad_flat.numel() == 22 * (N + m) and torch.equal(bits(ga.grad_flat), bits(gb.grad_flat))
    lo = 0
    for width in GRAD_WIDTHS:
        seg = ga.grad_flat[lo * (N + m) : (lo + width) * (N + m)]
        assert torch.equal(bits(seg[: width * N]), bits(old_flat[lo * N : (lo + width) * N])) and float(seg[width * N :].abs().max()) == 0.0, lo
        lo += width
    assert float(ga.total_weight[:N].max()) > 0.0
    assert ga.mean.shape[0] == N + m and torch.equal(ga.mean, pa._xyz)
    assert ra.cuda_module.check_bvh() == 0, ra.cuda_module.last_error()
    finals = []
    for pc, rt, step in sides:
        with torch.no_grad():
            ren.render(cameras[1], rt, targets_available=False)
        finals.append(rt.cuda_module.get_framebuffer().output_final.clone())
    assert torch.equal(bits(finals[0]), bits(finals[1])) and float(finals[0].abs().max()) > 0.0
    assert ra.cuda_module.get_counters()[11] == 0


def test_add_farfield_points(tr, ren, syn, recipe):
    ini = importlib.import_module(PKG + ".initialization")
    g = syn.make_scene(N, "trained", seed=4)
    cameras = scene_cameras(ren, syn)
    centers, znear, kept = recipe["centers"], recipe["znear"], recipe["kept"]
    k = kept.shape[0]
    sides = [make_side(ren, tr, g) for _ in range(2)]  # two independent copies of the model: the ranks of a partition
    results = []
    for pc, rt, step in sides:
        counter = torch.ones((N, 1), dtype=torch.int32, device="cuda")
        results.append(step.add_farfield_points(FILTER_N, 1.0, recipe["seed"], cam_centers=centers, cam_znear=znear, extra=[(counter, 0)]))
    (pa, ra, sa), (pb, rb, sb) = sides
    n_added, (counter_a,) = results[0]
    assert n_added == k == FILTER_N - int(recipe["inside"].sum()) and results[1][0] == k
    assert pa._xyz.shape[0] == N + k and torch.equal(bits(pa._xyz[N:]), bits(kept))
    want = ini.gaussians_from_cloud(kept, torch.full((k, 3), 0.2, device="cuda"), init_scale=0.1, init_opa=0.1, init_roughness=0.0, init_f0=0.04)
    assert torch.equal(bits(pa._scaling[N:]), bits(want["scale"])) and torch.equal(bits(pa._opacity[N:]), bits(want["opacity"]))
    const = lambda value, width: torch.full((k, width), value, dtype=torch.float32, device="cuda")
    assert torch.equal(pa._diffuse[N:], const(0.2, 3)) and torch.equal(pa._f0[N:], const(0.04, 3)) and torch.equal(pa._roughness[N:], const(0.0, 1))
    assert torch.equal(bits(pa._normal[N:]), bits(const(0.0, 3)))
    assert torch.equal(pa._rotation[N:], torch.tensor([1.0, 0.0, 0.0, 0.0], device="cuda").expand(k, 4))
    assert torch.equal(counter_a, torch.cat([torch.ones((N, 1), dtype=torch.int32, device="cuda"), torch.zeros((k, 1), dtype=torch.int32, device="cuda")]))
    dist = np.linalg.norm(pa._xyz[N:].cpu().numpy().astype(np.float64)[:, None, :] - centers.cpu().numpy().astype(np.float64)[None], axis=2)
    assert not np.any(dist < znear.cpu().numpy()[None])  # no new row lies inside a sphere
    # the multi-rank guarantee: the same call on two copies leaves every tensor bit-identical
    ga, gb = ra.cuda_module.get_gaussians(), rb.cuda_module.get_gaussians()
    for x, y in zip(state_of(tr, pa, sa) + [ga.grad_flat, ga.mean, ga.scale, results[0][1][0]], state_of(tr, pb, sb) + [gb.grad_flat, gb.mean, gb.scale, results[1][1][0]]):
        assert x.shape == y.shape and x.data_ptr() != y.data_ptr() and torch.equal(bits(x), bits(y))
    assert ra.cuda_module.check_bvh() == 0, ra.cuda_module.last_error()
    # without cameras every candidate is added
    assert sb.add_farfield_points(100, 1.0, 3)[0] == 100 and pb._xyz.shape[0] == N + k + 100
    # training goes on: a step after growth runs, and the new rows move
    start = [getattr(pa, a)[N:].clone() for _, a, _ in tr.GROUPS]
    for cam in cameras:
        ren.render(cam, ra)
    sa.step()
    moved = sum(int((getattr(pa, a)[N:] != s).any(dim=1).sum()) for (_, a, _), s in zip(tr.GROUPS, start))
    assert moved > 0 and sa.steps == 1
    assert all(bool(torch.isfinite(getattr(pa, a)).all()) for _, a, _ in tr.GROUPS)
    assert ra.cuda_module.get_counters()[11] == 0
