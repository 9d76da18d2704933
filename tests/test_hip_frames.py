"""Evaluation frames on the GPU: the fused kernel of csrc/frames.hip (torch.ops.egr.eval_frames; evaluation.frames) and evaluation.export_views.
Team help is off (conftest.py), so launches are reproducible bit for bit.

Every byte is compared EXACTLY:
  render, diffuse, specular     against evaluation.quantise of the `display` tensor of the existing torch.ops.egr.eval_metrics on the same inputs (the same tone_display)
  depth, normal, roughness, f0  against the literal torch expressions on the CPU in fp32: x / hi, (x - lo) / (hi - lo), x / 2 + 0.5 and the identity are correctly
                                rounded single operations, so there is nothing to tolerate. NaN positions are held to the definition (byte 0).
  sse8                          against the int64 sum numpy computes from the returned frames
  psnr8                         against numpy fp64 from that integer, relative 16 * 2^-53: a division, a square root, a log10 and a mean
                                (measured on an MI355X: DESIGN.md 8f-9)
The shapes are the smallest that reach every path: one pixel; hw odd (element-wise path); hw % 4 == 0 with W % 4 != 0 (word stores when separate, byte stores side by
side); aligned and unaligned with more pixels (2304, 2310) than one workgroup's 1024 quads cover in a step, and enough values for every threshold."""
import importlib
import json
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from hip_common import cam_obj, ren, report, tracer, views  # noqa: E402,F401

pytestmark = pytest.mark.gpu
PKG = "editable-gaussian-reflections_amd"
SHAPES = [(1, 1, 1), (2, 5, 7), (2, 6, 10), (1, 32, 72), (2, 33, 70)]
KINDS = ("render", "diffuse", "specular", "depth", "normal", "roughness", "f0")
CHANNELS = (3, 3, 3, 1, 3, 1, 3)
SPECIALS = [float("nan"), float("inf"), -float("inf"), -0.0, -0.3, 1.5, 1e30, 1e-40]


@pytest.fixture(scope="module")
def ev(ren):
    mod = importlib.import_module(PKG + ".evaluation")
    mod.load_library()
    return mod


def thresholds():
    """Every (k + 0.5) / 255 and k / 255 in fp32 with both neighbours, then the specials: 1544 values."""
    k = torch.arange(256, dtype=torch.float64)
    mids = torch.cat([((k + 0.5) / 255).to(torch.float32), (k / 255).to(torch.float32)])
    return torch.cat([mids, torch.nextafter(mids, torch.full_like(mids, 2.0)), torch.nextafter(mids, torch.full_like(mids, -1.0)), torch.tensor(SPECIALS)])


_INPUTS = {}


def make_inputs(V, H, W):
    """CPU tensors, made once per shape and never modified: predictions in the layout of render_views_raw and channel-major targets. Unit-range kinds start with the
    threshold values (as many as the tensor holds, from a rotating start so that the small shapes see different ones); normals hold 2x - 1 of them; the HDR kinds
    hold the specials; depth predictions hold thresholds scaled by 3 and the specials. Depth targets are positive; the two small shapes add a zero and a subnormal
    (lo = 0 or tiny), the two large ones keep their minimum near 0.5, so that "minmax" subtracts a lo well above 0 on thousands of pixels."""
    if (V, H, W) in _INPUTS:
        return _INPUTS[(V, H, W)]
    g = torch.Generator().manual_seed(1000 * H + W)
    th = thresholds()

    def seeded(shape, base, values, shift):
        t = base.clone().reshape(-1)
        n = min(t.numel(), values.numel())
        t[torch.randperm(t.numel(), generator=g)[:n]] = values.roll(shift)[:n]
        return t.reshape(shape).contiguous()

    rnd = lambda *s: torch.rand(*s, generator=g)
    hdr_specials = torch.tensor(SPECIALS + [3e38, -0.01, 0.0])
    pm3, pm1, cm3, cm1 = (V, 3, H, W, 3), (V, 3, H, W, 1), (V, 3, H, W), (V, 1, H, W)
    pred = dict(final=seeded((V, H, W, 3), 3 * rnd(V, H, W, 3) ** 2, hdr_specials, 0), rgb=seeded(pm3, 2 * rnd(*pm3) ** 2, hdr_specials, 3),
                depth=seeded(pm1, 0.5 + 3.5 * rnd(*pm1), torch.cat([3 * th[:512], th[-8:]]), 5), normal=seeded(pm3, 2 * rnd(*pm3) - 1, 2 * th - 1, 7),
                roughness=seeded(pm1, rnd(*pm1), th, 11), f0=seeded(pm3, rnd(*pm3), th, 13))
    noisy = lambda t: (t * (1 + 0.17 * torch.randn(t.shape, generator=g))).abs()
    pm = lambda t: t.movedim(-1, 1)  # [V,H,W,C] -> [V,C,H,W]
    target = dict(render=seeded(cm3, noisy(pm(pred["final"])).nan_to_num(0.5, 2.0, 0.1), hdr_specials, 1),
                  diffuse=seeded(cm3, noisy(pm(pred["rgb"][:, 0])).nan_to_num(0.5, 2.0, 0.1), hdr_specials, 2),
                  specular=seeded(cm3, noisy(pm(pred["rgb"][:, 1] + pred["rgb"][:, 2])).nan_to_num(0.5, 2.0, 0.1), hdr_specials, 4),
                  depth=seeded(cm1, 0.5 + 3.5 * rnd(*cm1), torch.tensor([0.0, 1e-40]) if 2 < H * W <= 60 else torch.tensor([]), 0), normal=seeded(cm3, 2 * rnd(*cm3) - 1, 2 * th - 1, 17),
                  roughness=seeded(cm1, rnd(*cm1), th, 19), f0=seeded(cm3, rnd(*cm3), th, 23))
    _INPUTS[(V, H, W)] = (pred, target)
    return pred, target


def on_gpu(d):
    return {k: v.cuda() for k, v in d.items()}


def literal_bytes(m, rule):
    """The literal torch expression of each rule on the mapped CPU tensor `m`; NaN positions by the definition (byte 0)."""
    y = m.mul(255).add(0.5).clamp(0, 255) if rule == "save" else m.clamp(0, 1) * 255
    return torch.where(torch.isnan(y), torch.zeros_like(y), y).to(torch.uint8)


def expected_plain(kind, pred, target, rule, depth_mode, lo_hi=None):
    """[V,2,H,W,3] expected bytes of depth / normal / roughness / f0 from CPU fp32 torch."""
    k = KINDS.index(kind)
    p = {"depth": pred["depth"], "normal": pred["normal"], "roughness": pred["roughness"], "f0": pred["f0"]}[kind][:, 0]  # [V,H,W,C]
    t = target[kind].movedim(1, -1)  # [V,H,W,C]
    sides = []
    for x in (p, t):
        if kind == "depth":
            lo = target["depth"].amin(dim=(1, 2, 3)).reshape(-1, 1, 1, 1) if lo_hi is None else lo_hi[0]
            hi = target["depth"].amax(dim=(1, 2, 3)).reshape(-1, 1, 1, 1) if lo_hi is None else lo_hi[1]
            m = x / hi if depth_mode == "max" else (x - lo) / (hi - lo)
        elif kind == "normal":
            m = x / 2 + 0.5
        else:
            m = x
        sides.append(literal_bytes(m, rule).expand(-1, -1, -1, 3) if CHANNELS[k] == 1 else literal_bytes(m, rule))
    return torch.stack(sides, dim=1)


def numpy_metrics(frames):
    """sse8 [V,7,3] int64 and psnr8 [V,7,2] fp64 from separate-layout frames [V,7,2,H,W,3], in numpy."""
    f = frames.cpu().numpy().astype(np.int64)
    V, _, _, H, W, _ = f.shape
    sse = ((f[:, :, 0] - f[:, :, 1]) ** 2).sum(axis=(2, 3))
    n = 65025.0 * float(H * W)
    with np.errstate(divide="ignore"):
        s = sse.astype(np.float64)
        per = 20.0 * np.log10(1.0 / np.sqrt(s / n))
        psnr = np.stack([((per[..., 0] + per[..., 1]) + per[..., 2]) / 3.0, 10.0 * np.log10(1.0 / (sse.sum(-1).astype(np.float64) / (3.0 * n)))], -1)
    return sse, psnr


@pytest.mark.parametrize("rule", ["save", "trunc"])
@pytest.mark.parametrize("V,H,W", SHAPES)
def test_tone_mapped_kinds_equal_quantise_of_the_existing_display(ev, V, H, W, rule):
    pred, target = (on_gpu(d) for d in make_inputs(V, H, W))
    _, _, disp = torch.ops.egr.eval_metrics(pred["final"], pred["rgb"], target["render"], target["diffuse"], target["specular"], True)  # [V,3,2,3,H,W]
    want = ev.quantise(disp.cpu(), rule).permute(0, 1, 2, 4, 5, 3)  # [V,3,2,H,W,3]
    got = ev.frames(final=pred["final"], rgb=pred["rgb"], targets={k: target[k] for k in KINDS[:3]}, kinds=KINDS[:3], rounding=rule)
    assert got.frames.shape == (V, 7, 2, H, W, 3) and got.frames.dtype == torch.uint8
    assert torch.equal(got.frames[:, :3].cpu(), want), int((got.frames[:, :3].cpu() != want).sum())
    if H * W > 100:
        assert int(torch.isnan(disp).sum()) > 0 and len(torch.unique(want)) > 100  # the specials are in, and the bytes are spread


@pytest.mark.parametrize("depth_mode", ["max", "minmax"])
@pytest.mark.parametrize("rule", ["save", "trunc"])
@pytest.mark.parametrize("V,H,W", SHAPES)
def test_plain_kinds_equal_the_literal_torch_expressions(ev, V, H, W, rule, depth_mode):
    cpu_pred, cpu_target = make_inputs(V, H, W)
    pred, target = on_gpu(cpu_pred), on_gpu(cpu_target)
    names = KINDS[3:]
    got = ev.frames(depth=pred["depth"], normal=pred["normal"], roughness=pred["roughness"], f0=pred["f0"], targets={k: target[k] for k in names}, kinds=names,
                    rounding=rule, depth_mode=depth_mode)
    fr = got.frames.cpu()
    for name in names:
        want = expected_plain(name, cpu_pred, cpu_target, rule, depth_mode)
        k = KINDS.index(name)
        assert torch.equal(fr[:, k], want), (name, int((fr[:, k] != want).sum()))
    if H * W >= 2304:  # every byte value occurs on both sides of the unit-range kinds (all thresholds are in)
        for name in ("roughness", "f0", "normal"):
            assert len(torch.unique(fr[:, KINDS.index(name), 0])) == 256 and len(torch.unique(fr[:, KINDS.index(name), 1])) == 256, name
    # depth_range: amin and amax of each view's target depth, bit for bit
    want_range = torch.stack([cpu_target["depth"].amin(dim=(1, 2, 3)), cpu_target["depth"].amax(dim=(1, 2, 3))], dim=1)
    assert torch.equal(got.depth_range.cpu().view(torch.int32), want_range.view(torch.int32)), (got.depth_range, want_range)


def test_depth_range_nan_and_zero(ev):
    V, H, W = 2, 33, 70
    cpu_pred, cpu_target = make_inputs(V, H, W)
    depth = cpu_pred["depth"].cuda()
    base = ev.frames(depth=depth, targets={"depth": cpu_target["depth"].cuda()}, kinds=["depth"])
    t = cpu_target["depth"].clone()
    t[1, 0, 17, 3] = float("nan")
    got = ev.frames(depth=depth, targets={"depth": t.cuda()}, kinds=["depth"])
    assert bool(torch.isnan(got.depth_range[1]).all()) and torch.equal(got.depth_range[0], base.depth_range[0])  # a NaN wins at both ends, in its own view
    assert int(got.frames[1, 3].max()) == 0 and torch.equal(got.frames[0, 3], base.frames[0, 3]) and int(base.frames[1, 3].max()) > 0
    assert torch.equal(got.sse8[1, 3].cpu(), torch.zeros(3, dtype=torch.int64)) and torch.equal(got.sse8[0, 3], base.sse8[0, 3])
    zero = torch.zeros_like(cpu_target["depth"])
    for mode in ("max", "minmax"):
        got = ev.frames(depth=depth, targets={"depth": zero.cuda()}, kinds=["depth"], depth_mode=mode)
        z = torch.zeros(V, 1, 1, 1)
        want = expected_plain("depth", cpu_pred, dict(cpu_target, depth=zero), "save", mode, lo_hi=(z, z))  # IEEE: x / 0 = +-inf -> 255 / 0, 0 / 0 = NaN -> 0
        assert torch.equal(got.frames[:, 3].cpu(), want), mode
        assert int(want[:, 0].max()) == 255 and int(want[:, 1].max()) == 0 and float(got.depth_range.abs().max()) == 0.0


@pytest.mark.parametrize("V,H,W", SHAPES)
def test_sse8_is_exact_and_psnr8_follows(ev, V, H, W):
    pred, target = (on_gpu(d) for d in make_inputs(V, H, W))
    got = ev.frames(**pred, targets=target)
    sse, psnr = numpy_metrics(got.frames)
    assert got.sse8.dtype == torch.int64 and np.array_equal(got.sse8.cpu().numpy(), sse)
    p = got.psnr8.cpu().numpy()
    assert got.psnr8.dtype == torch.float64 and np.array_equal(np.isinf(p), np.isinf(psnr)) and not np.isnan(p).any()
    fin = np.isfinite(psnr)
    err, size = np.abs(p[fin] - psnr[fin]), np.abs(psnr[fin])  # (a PSNR of exactly 0 dB - one pixel, mse 1 - has to be met exactly)
    rel = float((err[size > 0] / size[size > 0]).max()) if (size > 0).any() else 0.0
    report(f"frames_psnr8_{V}x{H}x{W}", worst_relative_error=f"{rel:.2e}", in_units_of_2pow53=f"{rel * 2.0 ** 53:.2f}", bar=16)
    assert bool((err <= 16 * 2.0 ** -53 * size).all()), (rel, err.max())
    again = ev.frames(**pred, targets=target)  # two runs: the same bits
    assert torch.equal(again.frames, got.frames) and torch.equal(again.sse8, got.sse8) and torch.equal(again.psnr8.view(torch.int64), got.psnr8.view(torch.int64))
    # identical sides: 0 and +inf; a kind without its target (or without its prediction): -1 and NaN
    same = dict(target, roughness=pred["roughness"][:, 0].movedim(-1, 1).contiguous(), f0=pred["f0"][:, 0].movedim(-1, 1).contiguous())
    del same["normal"]
    ident = ev.frames(**dict(pred, final=None), targets=same)
    for k in (5, 6):
        assert int(ident.sse8[:, k].abs().max()) == 0 and bool((ident.psnr8[:, k] == float("inf")).all())
    for k in (0, 4):  # render lacks its prediction, normal its target
        assert bool((ident.sse8[:, k] == -1).all()) and bool(torch.isnan(ident.psnr8[:, k]).all())
    assert torch.equal(ident.frames[:, 4, 0], got.frames[:, 4, 0]) and torch.equal(ident.frames[:, 0, 1], got.frames[:, 0, 1])  # the side that exists is written
    assert torch.equal(ident.sse8[:, 1:4], got.sse8[:, 1:4])


@pytest.mark.parametrize("rule,depth_mode", [("save", "max"), ("trunc", "minmax")])
@pytest.mark.parametrize("V,H,W", SHAPES)
def test_side_by_side_is_the_concatenation(ev, V, H, W, rule, depth_mode):
    pred, target = (on_gpu(d) for d in make_inputs(V, H, W))
    sep = ev.frames(**pred, targets=target, rounding=rule, depth_mode=depth_mode)
    sbs = ev.frames(**pred, targets=target, rounding=rule, depth_mode=depth_mode, layout="side_by_side")
    assert sbs.frames.shape == (V, 7, H, 2 * W, 3)
    assert torch.equal(sbs.frames, torch.cat([sep.frames[:, :, 0], sep.frames[:, :, 1]], dim=3))
    assert torch.equal(sbs.sse8, sep.sse8) and torch.equal(sbs.psnr8.view(torch.int64), sep.psnr8.view(torch.int64)) and torch.equal(sbs.depth_range, sep.depth_range)


@pytest.mark.parametrize("shift", [0, 1], ids=["frames_aligned", "frames_off_by_one_byte"])
@pytest.mark.parametrize("V,H,W", SHAPES)
def test_kinds_and_bounds_on_caller_buffers(ev, V, H, W, shift):
    """Through ctypes on buffers filled with a sentinel: unselected slots and 64 guard bytes around every output keep it; a view does not depend on its neighbours."""
    cabi = importlib.import_module(PKG + ".c_abi")
    pred, target = (on_gpu(d) for d in make_inputs(V, H, W))
    full = ev.frames(**pred, targets=target)
    G, S = 64, 0xA5
    selected = ("render", "depth", "normal", "f0")  # f0 without its target, roughness and the others not selected
    mask = sum(1 << KINDS.index(k) for k in selected)
    stream, device = torch.cuda.current_stream().cuda_stream, torch.cuda.current_device()

    def run(v0, v1, layout):
        n = v1 - v0
        sizes = dict(frames=n * 7 * 2 * H * W * 3, sse8=n * 21 * 8, psnr8=n * 14 * 8, depth_range=n * 8)
        bufs = {k: torch.full((G + shift + b + G,), S, dtype=torch.uint8, device="cuda") for k, b in sizes.items()}
        off = {k: G + (shift if k == "frames" else 0) for k in sizes}  # (torch's allocations are at least 8-byte aligned, and so is G)
        assert all((bufs[k].data_ptr() + off[k]) % 8 == 0 for k in sizes if k != "frames")
        ws = torch.empty(cabi.frames_workspace_bytes(n, H, W) // 8 + 1, dtype=torch.float64, device="cuda")
        keep_p = {k: t[v0:v1].contiguous() for k, t in pred.items()}  # (the slices live until the synchronize below)
        keep_t = {k: target[k][v0:v1].contiguous() for k in KINDS if k != "f0"}
        preds, targets = {k: t.data_ptr() for k, t in keep_p.items()}, {k: t.data_ptr() for k, t in keep_t.items()}
        cabi.eval_frames(n, H, W, bufs["frames"].data_ptr() + off["frames"], bufs["sse8"].data_ptr() + off["sse8"], bufs["psnr8"].data_ptr() + off["psnr8"], ws.data_ptr(),
                         predictions=preds, targets=targets, kinds=mask, layout=layout, depth_range=bufs["depth_range"].data_ptr() + off["depth_range"], device=device, stream=stream)
        torch.cuda.synchronize()
        out = {}
        for k, b in sizes.items():
            whole = bufs[k].cpu()
            body = whole[off[k] : off[k] + b]
            assert bool((whole[: off[k]] == S).all()) and bool((whole[off[k] + b :] == S).all()), ("guard bytes", k)
            out[k] = body
        return out

    out = run(0, V, cabi.EGR_FRAMES_SEPARATE)
    fr = out["frames"].reshape(V, 7, 2, H, W, 3)
    sse = out["sse8"].view(torch.int64).reshape(V, 7, 3)
    psnr = out["psnr8"].view(torch.float64).reshape(V, 7, 2)
    sentinel64 = int.from_bytes(bytes([S] * 8), "little", signed=True)
    for k, name in enumerate(KINDS):
        if name not in selected:
            assert bool((fr[:, k] == S).all()) and bool((sse[:, k] == sentinel64).all()) and bool((psnr[:, k].view(torch.int64) == sentinel64).all()), name
        elif name == "f0":
            assert torch.equal(fr[:, k, 0], full.frames[:, k, 0].cpu()) and bool((fr[:, k, 1] == S).all())  # the prediction side alone
            assert bool((sse[:, k] == -1).all()) and bool(torch.isnan(psnr[:, k]).all())
        else:
            assert torch.equal(fr[:, k], full.frames[:, k].cpu()) and torch.equal(sse[:, k], full.sse8[:, k].cpu()), name
            assert torch.equal(psnr[:, k].view(torch.int64), full.psnr8[:, k].cpu().view(torch.int64)), name
    assert torch.equal(out["depth_range"].view(torch.float32).reshape(V, 2), full.depth_range.cpu())
    side = run(0, V, cabi.EGR_FRAMES_SIDE_BY_SIDE)["frames"].reshape(V, 7, H, 2 * W, 3)
    for k, name in enumerate(KINDS):
        if name not in selected:
            assert bool((side[:, k] == S).all()), name
        elif name == "f0":
            assert torch.equal(side[:, k, :, :W], full.frames[:, k, 0].cpu()) and bool((side[:, k, :, W:] == S).all())
        else:
            assert torch.equal(side[:, k], torch.cat([full.frames[:, k, 0], full.frames[:, k, 1]], dim=2).cpu()), name
    if V == 2:  # V = 1 on a slice equals that slice of V = 2
        one = run(1, 2, cabi.EGR_FRAMES_SEPARATE)
        assert torch.equal(one["frames"].reshape(7, 2, H, W, 3), fr[1]) and torch.equal(one["sse8"], out["sse8"].reshape(V, -1)[1]) and torch.equal(one["psnr8"], out["psnr8"].reshape(V, -1)[1])
        assert torch.equal(one["depth_range"], out["depth_range"].reshape(V, -1)[1])


def test_depth_without_its_target_is_skipped(ev):
    V, H, W = 2, 5, 7
    pred, target = (on_gpu(d) for d in make_inputs(V, H, W))
    got = ev.frames(depth=pred["depth"], roughness=pred["roughness"], targets={"roughness": target["roughness"]}, kinds=["depth", "roughness"])
    full = ev.frames(**pred, targets=target)
    assert bool((got.sse8[:, 3] == -1).all()) and bool(torch.isnan(got.psnr8[:, 3]).all()) and torch.equal(got.frames[:, 5], full.frames[:, 5])
    alone = ev.frames(depth=pred["depth"], kinds=["depth"])  # nothing to write: -1 and NaN are still reported
    assert bool((alone.sse8[:, 3] == -1).all()) and bool(torch.isnan(alone.psnr8[:, 3]).all())
    with pytest.raises(RuntimeError, match="need rgb"):
        ev.frames(final=pred["final"], targets={"diffuse": target["diffuse"]}, kinds=["diffuse"])
    with pytest.raises(ValueError, match="kinds"):
        ev.frames(final=pred["final"], kinds=["colour"])


def read_tree(fm, files):
    return [{kind: {side: fm.read_png(path) for side, path in sides.items()} for kind, sides in per_view.items()} for per_view in files]


def test_export_views_end_to_end(ren, ev, syn, tmp_path):
    fm = importlib.import_module(PKG + ".formats")
    W, H, V, S, base = 37, 19, 3, 2, 20
    torch.manual_seed(11)  # (random_seeds of a new tracer: the same jitter on every run)
    rt = tracer(ren, syn, W=W, H=H, N=300)
    m = rt.cuda_module
    m.get_config().jitter_primary_rays.fill_(True)
    tg = syn.make_targets(W, H)
    cams = [cam_obj(ren, c, tg) for c in views(syn, V)]
    for i, c in enumerate(cams):  # every view its own ground truth
        c.diffuse_image = (c.diffuse_image * (1.0 + 0.1 * i)).contiguous()
        c.original_image = (c.diffuse_image + c.specular_image).contiguous()
        c.depth_image = (c.depth_image * (1.0 + 0.5 * i) + torch.linspace(0, 1, W, device="cuda")).contiguous()
    fb = m.get_framebuffer()
    held = {k: getattr(fb, k).clone() for k in ("output_final", "output_denoised", "output_rgb", "output_depth", "accumulated_rgb", "accumulated_sample_count")}
    calls = lambda: int(m.get_metadata().total_num_calls)
    m.get_metadata().total_num_calls.fill_(base)
    plain = ev.evaluate_views(cams, rt, spp=S, ssim=True)
    m.get_metadata().total_num_calls.fill_(base)
    mem = ev.export_views(cams, rt, out_dir=None, spp=S, ssim=True)
    assert calls() == base + V * S == base + 6
    assert mem.files == [{}, {}, {}] and len(mem.frames) == V and sorted(mem.frames[0]) == sorted(KINDS) and not os.listdir(tmp_path)
    out = str(tmp_path / "out")
    m.get_metadata().total_num_calls.fill_(base)
    res = ev.export_views(cams, rt, out_dir=out, spp=S, ssim=True)
    assert calls() == base + 6 and res.frames is None
    for k, t in held.items():
        assert torch.equal(getattr(fb, k), t), k  # the framebuffer keeps its bits
    # the files exist under the reference's names and decode to the frames
    for v in range(V):
        for kind in KINDS:
            want = {"pred": os.path.join(out, kind, f"{v:05d}_{kind}.png"), "gt": os.path.join(out, kind + "_gt", f"{v:05d}_{kind}.png")}
            assert res.files[v][kind] == want and all(os.path.isfile(p) for p in want.values())
    assert sorted(os.listdir(out)) == sorted([k for k in KINDS] + [k + "_gt" for k in KINDS] + ["metrics.json"])
    decoded = read_tree(fm, res.files)
    for v in range(V):
        for kind in KINDS:
            for side in ("pred", "gt"):
                a = decoded[v][kind][side]
                assert a.shape == (H, W, 3) and np.array_equal(a, mem.frames[v][kind][side]), (v, kind, side)
        assert np.array_equal(decoded[v]["depth"]["gt"][..., 0], decoded[v]["depth"]["gt"][..., 2]) and int(decoded[v]["depth"]["gt"].max()) == 255  # x / amax, replicated
    # metrics.json = metrics.py on the decoded files: PeakSignalNoiseRatio(data_range = 1) of to_tensor bytes, the mean over the views, 2 places
    recomputed = {}
    for kind in KINDS:
        per_view = []
        for v in range(V):
            d = decoded[v][kind]["pred"].astype(np.int64) - decoded[v][kind]["gt"].astype(np.int64)
            sse = int((d * d).sum())
            assert sse == int(res.sse8[kind][v].sum())
            per_view.append(10.0 * np.log10(1.0 / (sse / (3.0 * 65025.0 * H * W))))
        recomputed[kind] = {"psnr": round(float(np.mean(per_view)), 2)}
    assert json.load(open(os.path.join(out, "metrics.json"))) == recomputed
    assert all(np.isfinite(recomputed[k]["psnr"]) for k in KINDS) and 5.0 < recomputed["render"]["psnr"] < 60.0, recomputed
    # the float fields are evaluate_views', bit for bit
    for name in ev.PASSES:
        for field in ("psnr", "psnr_global", "sse", "ssim", "ssim_interior", "ssim_channels"):
            a, b = getattr(res, field)[name], getattr(plain, field)[name]
            assert torch.equal(a.nan_to_num(-7.0), b.nan_to_num(-7.0)) and torch.equal(getattr(mem, field)[name].nan_to_num(-7.0), b.nan_to_num(-7.0)), (name, field)
        assert res.mean[name] == plain.mean[name] and res.mean_ssim[name] == plain.mean_ssim[name]
    for kind in KINDS:
        assert torch.equal(res.psnr8[kind], mem.psnr8[kind]) and torch.equal(res.sse8[kind], mem.sse8[kind]) and res.psnr8[kind].dtype == torch.float64 and res.sse8[kind].dtype == torch.int64
    want_range = torch.stack([torch.stack([c.depth_image.amin(), c.depth_image.amax()]) for c in cams]).cpu()
    assert torch.equal(res.depth_range, want_range)
    # a chunk boundary changes no byte; side by side is one file per kind
    m.get_metadata().total_num_calls.fill_(base)
    two = ev.export_views(cams, rt, out_dir=None, spp=S, views_per_call=2)
    m.get_metadata().total_num_calls.fill_(base)
    vs_dir = str(tmp_path / "vs")
    vs = ev.export_views(cams, rt, out_dir=vs_dir, spp=S, views_per_call=2, layout="side_by_side", kinds=("render", "normal"), png_level=1)
    assert sorted(os.listdir(vs_dir)) == ["metrics.json", "normal_vs", "render_vs"] and sorted(json.load(open(os.path.join(vs_dir, "metrics.json")))) == ["normal", "render"]
    for v in range(V):
        for kind in KINDS:
            for side in ("pred", "gt"):
                assert np.array_equal(two.frames[v][kind][side], mem.frames[v][kind][side]), (v, kind, side)
        for kind in ("render", "normal"):
            assert vs.files[v][kind] == {"vs": os.path.join(vs_dir, kind + "_vs", f"{v:05d}_{kind}.png")}
            assert np.array_equal(fm.read_png(vs.files[v][kind]["vs"]), np.concatenate([mem.frames[v][kind]["pred"], mem.frames[v][kind]["gt"]], axis=1))
    for kind in KINDS:
        assert torch.equal(two.psnr8_global[kind], mem.psnr8_global[kind])
    # novel views: cameras without ground truth write the prediction sides only (depth needs its target's range: skipped)
    novel = [cam_obj(ren, c) for c in views(syn, V)]
    m.get_metadata().total_num_calls.fill_(base)
    nv_dir = str(tmp_path / "novel")
    nv = ev.export_views(novel, rt, out_dir=nv_dir, spp=S)
    assert sorted(os.listdir(nv_dir)) == sorted([k for k in KINDS if k != "depth"] + ["metrics.json"]) and json.load(open(os.path.join(nv_dir, "metrics.json"))) == {}
    for v in range(V):
        assert sorted(nv.files[v]) == sorted(k for k in KINDS if k != "depth")
        for kind, sides in nv.files[v].items():
            assert list(sides) == ["pred"] and np.array_equal(fm.read_png(sides["pred"]), mem.frames[v][kind]["pred"]), (v, kind)
    assert nv.depth_range is None and bool(torch.isnan(nv.psnr8["render"]).all()) and bool((nv.sse8["depth"] == -1).all())
