"""egr_raytrace_targets on a LIVE context through the ctypes mirror (c_abi.RawRaytracer, no torch shim in between): what it refuses - each with its own
egr_last_error text, and before anything is launched - and one successful call through the mirror method, held against egr_set_targets_chw followed by
egr_raytrace_import. torch is only the allocator of the device buffers."""
import ctypes as C
import importlib

import numpy as np
import pytest

from fused_io_common import H, N, W, cloud, same_bits, torch
from test_hip_fused_io_c_abi import GRADS, PKG, buffers, own_grads

pytestmark = pytest.mark.gpu
ORDER = (("diffuse", 3), ("specular", 3), ("depth", 1), ("normal", 3), ("roughness", 1), ("f0", 3))  # the order of egr_set_targets_chw's pointers


@pytest.fixture()
def live(syn):
    if not torch.cuda.is_available():
        pytest.fail("-m gpu tests need a GPU; the product has no CPU fallback")
    cabi = importlib.import_module(PKG + ".c_abi")
    T = buffers(syn, cloud(syn))
    raw = cabi.RawRaytracer(W, H, N, {k: v.data_ptr() for k, v in T.items()}, ppll_forward_size=8_000_000, ppll_backward_size=8_000_000,
                            device=torch.cuda.current_device(), stream=torch.cuda.current_stream().cuda_stream)
    yield cabi, raw, T
    raw.close()


def planes(T, seed=4):
    """The caller's six images, channel-major: the bound pixel-major targets plus noise of their own (so that they are not what the framebuffer holds)."""
    gen = torch.Generator().manual_seed(seed)
    return [(T["target_" + k].permute(2, 0, 1) + (0.3 * torch.randn((c, H, W), generator=gen)).cuda()).contiguous() for k, c in ORDER]


def test_what_egr_raytrace_targets_refuses_on_a_live_context(live):
    cabi, raw, T = live
    L, ctx, st = raw.L, raw.ctx, raw.stream
    grads, imgs = own_grads(), planes(T)
    grads_before = {k: grads[k].clone() for k, _ in GRADS}
    fb_before = {k: T["target_" + k].clone() for k, _ in ORDER}
    err = lambda: L.egr_last_error(ctx).decode()
    six = (C.c_void_p * 6)(*[t.data_ptr() for t in imgs])
    dst = lambda **over: cabi.egr_gaussians(count=N, **{**{k: grads[k].data_ptr() for k, _ in GRADS}, **over})
    assert L.egr_raytrace_targets(ctx, 0, None, C.byref(six), st) != 0 and "egr_raytrace_targets: targets need a grad launch" in err()
    assert L.egr_raytrace_targets(ctx, 0, C.byref(dst()), None, st) != 0 and "egr_raytrace_targets: dst needs a grad launch" in err()
    assert L.egr_raytrace_targets(ctx, 0, C.byref(dst()), C.byref(six), st) != 0 and "egr_raytrace_targets: targets need a grad launch" in err()
    for k, _ in GRADS:  # what egr_raytrace_import refuses in dst, under this entry's name
        assert L.egr_raytrace_targets(ctx, 1, C.byref(dst(**{k: None})), C.byref(six), st) != 0 and "egr_raytrace_targets: dst and its eight" in err(), k
        assert L.egr_raytrace_targets(ctx, 1, C.byref(dst(**{k: T[k].data_ptr()})), C.byref(six), st) != 0 and "egr_raytrace_targets: dst must not be the bound" in err(), k
    assert L.egr_set_grad_overwrite(ctx, 1) == 0
    assert L.egr_raytrace_targets(ctx, 1, C.byref(dst()), C.byref(six), st) != 0 and "egr_raytrace_targets: the context writes a per-launch gradient buffer" in err()
    assert L.egr_set_grad_overwrite(ctx, 0) == 0
    assert L.egr_raytrace_targets(None, 1, None, C.byref(six), st) != 0 and b"null context" in L.egr_last_error(None)
    # ---- nothing was launched: no call counted, no gradient touched, the framebuffer's targets as they were
    torch.cuda.synchronize()
    assert int(T["total_num_calls"]) == 0
    for k, _ in GRADS:
        assert same_bits(grads[k], grads_before[k]) and not bool(T[k].any()), k
    for k, _ in ORDER:
        assert same_bits(T["target_" + k], fb_before[k]), k
    assert L.egr_debug_check_bvh(ctx, st) == 0


def test_one_call_through_the_mirror_method(live):
    cabi, raw, T = live
    imgs = planes(T)
    kept = [t.clone() for t in imgs]
    fb_before = {k: T["target_" + k].clone() for k, _ in ORDER}
    bound = lambda: {k: T[k].clone() for k, _ in GRADS + (("total_weight", 1),)}

    def clear():
        for k, _ in GRADS + (("total_weight", 1),):
            T[k].zero_()
        T["total_num_calls"].zero_()

    # in place, with the import: the framebuffer's targets stay, the caller's gradients get caller + bound
    grads = own_grads()
    before = {k: grads[k].clone() for k, _ in GRADS}
    raw.raytrace_targets(True, {k: grads[k].data_ptr() for k, _ in GRADS}, [t.data_ptr() for t in imgs])
    c = raw.counters()
    assert c.status == 0 and c.rays[0] == W * H and int(T["total_num_calls"]) == 1 and bool(T["grads_enabled"])
    in_place = bound()
    for k, _ in GRADS:
        assert bool(torch.nan_to_num(T[k]).any()), k
        assert same_bits(grads[k], before[k] + T[k]), k
    for (k, _), t, t0 in zip(ORDER, imgs, kept):
        assert same_bits(T["target_" + k], fb_before[k]) and same_bits(t, t0), k
    # the sequence it replaces: upload, then the importing launch - the same rays (total_num_calls), gradients equal up to the order of the float atomics
    clear()
    assert raw.L.egr_set_targets_chw(raw.ctx, *[t.data_ptr() for t in imgs], raw.stream) == 0
    scratch = own_grads()
    raw.raytrace_import({k: scratch[k].data_ptr() for k, _ in GRADS})
    assert raw.counters().status == 0
    classic = bound()
    # ... and a launch that reads the framebuffer's targets through the new entry (targets = NULL) is that launch again
    clear()
    raw.raytrace_targets(True, None, None)
    assert raw.counters().status == 0
    plain = bound()
    for k in classic:
        top = float(torch.nan_to_num(classic[k]).abs().max())
        assert top > 0, k
        for name, other in (("in_place", in_place), ("targets_null", plain)):
            d = float((torch.nan_to_num(other[k]).double() - torch.nan_to_num(classic[k]).double()).abs().max())
            assert d <= 1e-5 * top, (name, k, d, top)
    # absent targets read zero: six NULL entries against zeros uploaded
    clear()
    raw.raytrace_targets(True, None, [None] * 6)
    assert raw.counters().status == 0
    nulls = bound()
    clear()
    assert raw.L.egr_set_targets_chw(raw.ctx, None, None, None, None, None, None, raw.stream) == 0
    raw.raytrace(True)
    assert raw.counters().status == 0
    zeros = bound()
    for k in zeros:
        top = float(torch.nan_to_num(zeros[k]).abs().max())
        d = float((torch.nan_to_num(nulls[k]).double() - torch.nan_to_num(zeros[k]).double()).abs().max())
        assert d <= 1e-5 * top, (k, d, top)
