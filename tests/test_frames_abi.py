"""CPU checks of the frames ABI (include/egr_raytracer.h: egr_eval_frames, egr_frames_args, EGR_FRAMES_*): the header text, the ctypes mirror, the exported symbol,
the torch op's schema, and the argument validation of egr_eval_frames - which runs before any HIP call, so all of this needs no device: the pointers are fake,
far apart, and a refused call never touches them."""
import ctypes as C
import importlib
import os
import re

import pytest

torch = pytest.importorskip("torch")
PKG = "editable-gaussian-reflections_amd"
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "egr_raytracer.h")
V, H, W = 2, 19, 37
STEP = 0x01000000  # 16 MiB between fake buffers: far more than any of them holds at 2 x 19 x 37
PRED = {name: 0x10000000 + i * STEP for i, name in enumerate(("final", "rgb", "depth", "normal", "roughness", "f0"))}
KINDS = ("render", "diffuse", "specular", "depth", "normal", "roughness", "f0")
TARGET = {name: 0x20000000 + i * STEP for i, name in enumerate(KINDS)}
FRAMES, SSE, PSNR, RANGE, WS = 0x30000000, 0x40000000, 0x41000000, 0x42000000, 0x50000000


@pytest.fixture(scope="module")
def cabi():
    return importlib.import_module(PKG + ".c_abi")


@pytest.fixture(scope="module")
def L(cabi):
    return cabi.lib()


def call(cabi, **kw):
    """egr_eval_frames with every argument valid unless overridden; returns the error message, "" on acceptance (never reached here: no test passes valid arguments)."""
    a = dict(num_views=V, height=H, width=W, frames=FRAMES, sse8=SSE, psnr8=PSNR, workspace=WS, predictions=dict(PRED), targets=dict(TARGET), depth_range=RANGE)
    a.update(kw)
    try:
        cabi.eval_frames(a.pop("num_views"), a.pop("height"), a.pop("width"), a.pop("frames"), a.pop("sse8"), a.pop("psnr8"), a.pop("workspace"), **a)
    except RuntimeError as e:
        return str(e)
    return ""


def test_header_declares_the_entry_and_states_the_contract():
    text = open(HEADER).read()
    hdr = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))
    assert "int egr_eval_frames(int device, const egr_frames_args *args, void *hip_stream);" in hdr
    assert "typedef struct egr_frames_args {" in hdr and "} egr_frames_args;" in hdr
    for macro in ("EGR_FRAMES_KINDS 7", "EGR_FRAMES_ALL_KINDS 0x7Fu", "EGR_FRAMES_ROUND_SAVE 0u", "EGR_FRAMES_ROUND_TRUNC 1u", "EGR_FRAMES_DEPTH_MAX 0u", "EGR_FRAMES_DEPTH_MINMAX 1u",
                  "EGR_FRAMES_SEPARATE 0u", "EGR_FRAMES_SIDE_BY_SIDE 1u", "EGR_FRAMES_WORKSPACE_BYTES(V, H, W)"):
        assert "#define " + macro in hdr, macro
    section = text[text.index("---- Evaluation frames") : text.index("int egr_eval_frames(")]
    for word in ("BEFORE any HIP call", "NaN gives byte 0", "exact", "DEFINITION", "not pinned by a fixture", "No atomics", "keep what they hold"):
        assert word in section, word
    assert 'return "egr-hip 0.8 (gfx950)"' in open(os.path.join(os.path.dirname(HEADER), "..", PKG, "csrc", "api.hip")).read()  # additive symbols: the version stays


def test_ctypes_mirror_agrees_with_the_header(cabi):
    text = open(HEADER).read()
    body = re.sub(r"/\*.*?\*/", "", text[text.index("typedef struct egr_frames_args {") : text.index("} egr_frames_args;")], flags=re.S)
    # the header's fields in order: 8 uint32, 6 prediction pointers, 7 target pointers, 5 more pointers - all naturally aligned, so the size is their sum
    names = [n.strip(" *") for line in body.split("{", 1)[1].split(";") if line.strip() for n in re.sub(r"^\s*(const\s+)?\w+\s", "", line.strip()).split(",")]
    names = [re.sub(r"\[.*\]", "", n) for n in names]
    assert names == [f[0] for f in cabi.egr_frames_args._fields_], names
    assert C.sizeof(cabi.egr_frames_args) == 8 * 4 + (6 + 7 + 5) * 8 == 176
    assert cabi.egr_frames_args.targets.size == 7 * 8 and cabi.egr_frames_args.final.offset == 32
    for name in ("KINDS", "ALL_KINDS", "ROUND_SAVE", "ROUND_TRUNC", "DEPTH_MAX", "DEPTH_MINMAX", "SEPARATE", "SIDE_BY_SIDE", "PIXELS_PER_WG", "RANGE_BLOCKS"):
        m = re.search(r"#define EGR_FRAMES_%s (0x[0-9A-Fa-f]+|\d+)u?\b" % name, text)
        assert m and int(m.group(1), 0) == getattr(cabi, "EGR_FRAMES_" + name), name
    assert cabi.FRAMES_KINDS == KINDS


def test_workspace_size_mirror(cabi):
    text = open(HEADER).read()
    assert "#define EGR_FRAMES_BLOCKS(H, W) (((size_t)(H) * (size_t)(W) + EGR_FRAMES_PIXELS_PER_WG - 1) / EGR_FRAMES_PIXELS_PER_WG)" in text
    assert ("#define EGR_FRAMES_WORKSPACE_BYTES(V, H, W) ((((size_t)(V) * (EGR_FRAMES_RANGE_BLOCKS * 8 + EGR_FRAMES_BLOCKS(H, W) * (21 * 4))) + 7) & ~(size_t)7)") in text
    used = lambda v, h, w: v * (64 * 8 + ((h * w + 4095) // 4096) * 84)  # the bytes the kernels touch: 64 key pairs and `blocks` partials of 21 uint32 per view
    macro = lambda v, h, w: (used(v, h, w) + 7) // 8 * 8  # the macro with the header's numbers
    for shape in ((1, 1, 1), (2, 5, 7), (8, 1080, 1920), (1, 1080, 1920), (3, 64, 64), (1, 19, 37)):
        assert cabi.frames_workspace_bytes(*shape) == macro(*shape) >= used(*shape), shape
        assert cabi.frames_workspace_bytes(*shape) % 8 == 0, shape  # a whole number of doubles: no allocation in 8-byte units can come out short
    assert used(1, 1, 1) == 596 and used(1, 1080, 1920) % 8 == 4  # an odd V x blocks: the partials end 4 bytes past a multiple of 8
    assert cabi.frames_workspace_bytes(1, 1, 1) == 600 and cabi.frames_workspace_bytes(1, 1080, 1920) == 512 + 507 * 84 + 4
    assert cabi.frames_workspace_bytes(8, 1080, 1920) == 8 * (512 + 507 * 84)
    # the op's own workspace: whole doubles that hold every byte of the macro (a truncating division would be 4 bytes short for an odd V x blocks)
    shim = open(os.path.join(os.path.dirname(HEADER), "..", PKG, "csrc", "torch_binding.cpp")).read()
    assert "(EGR_FRAMES_WORKSPACE_BYTES(V, H, W) + 7) / 8" in shim and "EGR_FRAMES_WORKSPACE_BYTES(V, H, W) / 8" not in shim


def test_symbol_resolves_and_the_op_has_its_schema(L):
    assert len(L.egr_eval_frames.argtypes) == 3
    assert L.egr_version().decode().startswith("egr-hip 0.8")
    importlib.import_module(PKG).load_library()
    assert str(torch.ops.egr.eval_frames.default._schema) == (
        "egr::eval_frames(Tensor? final, Tensor? rgb, Tensor? depth, Tensor? normal, Tensor? roughness, Tensor? f0, Tensor? t_final, Tensor? t_diffuse, "
        "Tensor? t_specular, Tensor? t_depth, Tensor? t_normal, Tensor? t_roughness, Tensor? t_f0, int kinds, int rounding, int depth_mode, bool side_by_side) -> "
        "(Tensor frames, Tensor sse8, Tensor psnr8, Tensor depth_range)")


def test_every_refusal_names_its_cause(cabi, L):
    assert L.egr_eval_frames(0, None, None) != 0 and "args" in L.egr_eval_last_error().decode()
    assert "num_views" in call(cabi, num_views=0) and "num_views" in call(cabi, num_views=65536)
    assert "height and width" in call(cabi, height=0) and "height and width" in call(cabi, width=0)
    assert "kinds is empty" in call(cabi, kinds=0) and "unknown bits" in call(cabi, kinds=0x80) and "unknown bits" in call(cabi, kinds=0x17F)
    assert "unknown rounding" in call(cabi, rounding=2) and "unknown depth_mode" in call(cabi, depth_mode=2) and "unknown layout" in call(cabi, layout=2)
    no_rgb = {k: v for k, v in PRED.items() if k != "rgb"}
    assert "need rgb" in call(cabi, predictions=no_rgb)
    assert "need rgb" in call(cabi, predictions=no_rgb, kinds=0b100) and "need rgb" in call(cabi, predictions=no_rgb, kinds=0b010)
    for name in ("frames", "sse8", "psnr8"):
        assert "required outputs" in call(cabi, **{name: None}), name
    assert "workspace" in call(cabi, workspace=None) and "8-byte aligned workspace" in call(cabi, workspace=WS + 4)
    image = V * H * W * 3 * 4
    assert "an output (frames) overlaps an input (final)" in call(cabi, frames=PRED["final"] + image - 1)  # frames starts in final's last byte
    assert "an output (frames) overlaps an input (rgb)" in call(cabi, frames=PRED["rgb"] + 3 * image - 1)
    assert "an output (sse8) overlaps an input (target depth)" in call(cabi, sse8=TARGET["depth"] + V * H * W * 4 - 8)
    assert "an output (psnr8) overlaps an input (target f0)" in call(cabi, psnr8=TARGET["f0"])
    assert "an output (workspace) overlaps an input (f0)" in call(cabi, workspace=PRED["f0"] + 8)
    assert "an output (depth_range) overlaps an input (roughness)" in call(cabi, depth_range=PRED["roughness"])
    frames_bytes = V * 7 * 2 * H * W * 3
    assert "two outputs (frames, sse8) overlap" in call(cabi, sse8=FRAMES + (frames_bytes - 1) // 8 * 8)  # sse8 starts in the last 8 bytes that touch frames
    assert "two outputs (sse8, psnr8) overlap" in call(cabi, psnr8=SSE + V * 21 * 8 - 8)
    assert "two outputs (psnr8, depth_range) overlap" in call(cabi, depth_range=PSNR + 8)
    assert "two outputs (frames, workspace) overlap" in call(cabi, workspace=FRAMES + 8)
    assert "two outputs (depth_range, workspace) overlap" in call(cabi, workspace=RANGE + 8)
    with pytest.raises(ValueError, match="unknown names"):
        cabi.eval_frames(V, H, W, FRAMES, SSE, PSNR, WS, predictions={"colour": 1})
