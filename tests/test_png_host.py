"""Host side of the frame export, no device: formats.write_png / read_png (8-bit grey and RGB, zlib and struct of the standard library) - round trips, the file
structure chunk by chunk, the refusals by name, all five filter types on rows encoded here by the PNG specification's definitions, and Pillow as a second
reader and writer where it is installed - and evaluation.quantise, the byte rule of csrc/frames.hip as plain torch, against the literal torch expressions."""
import importlib
import io
import struct
import zlib

import numpy as np
import pytest

torch = pytest.importorskip("torch")
PKG = "editable-gaussian-reflections_amd"
SIZES = ((1, 1), (1, 17), (17, 1), (19, 37))


@pytest.fixture(scope="module")
def fm():
    return importlib.import_module(PKG + ".formats")


@pytest.fixture(scope="module")
def ev():
    return importlib.import_module(PKG + ".evaluation")


def image(h, w, rgb, seed=0):
    """Half smooth (so that filters and compression have something to do), half noise."""
    rng = np.random.default_rng(seed + 1000 * h + w)
    yy, xx = np.mgrid[0:h, 0:w]
    a = np.stack([(5 * yy + 3 * xx) % 256, (2 * yy + 7 * xx + 40) % 256, (yy * xx) % 256], -1).astype(np.uint8)
    noise = rng.integers(0, 256, a.shape, dtype=np.uint8)
    a = np.where((xx % 2 == 0)[..., None], a, noise).astype(np.uint8)
    return np.ascontiguousarray(a if rgb else a[..., 0])


def chunks(data):
    """[(kind, body, crc ok)] of a PNG byte string, after the signature."""
    out, at = [], 8
    while at < len(data):
        (n,) = struct.unpack(">I", data[at : at + 4])
        kind, body = data[at + 4 : at + 8], data[at + 8 : at + 8 + n]
        out.append((kind, body, struct.unpack(">I", data[at + 8 + n : at + 12 + n])[0] == zlib.crc32(kind + body) & 0xFFFFFFFF))
        at += 12 + n
    assert at == len(data)
    return out


def make_png(w, h, depth, colour, interlace, raw, level=6):
    """A PNG from raw filtered scanlines, for the reader's tests."""
    chunk = lambda k, d: struct.pack(">I", len(d)) + k + d + struct.pack(">I", zlib.crc32(k + d) & 0xFFFFFFFF)
    return b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, depth, colour, 0, 0, interlace)) + chunk(b"IDAT", zlib.compress(raw, level)) + chunk(b"IEND", b"")


@pytest.mark.parametrize("level", [0, 9])
@pytest.mark.parametrize("filt", ["none", "sub", "up"])
@pytest.mark.parametrize("rgb", [False, True], ids=["grey", "rgb"])
@pytest.mark.parametrize("h,w", SIZES)
def test_round_trip(fm, h, w, rgb, filt, level):
    a = image(h, w, rgb)
    data = fm.encode_png(a, level=level, filter=filt)
    back = fm.decode_png(data)
    assert back.dtype == np.uint8 and back.shape == a.shape and np.array_equal(back, a)
    f = io.BytesIO()
    assert fm.write_png(f, a, level=level, filter=filt) == len(data) and f.getvalue() == data  # a file object takes the same bytes
    f.seek(0)
    assert np.array_equal(fm.read_png(f), a)


def test_paths_and_defaults(fm, tmp_path):
    a = image(19, 37, True)
    path = str(tmp_path / "a.png")
    n = fm.write_png(path, a)
    assert n == (tmp_path / "a.png").stat().st_size and np.array_equal(fm.read_png(path), a)
    assert open(path, "rb").read() == fm.encode_png(a, 6, "up")  # the defaults
    for bad in (a.astype(np.float32), a[..., :2], np.zeros((0, 3, 3), np.uint8), a[None]):
        with pytest.raises(ValueError, match="uint8"):
            fm.encode_png(bad)
    with pytest.raises(ValueError, match="filter"):
        fm.encode_png(a, filter="paeth")
    with pytest.raises(ValueError, match="level"):
        fm.encode_png(a, level=10)


@pytest.mark.parametrize("rgb", [False, True], ids=["grey", "rgb"])
def test_file_structure(fm, rgb):
    a = image(19, 37, rgb)
    for filt, code in (("none", 0), ("sub", 1), ("up", 2)):
        data = fm.encode_png(a, level=6, filter=filt)
        assert data[:8] == b"\x89PNG\r\n\x1a\n"
        cs = chunks(data)
        assert [k for k, _, _ in cs] == [b"IHDR", b"IDAT", b"IEND"] and all(ok for _, _, ok in cs)  # IHDR first, one zlib stream, IEND last, every CRC verifies
        assert struct.unpack(">IIBBBBB", cs[0][1]) == (37, 19, 8, 2 if rgb else 0, 0, 0, 0) and cs[2][1] == b""
        raw = np.frombuffer(zlib.decompress(cs[1][1]), np.uint8).reshape(19, -1)
        assert raw.shape[1] == 1 + 37 * (3 if rgb else 1) and bool((raw[:, 0] == code).all())
        if filt == "none":
            assert np.array_equal(raw[:, 1:].reshape(a.shape), a)


def test_refusals_by_name(fm):
    a = image(19, 37, True)
    data = bytearray(fm.encode_png(a))
    for at in (20, 60, len(data) - 2):  # a byte of IHDR, of IDAT, of IEND's CRC
        bad = bytearray(data)
        bad[at] ^= 0x10
        with pytest.raises(ValueError, match="CRC"):
            fm.decode_png(bytes(bad))
    with pytest.raises(ValueError, match="signature"):
        fm.decode_png(b"\x89PNX" + bytes(data[4:]))
    with pytest.raises(ValueError, match="truncated"):
        fm.decode_png(bytes(data[:-3]))
    row = lambda n: b"\x00" + bytes(n)
    with pytest.raises(ValueError, match="16-bit"):
        fm.decode_png(make_png(2, 2, 16, 2, 0, row(12) * 2))
    with pytest.raises(ValueError, match="palette"):
        fm.decode_png(make_png(2, 2, 8, 3, 0, row(2) * 2))
    with pytest.raises(ValueError, match="interlaced"):
        fm.decode_png(make_png(2, 2, 8, 2, 1, row(6) * 2))
    with pytest.raises(ValueError, match="1-bit"):
        fm.decode_png(make_png(8, 1, 1, 0, 0, row(1)))
    with pytest.raises(ValueError, match="grey with alpha"):
        fm.decode_png(make_png(2, 2, 8, 4, 0, row(4) * 2))
    with pytest.raises(ValueError, match="filter type 5"):
        fm.decode_png(make_png(2, 1, 8, 0, 0, b"\x05\x00\x00"))
    with pytest.raises(ValueError, match="bytes of image data"):
        fm.decode_png(make_png(2, 2, 8, 0, 0, row(2)))


def spec_filter(a, types):
    """Scanlines of `a` ([H,W,C] uint8) filtered row y with type types[y], by the definitions of the PNG specification (section 9), one byte at a time."""
    h, w, c = a.shape
    flat = a.reshape(h, w * c).astype(np.int32)
    out = bytearray()
    for y in range(h):
        t = types[y]
        out.append(t)
        for i in range(w * c):
            left = flat[y, i - c] if i >= c else 0
            up = flat[y - 1, i] if y else 0
            ul = flat[y - 1, i - c] if y and i >= c else 0
            if t == 4:
                p = left + up - ul
                pa, pb, pc = abs(p - left), abs(p - up), abs(p - ul)
                pred = left if pa <= pb and pa <= pc else (up if pb <= pc else ul)
            else:
                pred = (0, left, up, (left + up) // 2)[t]
            out.append((flat[y, i] - pred) & 0xFF)
    return bytes(out)


@pytest.mark.parametrize("channels,colour", [(1, 0), (3, 2), (4, 6)], ids=["grey", "rgb", "rgba"])
def test_reader_decodes_all_five_filter_types(fm, channels, colour):
    rng = np.random.default_rng(channels)
    for h, w in ((1, 1), (1, 17), (17, 1), (19, 37)):
        a = rng.integers(0, 256, (h, w, channels), dtype=np.uint8)
        a[:, ::3] = (a[:, ::3].astype(np.int32) // 16 * 16).astype(np.uint8)  # some structure, so that Paeth takes all three branches
        for types in ([t] * h for t in range(5)):
            got = fm.decode_png(make_png(w, h, 8, colour, 0, spec_filter(a, types)))
            assert np.array_equal(got, a[..., 0] if channels == 1 else a), (h, w, types[0])
        mixed = [(3 * y + 1) % 5 for y in range(h)]  # every type follows every other
        got = fm.decode_png(make_png(w, h, 8, colour, 0, spec_filter(a, mixed)))
        assert np.array_equal(got, a[..., 0] if channels == 1 else a), (h, w, "mixed")


def test_pillow_reads_our_files_and_we_read_pillows(fm):
    PIL_Image = pytest.importorskip("PIL.Image")
    seen = set()
    for h, w in SIZES + ((80, 90),):
        for rgb in (False, True):
            a = image(h, w, rgb)
            for filt in ("none", "sub", "up"):
                got = np.asarray(PIL_Image.open(io.BytesIO(fm.encode_png(a, 6, filt))))
                assert got.shape == a.shape and np.array_equal(got, a), (h, w, rgb, filt)
            for kw in ({}, {"optimize": True}, {"compress_level": 1}):
                f = io.BytesIO()
                PIL_Image.fromarray(a).save(f, "PNG", **kw)
                assert np.array_equal(fm.decode_png(f.getvalue()), a), (h, w, rgb, kw)
                raw = zlib.decompress(b"".join(b for k, b, _ in chunks(f.getvalue()) if k == b"IDAT"))
                seen |= set(np.frombuffer(raw, np.uint8).reshape(h, -1)[:, 0].tolist())
    smooth = np.add.outer(np.arange(64) ** 2 // 16, np.arange(96) * 2).astype(np.uint8)  # gradients: Pillow's adaptive choice picks average and Paeth rows
    for a in (smooth, np.stack([smooth, smooth[::-1], smooth[:, ::-1]], -1)):
        f = io.BytesIO()
        PIL_Image.fromarray(np.ascontiguousarray(a)).save(f, "PNG")
        assert np.array_equal(fm.decode_png(f.getvalue()), a)
        raw = zlib.decompress(b"".join(b for k, b, _ in chunks(f.getvalue()) if k == b"IDAT"))
        seen |= set(np.frombuffer(raw, np.uint8).reshape(a.shape[0], -1)[:, 0].tolist())
    print("filter types in Pillow's files:", sorted(seen))
    assert len(seen) >= 2  # (which types Pillow picks is its business; test_reader_decodes_all_five_filter_types covers every type)


def test_no_pil_import_in_the_package():
    import os

    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), PKG)
    for name in sorted(os.listdir(root)):
        if name.endswith(".py"):
            text = open(os.path.join(root, name)).read()
            assert "import PIL" not in text and "from PIL" not in text, name


def literal(x, rule):
    """The torch expressions the two rules restate, on the CPU."""
    if rule == "save":
        return x.mul(255).add(0.5).clamp(0, 255).to(torch.uint8)  # torchvision.utils.save_image
    return (x.clamp(0, 1) * 255).to(torch.uint8)  # format_image, render.py:303


def test_quantise_known_values(ev):
    q = lambda v, rule: int(ev.quantise(torch.tensor([v], dtype=torch.float32), rule)[0])
    assert q(0.5, "save") == 128 and q(0.5, "trunc") == 127
    assert q(0.0, "save") == 0 and q(1.0, "save") == 255 and q(0.0, "trunc") == 0 and q(1.0, "trunc") == 255
    for rule in ("save", "trunc"):
        # the specials, as csrc/frames.hip defines them: NaN -> 0 (a definition), +inf -> 255, -inf -> 0
        assert [q(v, rule) for v in (float("nan"), float("inf"), -float("inf"), -0.0, -0.3, 1.5, 1e30, 1e-40)] == [0, 255, 0, 0, 0, 255, 255, 0], rule
    with pytest.raises(ValueError, match="rule"):
        ev.quantise(torch.zeros(1), "round")
    out = ev.quantise(torch.rand(2, 3, 5, dtype=torch.float64), "save")
    assert out.dtype == torch.uint8 and out.shape == (2, 3, 5)


def test_quantise_equals_the_literal_expressions_at_every_threshold(ev):
    k = torch.arange(256, dtype=torch.float64)
    mids = torch.cat([((k + 0.5) / 255).to(torch.float32), (k / 255).to(torch.float32)])  # the thresholds of "save" and of "trunc"
    up = torch.nextafter(mids, torch.full_like(mids, 2.0))
    down = torch.nextafter(mids, torch.full_like(mids, -1.0))
    x = torch.cat([mids, up, down, torch.tensor([-0.0, -0.3, 1.5, 1e30, 1e-40, float("inf"), -float("inf")])])
    for rule in ("save", "trunc"):
        assert torch.equal(ev.quantise(x, rule), literal(x, rule)), rule
    # the thresholds are where they belong: (k + 0.5) / 255 is the first value of byte k + 1 under "save" up to the rounding of the fp32 product
    save = ev.quantise(torch.cat([down[:256], up[:256]]), "save").reshape(2, 256).to(torch.int64)
    assert bool((save[0] >= k.long()).all()) and bool((save[1] <= (k.long() + 1).clamp(max=255)).all()) and bool((save[1] - save[0] <= 1).all())
