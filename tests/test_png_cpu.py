"""CPU: the PNG contract's numpy restatement (tests/png_np.py) against PIL and zlib - lossless, a valid zlib stream, CRCs, Adler -
the coverage of the fixture set the GPU test compares bytes on, the length limiter, the size against zlib, the demo flag and the
argument errors that need no GPU."""
import ctypes as C
import functools
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_np, png_np

# Size of the restatement's IDAT data over zlib.compress(filtered stream, 1), measured: photo-like 120 x 168 0.928,
# gradient 120 x 168 1.450, rendered-like 120 x 168 0.930 (two segments each, about 160 bytes of code lengths per segment: that is what
# the small gradient file mostly consists of).  The bound per picture is the measured ratio rounded up to the next 0.05; the
# restatement is deterministic, the margin leaves room for later tuning.
ZLIB1_RATIO = {"photo": 0.95, "gradient": 1.50, "rendered": 0.95}


def chunks(data: bytes):
    """[(type, data)] of a PNG file; asserts the signature, that the chunks fill the file and every CRC."""
    assert data[:8] == png_np.SIGNATURE
    out, i = [], 8
    while i < len(data):
        n = struct.unpack(">I", data[i:i + 4])[0]
        kind, body = data[i + 4:i + 8], data[i + 8:i + 8 + n]
        assert struct.unpack(">I", data[i + 8 + n:i + 12 + n])[0] == zlib.crc32(kind + body), (kind, i)
        out.append((kind, body))
        i += 12 + n
    assert i == len(data)
    return out


def rendered_like(H=120, W=168):
    """A stand-in for a rendered frame that needs no GPU: a photo-like background with a shaded, flat-coloured disc over it."""
    img = png_np.photo_like(H, W, seed=3).astype(np.int64)
    y, x = np.mgrid[0:H, 0:W]
    r2 = (x - W // 2) ** 2 + (y - H // 2) ** 2
    disc = r2 < (H // 3) ** 2
    shade = 200 - (r2 * 90) // (H // 3) ** 2
    img[disc] = np.stack([shade, shade // 2, 60 + 0 * shade], -1)[disc]
    return np.clip(img, 0, 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def analysed():
    return [(name, img) + png_np.analyse(img) for name, img in png_np.fixture_set()]


def test_lossless_stream_crcs_adler_and_bound():
    for name, img, data, info in analysed():
        H, W = img.shape[:2]
        im = Image.open(io.BytesIO(data))
        assert im.format == "PNG" and im.mode == "RGB" and im.size == (W, H), name
        assert np.array_equal(np.asarray(im.convert("RGB")), img), name
        ch = chunks(data)
        nseg = -(-H * (1 + 3 * W) // png_np.SEGMENT)
        assert [k for k, _ in ch] == [b"IHDR"] + [b"IDAT"] * nseg + [b"IEND"], name
        assert ch[0][1] == struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0)
        idat = b"".join(b for k, b in ch if k == b"IDAT")
        filtered = info["filtered"].tobytes()
        assert len(filtered) == H * (1 + 3 * W)
        assert idat[:2] == b"\x78\x01" and zlib.decompress(idat) == filtered, name
        assert struct.unpack(">I", idat[-4:])[0] == zlib.adler32(filtered), name
        assert len(data) <= png_np.worst_case_bytes(H, W), name


def test_filter_choice_is_libpngs_heuristic():
    """The rows, re-filtered one by one in plain Python with every type: the chosen one has the smallest sum, the lowest on ties."""
    img = png_np.special(24, 40)
    filt, ftype, _ = png_np.filter_rows(img)
    rows = filt.reshape(24, 1 + 120)
    raw = img.reshape(24, 120).astype(int)
    for y in range(24):
        sums = []
        for t in range(5):
            tot = 0
            out = []
            for i in range(120):
                a = raw[y, i - 3] if i >= 3 else 0
                b = raw[y - 1, i] if y else 0
                c = raw[y - 1, i - 3] if y and i >= 3 else 0
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = [0, a, b, (a + b) // 2, a if pa <= pb and pa <= pc else (b if pb <= pc else c)][t]
                v = (raw[y, i] - pred) & 255
                out.append(v)
                tot += v if v < 128 else 256 - v
            sums.append((tot, t, out))
        best = min(sums)
        assert rows[y, 0] == ftype[y] == best[1] and rows[y, 1:].tolist() == best[2]


def test_fixture_set_covers_the_hard_cases():
    filters, ties = set(), 0
    m258 = d3 = drow = dhash = stored = nomatch = 0
    max_len = 0
    for name, img, data, info in analysed():
        W = img.shape[1]
        filters |= set(info["filters"].tolist())
        ties += len(info["ties"])
        for s in info["segments"]:
            stored += s["stored"]
            nomatch += s["matches"] == 0
            max_len = max(max_len, s["max_len"])
            for p, ln, d in s["tokens"]:
                if d:
                    assert 3 <= ln <= 258 and 1 <= d <= p
                    m258 += ln == 258
                    d3 += d == 3
                    drow += d == 1 + 3 * W
                    dhash += d not in (3, 1 + 3 * W)
    print(dict(filters=filters, ties=ties, m258=m258, d3=d3, drow=drow, dhash=dhash, stored=stored, nomatch=nomatch, max_len=max_len))
    assert filters == {0, 1, 2, 3, 4} and ties > 0
    assert m258 > 0 and d3 > 0 and drow > 0 and dhash > 0
    assert stored > 0 and nomatch > 0
    assert max_len == 15
    # the 2 x 11000 picture: a row is longer than a segment, the row-up candidate never lies inside one
    info = [i for n, _, _, i in analysed() if n == "special_2x11000"][0]
    assert not any(d == 1 + 3 * 11000 for s in info["segments"] for _, _, d in s["tokens"])
    # the noise is what falls back to stored blocks
    assert all(s["stored"] for n, _, _, i in analysed() if n.startswith("noise") for s in i["segments"])


def test_length_limiter():
    """A Fibonacci-like histogram asks for depths far above 15: after the repair every length is <= 15, 15 occurs, Kraft holds
    with equality and rarer symbols never have shorter codes."""
    fib = [1, 1]
    while len(fib) < 30:
        fib.append(fib[-1] + fib[-2])
    for counts in (fib, fib[:20] + [0, 0, 7] + fib[20:], [1] * 286, [3, 0, 0, 5], [0, 9]):
        lens = png_np.code_lengths(counts)
        used = [(c, l) for c, l in zip(counts, lens) if c]
        assert all(l == 0 for c, l in zip(counts, lens) if not c)
        assert all(1 <= l <= 15 for _, l in used)
        if len(used) > 1:
            assert sum(2 ** (15 - l) for _, l in used) == 2 ** 15, counts
        for (c1, l1) in used:
            for (c2, l2) in used:
                assert not (c1 < c2 and l1 < l2)
        codes = png_np.canonical_codes(lens)
        words = {format(c, "0%db" % l)[::-1] for c, l in zip(codes, lens) if l}
        assert len(words) == len(used) and not any(a != b and b.startswith(a) for a in words for b in words)
    assert max(png_np.code_lengths(fib)) == 15
    assert png_np.limit_counts([0, 0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2])[15] > 0
    assert png_np.code_lengths([5, 5]) == [1, 1] and png_np.code_lengths([0, 4, 0]) == [0, 1, 0]


def test_literals_only_switch():
    img = png_np.flat_picture(48, 64)
    data, info = png_np.analyse(img, lz=False)
    assert all(d == 0 for s in info["segments"] for _, _, d in s["tokens"])
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(data)).convert("RGB")), img)
    assert len(png_np.encode(img)) < len(data)


def test_long_matches_work():
    """The flat 240 x 320 picture codes to at most 3 % of its filtered stream (literals-only Huffman: 12.7 %, zlib level 1: 0.7 %)."""
    name, img, data, info = [a for a in analysed() if a[0] == "flat_240x320"][0]
    idat = sum(len(b) for k, b in chunks(data) if k == b"IDAT")
    print(f"flat 240x320: {idat} bytes of {info['filtered'].size} = {100.0 * idat / info['filtered'].size:.2f} %")
    assert idat <= 0.03 * info["filtered"].size


def test_size_against_zlib_level_1():
    pics = {"photo": png_np.photo_like(120, 168), "gradient": jpeg_np.fixture("gradient", 120, 168), "rendered": rendered_like()}
    for name, img in pics.items():
        data, info = png_np.analyse(img)
        idat = sum(len(b) for k, b in chunks(data) if k == b"IDAT")
        z1 = len(zlib.compress(info["filtered"].tobytes(), 1))
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, "PNG")
        print(f"{name}: IDAT {idat}, zlib level 1 {z1}, ratio {idat / z1:.3f}; file {len(data)}, PIL's {len(buf.getvalue())}, "
              f"ratio {len(data) / len(buf.getvalue()):.3f}")
        assert idat <= z1 * ZLIB1_RATIO[name], name


def test_encoder_argument_errors_without_gpu():
    """Bad sizes are refused before any GPU work, by the wrapper and by the C entries; the worst-case bound is the documented one."""
    from poco_amd import _lib, png
    from poco_amd._lib import PocoHipError, lib
    for h, w in ((0, 16), (16, 0), (16385, 16), (16, 16385)):
        with pytest.raises(PocoHipError, match="max_h, max_w"):
            png.PngEncoder(None, h, w)
    L = lib()
    syms = _lib.header_symbols()
    for s in ("poco_png_encoder_create", "poco_png_encode", "poco_png_encoder_destroy"):
        assert s in syms and hasattr(L, s), s
    assert "#define POCO_ABI_VERSION 4" in _lib.HEADER.read_text()
    L.poco_png_encoder_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    for a in ((0, 16), (16, 0), (16385, 16), (16, 16385)):
        assert L.poco_png_encoder_create(*a, C.byref(h)) == 1 and not h.value
        assert L.poco_last_error().startswith(b"poco_png_encoder_create") and b"max_h" in L.poco_last_error()
    assert L.poco_png_encoder_create(16, 16, None) == 1 and b"null" in L.poco_last_error()
    L.poco_png_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    fake = C.c_void_p(4096)                                  # never dereferenced: refused before a pointer is used
    assert L.poco_png_encode(None, fake, 16, 16, fake, 1 << 20, fake, None) == 1
    assert L.poco_last_error().startswith(b"poco_png_encode") and b"null" in L.poco_last_error()
    L.poco_png_encoder_destroy.argtypes = [C.c_void_p]
    L.poco_png_encoder_destroy.restype = None
    L.poco_png_encoder_destroy(None)
    assert png.worst_case_bytes(1080, 1920) == png_np.worst_case_bytes(1080, 1920) == 51 + 1080 * 5761 + 22 * 190
    assert png.worst_case_bytes(1, 1) == 51 + 4 + 22 and png.SEGMENT == png_np.SEGMENT


def test_demo_flag():
    import demo
    base = ["--cfg", "c.yaml", "--ckpt", "x.pt"]
    a = demo.parse_args(base)
    assert a.encode == "host" and a.image_format == "png"
    a = demo.parse_args(base + ["--encode", "gpu"])
    assert a.encode == "gpu"
    a = demo.parse_args(base + ["--encode", "gpu", "--image_format", "jpg"])          # not an error: jpg ignores the flag
    assert a.encode == "gpu" and a.image_format == "jpg"
    with pytest.raises(SystemExit):
        demo.parse_args(base + ["--encode", "fpga"])
