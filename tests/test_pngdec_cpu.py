"""CPU: the PNG decoder's numpy restatement (tests/pngdec_np.py) against zlib and PIL on the fixture set the GPU test compares bytes
on (every fixture is made here from a seed; the stats prove each is what its name says), what parse_png declines, the damaged
streams and their statuses, the exported symbols and the demo flag."""
import functools
import io
import struct
import zlib

import numpy as np
import pytest
from PIL import Image

from poco_amd import _lib
from poco_amd.png import parse_png
from tests import png_np, pngdec_np
from tests.test_jpeg_cpu import photo_like
from tests.test_png_cpu import rendered_like

SIG = b"\x89PNG\r\n\x1a\n"
BPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}


def chunk(kind: bytes, data: bytes, bad_crc: bool = False) -> bytes:
    crc = zlib.crc32(kind + data) ^ (1 if bad_crc else 0)
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", crc)


def filter_stream(px: np.ndarray, bpp: int, filters) -> bytes:
    """The filtered stream of uint8 [H, W * bpp] rows with filter type filters[y % len(filters)] on row y."""
    H, stride = px.shape
    rows = px.astype(np.int64)
    out = bytearray()
    prev = np.zeros(stride, np.int64)
    for y in range(H):
        ft, line = filters[y % len(filters)], rows[y]
        a = np.concatenate([np.zeros(bpp, np.int64), line[:-bpp]]) if stride > bpp else np.zeros(stride, np.int64)
        c = np.concatenate([np.zeros(bpp, np.int64), prev[:-bpp]]) if stride > bpp else np.zeros(stride, np.int64)
        if ft == 0:
            p = 0
        elif ft == 1:
            p = a
        elif ft == 2:
            p = prev
        elif ft == 3:
            p = (a + prev) >> 1
        elif ft == 4:
            pa, pb, pc = np.abs(prev - c), np.abs(a - c), np.abs(a + prev - 2 * c)
            p = np.where((pa <= pb) & (pa <= pc), a, np.where(pb <= pc, prev, c))
        else:
            p = 0                       # a filter byte the format does not know: the bytes are stored as they are
        out.append(ft)
        out += ((line - p) & 255).astype(np.uint8).tobytes()
        prev = line
    return bytes(out)


def assemble(H, W, colour_type, zdata: bytes, idat=None, extra=(), palette=None, between=None, depth=8, interlace=0, iend=True,
             bad_idat_crc=False) -> bytes:
    """A PNG file around the zlib data: IHDR, PLTE, the extra chunks, IDAT chunks of the sizes `idat` (the last size repeats),
    `between` after the first IDAT chunk, IEND."""
    out = SIG + chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, depth, colour_type, 0, 0, interlace))
    if palette is not None:
        out += chunk(b"PLTE", bytes(palette))
    for kind, data in extra:
        out += chunk(kind, data)
    sizes, pos, k = list(idat or [len(zdata)]), 0, 0
    first = True
    while pos < len(zdata) or first:
        n = sizes[min(k, len(sizes) - 1)]
        out += chunk(b"IDAT", zdata[pos:pos + n], bad_crc=bad_idat_crc and first)
        if first and between is not None:
            out += chunk(*between)
        first = False
        pos += n
        k += 1
    return out + (chunk(b"IEND", b"") if iend else b"")


def make_png(pixels, colour_type, filters=(0,), zlib_args=None, idat=None, extra=(), palette=None, flush_rows=False, **kw) -> bytes:
    """A PNG written by hand: a chosen filter type per row, chosen zlib.compressobj parameters (level, wbits, strategy; flush_rows:
    Z_FULL_FLUSH after every row), chosen IDAT split points, extra chunks."""
    bpp = BPP[colour_type]
    px = np.asarray(pixels, np.uint8)
    H, W = px.shape[:2]
    raw = filter_stream(px.reshape(H, W * bpp), bpp, list(filters))
    z = dict(level=6, wbits=15, strategy=zlib.Z_DEFAULT_STRATEGY)
    z.update(zlib_args or {})
    co = zlib.compressobj(z["level"], zlib.DEFLATED, z["wbits"], 9, z["strategy"])
    stride = 1 + W * bpp
    if flush_rows:
        zdata = b"".join(co.compress(raw[y * stride:(y + 1) * stride]) + co.flush(zlib.Z_FULL_FLUSH) for y in range(H)) + co.flush()
    else:
        zdata = co.compress(raw) + co.flush()
    return assemble(H, W, colour_type, zdata, idat, extra, palette, **kw)


def from_stream(H, W, colour_type, stream: bytes, raw: bytes = b"", **kw) -> bytes:
    """A PNG around a raw deflate stream that inflates to `raw` (zlib header 78 01 and the Adler-32 of `raw`)."""
    return assemble(H, W, colour_type, b"\x78\x01" + stream + struct.pack(">I", zlib.adler32(raw)), **kw)


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):              # LSB first
        self.acc |= v << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 255)
            self.acc >>= 8
            self.n -= 8

    def code(self, v, n):              # a Huffman code: MSB first
        self.bits(int(format(v, f"0{n}b")[::-1], 2), n)

    def fixed_lit(self, s):
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def fixed_match(self, ln, dist):
        ls, (lb, le) = next((i, t) for i, t in reversed(list(enumerate(pngdec_np._LEN))) if t[0] <= ln and (i == 28) == (ln == 258))
        self.fixed_lit(257 + ls)
        self.bits(ln - lb, le)
        ds, (db, de) = next((i, t) for i, t in reversed(list(enumerate(pngdec_np._DIST))) if t[0] <= dist)
        self.code(ds, 5)
        self.bits(dist - db, de)

    def done(self) -> bytes:
        if self.n:
            self.bits(0, 8 - self.n)
        return bytes(self.out)


def pil_png(img, **kw) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "PNG", **kw)
    return buf.getvalue()


def period_32768() -> bytes:
    """260 x 255 grey, filter 0: rows repeat after 128, so the filtered stream (256 bytes per row) has period exactly 32 768.  One
    stored block carries the first period, a fixed-Huffman block the rest as matches of distance 32 768 (zlib itself never reaches
    back further than 32 506)."""
    rng = np.random.default_rng(77)
    px = np.tile(rng.integers(0, 256, (128, 255), dtype=np.uint8), (3, 1))[:260]
    raw = filter_stream(px, 1, [0])
    w = BitWriter()
    w.bits(0, 3)
    w.bits(0, 5)
    w.out += struct.pack("<HH", 32768, 32768 ^ 0xFFFF) + raw[:32768]
    w.bits(1, 1)
    w.bits(1, 2)
    left = len(raw) - 32768
    while left:
        ln = 258 if left >= 261 or left == 258 else min(left, 255) if left > 258 else left
        w.fixed_match(ln, 32768)
        left -= ln
    w.fixed_lit(256)
    return from_stream(260, 255, 0, w.done(), raw)


@functools.lru_cache(maxsize=None)
def fixture_set():
    """{name: the bytes of a .png file}"""
    rng = np.random.default_rng(5)
    photo = photo_like(120, 168, 11)
    fs = {}
    fs["1x1_rgb"] = make_png(rng.integers(0, 256, (1, 1, 3), dtype=np.uint8), 2, filters=[4])
    fs["1x7_grey"] = make_png(rng.integers(0, 256, (1, 7), dtype=np.uint8), 0, filters=[3])
    fs["7x1_rgba"] = make_png(rng.integers(0, 256, (7, 1, 4), dtype=np.uint8), 6, filters=[4, 3, 1, 2, 0])
    small = photo_like(17, 33, 3)
    for k in range(5):
        fs[f"17x33_filters_from{k}"] = make_png(small, 2, filters=[(k + i) % 5 for i in range(5)])
    fs["120x168_pil_default"] = pil_png(photo)
    fs["120x168_pil_level0_stored"] = pil_png(photo, compress_level=0)
    fs["120x168_pil_level9_optimize"] = pil_png(photo, compress_level=9, optimize=True)
    fs["120x168_fixed"] = make_png(photo, 2, filters=[4], zlib_args=dict(strategy=zlib.Z_FIXED))
    fs["120x168_rle"] = make_png(photo, 2, filters=[1], zlib_args=dict(strategy=zlib.Z_RLE))
    fs["120x168_huffman_only"] = make_png(photo, 2, filters=[4], zlib_args=dict(strategy=zlib.Z_HUFFMAN_ONLY))
    fs["120x168_wbits9"] = make_png(photo, 2, filters=[1, 4], zlib_args=dict(wbits=9))
    fs["120x168_flush_split"] = make_png(photo, 2, filters=[4, 2], flush_rows=True, idat=[1] * 64 + [0] + [8192])
    fs["240x320_flat_len258"] = pil_png(png_np.flat_picture(240, 320))
    fs["260x255_period32768"] = period_32768()
    fs["96x700_long"] = pil_png(photo_like(96, 700, 13))
    pal = rng.integers(0, 256, 15, dtype=np.uint8).tobytes()
    fs["40x50_palette_trns"] = make_png(rng.integers(0, 5, (40, 50), dtype=np.uint8), 3, filters=[0, 1], palette=pal,
                                        extra=[(b"tRNS", bytes([0, 128, 255]))])
    fs["33x20_grey_alpha"] = make_png(rng.integers(0, 256, (33, 20, 2), dtype=np.uint8), 4, filters=[4, 3])
    fs["30x41_rgb_trns_gama_text"] = make_png(photo_like(30, 41, 8), 2, filters=[2, 4],
                                              extra=[(b"gAMA", struct.pack(">I", 45455)), (b"tRNS", bytes(6)),
                                                     (b"tEXt", b"Comment\0made by hand")])
    fs["120x168_own_encoder"] = png_np.encode(rendered_like())
    return fs


@functools.lru_cache(maxsize=None)
def restated(name):
    return pngdec_np.decode(fixture_set()[name])


def pil_rgb(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def zdata_of(data: bytes) -> bytes:
    info = parse_png(data)
    return b"".join(info.data[o:o + l] for o, l in info.idat)


@functools.lru_cache(maxsize=None)
def damaged_set():
    """{name: (the bytes of a .png file parse_png accepts, zlib.decompress must raise)}: every one a non-zero status."""
    ds = {}
    H, W = 4, 4                                                  # grey: 20 bytes of filtered stream
    w = BitWriter()
    w.bits(1, 1); w.bits(1, 2); w.fixed_lit(0); w.fixed_lit(7); w.fixed_match(18, 5); w.fixed_lit(256)
    ds["distance_beyond_output"] = (from_stream(H, W, 0, w.done()), True)
    ds["stored_len_nlen"] = (from_stream(H, W, 0, b"\x01" + struct.pack("<HH", 20, 20) + bytes(20)), True)
    ds["block_type_3"] = (from_stream(H, W, 0, b"\x07" + bytes(24)), True)
    w = BitWriter()                                              # HLIT 257, HDIST 1, code-length code {0: 1 bit, 1: 1 bit}
    w.bits(1, 1); w.bits(2, 2); w.bits(0, 5); w.bits(0, 5); w.bits(14, 4)
    for sym in pngdec_np._CL_ORDER[:18]:
        w.bits(1 if sym in (0, 1) else 0, 3)
    for _ in range(258):
        w.code(1, 1)                                             # every symbol one bit long: over-subscribed
    w.bits(0, 32)
    ds["oversubscribed_lengths"] = (from_stream(H, W, 0, w.done()), True)
    w = BitWriter()                                              # code-length code {0: 1 bit, 8: 1 bit}; 256 literals of 8 bits, no 256
    w.bits(1, 1); w.bits(2, 2); w.bits(0, 5); w.bits(0, 5); w.bits(1, 4)
    for sym in pngdec_np._CL_ORDER[:5]:
        w.bits(1 if sym in (0, 8) else 0, 3)
    for _ in range(256):
        w.code(1, 1)
    w.code(0, 1); w.code(0, 1)
    w.bits(0, 32)
    ds["no_end_of_block"] = (from_stream(H, W, 0, w.done()), True)
    w = BitWriter()
    w.bits(1, 1); w.bits(1, 2); w.fixed_lit(0); w.fixed_lit(286); w.bits(0, 16); w.fixed_lit(256)
    ds["symbol_286"] = (from_stream(H, W, 0, w.done()), True)
    src = fixture_set()["120x168_pil_default"]
    z = zdata_of(src)
    ds["cut_at_half"] = (assemble(120, 168, 2, z[:len(z) // 2]), False)
    photo = photo_like(120, 168, 11)
    raw = filter_stream(photo.reshape(120, 168 * 3), 3, [4])
    ds["one_row_short"] = (assemble(120, 168, 2, zlib.compress(raw[:-(1 + 168 * 3)])), False)
    ds["one_byte"] = (from_stream(H, W, 0, b"\x03"), False)
    ds["filter_byte_5"] = (make_png(photo_like(17, 33, 3), 2, filters=[4, 5, 1]), False)
    return ds


def test_restatement_equals_zlib_and_pil():
    for name, data in fixture_set().items():
        info = parse_png(data)
        assert info is not None, name
        z = b"".join(data[o:o + l] for o, l in info.idat)
        assert info.stream_length == len(z) - 6, name
        raw, st, _ = pngdec_np.inflate(pngdec_np.stream_of(info))
        assert st == 0 and raw == zlib.decompress(z), name
        rgb, st, _ = restated(name)
        assert st == 0 and np.array_equal(rgb, pil_rgb(data)), name


def test_fixtures_are_what_their_names_say():
    fs = fixture_set()
    st = {n: restated(n)[2] for n in fs}
    infos = {n: parse_png(d) for n, d in fs.items()}
    assert (infos["1x1_rgb"].height, infos["1x7_grey"].width, infos["7x1_rgba"].height) == (1, 7, 7)
    assert st["120x168_pil_level0_stored"]["block_types"] == {0} and st["120x168_pil_level0_stored"]["blocks"] > 1
    assert 2 in st["120x168_pil_default"]["block_types"] and 2 in st["120x168_pil_level9_optimize"]["block_types"]
    assert st["120x168_fixed"]["block_types"] == {1}
    assert st["120x168_rle"]["overlap"] and st["120x168_rle"]["max_dist"] == 1
    assert st["120x168_huffman_only"]["matches"] == 0
    assert zdata_of(fs["120x168_wbits9"])[0] >> 4 == 1 and st["120x168_wbits9"]["max_dist"] <= 512
    split = infos["120x168_flush_split"].idat
    assert [l for _, l in split[:66]] == [1] * 64 + [0, 8192] and st["120x168_flush_split"]["blocks"] >= 240
    assert st["240x320_flat_len258"]["max_len"] == 258
    assert st["260x255_period32768"]["max_dist"] == 32768
    assert infos["96x700_long"].height * (1 + 3 * 700) > 2 * 65536
    assert infos["40x50_palette_trns"].colour_type == 3 and infos["40x50_palette_trns"].palette[15:] == bytes(768 - 15)
    assert infos["33x20_grey_alpha"].colour_type == 4 and infos["30x41_rgb_trns_gama_text"].colour_type == 2
    assert {i.colour_type for i in infos.values()} == {0, 2, 3, 4, 6}
    first_rows = {pngdec_np.inflate(pngdec_np.stream_of(infos[f"17x33_filters_from{k}"]))[0][0] for k in range(5)}
    assert first_rows == {0, 1, 2, 3, 4}


def test_parse_png_declines():
    photo = photo_like(24, 32, 2)
    good = pil_png(photo)
    z = zdata_of(good)
    assert parse_png(good) is not None
    grey16 = (np.arange(24 * 32, dtype=np.uint16).reshape(24, 32) * 80)
    buf = io.BytesIO()
    Image.fromarray(grey16).save(buf, "PNG")
    declined = {"16-bit": buf.getvalue()}
    for bits in (1, 2, 4):
        declined[f"{bits}-bit"] = assemble(24, 32, 0, zlib.compress(bytes(24 * (1 + 32 * bits // 8))), depth=bits)
    buf = io.BytesIO()
    Image.fromarray(photo).save(buf, "PNG")
    declined["interlaced"] = assemble(24, 32, 2, z, interlace=1)
    declined["acTL"] = assemble(24, 32, 2, z, extra=[(b"acTL", struct.pack(">II", 1, 0))])
    declined["idat_crc"] = assemble(24, 32, 2, z, bad_idat_crc=True)
    declined["fdict"] = assemble(24, 32, 2, bytes([0x78, 0x20 | (31 - (0x78 * 256 + 0x20) % 31)]) + z[2:])
    declined["fcheck"] = assemble(24, 32, 2, bytes([z[0], z[1] ^ 1]) + z[2:])
    declined["idat_not_consecutive"] = assemble(24, 32, 2, z, idat=[len(z) // 2], between=(b"tEXt", b"k\0v"))
    declined["no_iend"] = assemble(24, 32, 2, z, iend=False)
    declined["cut_in_chunk"] = good[:len(good) - 20]
    jpg = io.BytesIO()
    Image.fromarray(photo).save(jpg, "JPEG")
    declined["jpeg"] = jpg.getvalue()
    declined["short_idat"] = assemble(24, 32, 2, b"\x78\x01\x03\0\0")
    declined["palette_without_plte"] = assemble(24, 32, 3, z)
    assert (0x78 * 256 + declined["fdict"][8 + 25 + 8 + 1]) % 31 == 0
    for name, data in declined.items():
        assert parse_png(data) is None, name
    for cut in range(0, len(good), 7):
        parse_png(good[:cut])                                    # never raises


def test_damaged_streams_get_a_status():
    for name, (data, zlib_raises) in damaged_set().items():
        info = parse_png(data)
        assert info is not None, name
        rgb, st, _ = pngdec_np.decode(info)
        assert st != 0 and rgb is None, name
        if zlib_raises:
            with pytest.raises(zlib.error):
                zlib.decompress(zdata_of(data))
    assert list(damaged_set())[:6] == ["distance_beyond_output", "stored_len_nlen", "block_type_3", "oversubscribed_lengths",
                                       "no_end_of_block", "symbol_286"]
    assert [zr for _, zr in damaged_set().values()][:6] == [True] * 6


def test_symbols_are_declared_and_exported():
    syms = _lib.header_symbols()
    L = _lib.lib()
    for s in ("poco_png_decoder_create", "poco_png_decode", "poco_png_decoder_destroy"):
        assert s in syms and hasattr(L, s), s
    assert "#define POCO_ABI_VERSION 4" in _lib.HEADER.read_text()


def test_demo_flag():
    import demo
    base = ["--cfg", "c.yaml", "--ckpt", "x.pt"]
    assert demo.parse_args(base).decode_png == "host"
    assert demo.parse_args(base + ["--decode_png", "gpu"]).decode_png == "gpu"
    with pytest.raises(SystemExit):
        demo.parse_args(base + ["--decode_png", "both"])
