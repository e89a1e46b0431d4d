"""Numpy restatement of the baseline JPEG encoder contract of csrc/jpeg_enc.hip (include/poco_hip.h): integer
arithmetic only, so the device must produce these BYTES, not merely similar pixels.

    encode(rgb uint8 [H,W,3], quality=90) -> bytes            encode_stats(...) -> (bytes, coverage statistics)

Baseline sequential (SOF0), 8 bit, YCbCr 4:2:0, JFIF.  Colour conversion, h2v2 downsampling, the "islow" forward DCT, quality
scaling and quantisation are libjpeg's integer forms (jccolor.c, jcsample.c, jfdctint.c, jcparam.c, jcdctmgr.c); the four Huffman
tables are Annex K's; one restart interval per MCU row.  Images are padded by edge replication to whole 16x16 MCUs."""
from __future__ import annotations

import numpy as np

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                   28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                   54, 47, 55, 62, 63])                     # zigzag position -> natural (row-major) index

QUANT_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                       14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                       49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
QUANT_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                         47, 66, 99, 99, 99, 99, 99, 99] + [99] * 32)

DC_LUMA_BITS = [0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0]
DC_CHROMA_BITS = [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0]
DC_VALS = list(range(12))
AC_LUMA_BITS = [0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D]
AC_LUMA_VALS = [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81,
    0x91, 0xA1, 0x08, 0x23, 0x42, 0xB1, 0xC1, 0x15, 0x52, 0xD1, 0xF0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0A, 0x16, 0x17, 0x18,
    0x19, 0x1A, 0x25, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48,
    0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74, 0x75,
    0x76, 0x77, 0x78, 0x79, 0x7A, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99,
    0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA, 0xC2, 0xC3,
    0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE1, 0xE2, 0xE3, 0xE4, 0xE5,
    0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF1, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]
AC_CHROMA_BITS = [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77]
AC_CHROMA_VALS = [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08,
    0x14, 0x42, 0x91, 0xA1, 0xB1, 0xC1, 0x09, 0x23, 0x33, 0x52, 0xF0, 0x15, 0x62, 0x72, 0xD1, 0x0A, 0x16, 0x24, 0x34, 0xE1, 0x25,
    0xF1, 0x17, 0x18, 0x19, 0x1A, 0x26, 0x27, 0x28, 0x29, 0x2A, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3A, 0x43, 0x44, 0x45, 0x46, 0x47,
    0x48, 0x49, 0x4A, 0x53, 0x54, 0x55, 0x56, 0x57, 0x58, 0x59, 0x5A, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6A, 0x73, 0x74,
    0x75, 0x76, 0x77, 0x78, 0x79, 0x7A, 0x82, 0x83, 0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8A, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97,
    0x98, 0x99, 0x9A, 0xA2, 0xA3, 0xA4, 0xA5, 0xA6, 0xA7, 0xA8, 0xA9, 0xAA, 0xB2, 0xB3, 0xB4, 0xB5, 0xB6, 0xB7, 0xB8, 0xB9, 0xBA,
    0xC2, 0xC3, 0xC4, 0xC5, 0xC6, 0xC7, 0xC8, 0xC9, 0xCA, 0xD2, 0xD3, 0xD4, 0xD5, 0xD6, 0xD7, 0xD8, 0xD9, 0xDA, 0xE2, 0xE3, 0xE4,
    0xE5, 0xE6, 0xE7, 0xE8, 0xE9, 0xEA, 0xF2, 0xF3, 0xF4, 0xF5, 0xF6, 0xF7, 0xF8, 0xF9, 0xFA]


def fix(x: float, bits: int) -> int:
    return int(x * (1 << bits) + 0.5)


def quant_tables(quality: int):
    """(luma, chroma) int [64] in natural order: jpeg_quality_scaling + jpeg_add_quant_table with force_baseline."""
    if not 1 <= int(quality) <= 100:
        raise ValueError("quality must be in 1..100")
    q = int(quality)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return tuple(np.clip((t * scale + 50) // 100, 1, 255) for t in (QUANT_LUMA, QUANT_CHROMA))


def huff_codes(bits, vals):
    """{symbol: (code, length)} of a DHT (Annex C canonical codes)."""
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


def rgb_to_ycc(rgb: np.ndarray):
    """jccolor.c rgb_ycc_convert: SCALEBITS = 16."""
    r, g, b = (rgb[..., i].astype(np.int64) for i in range(3))
    half, off = 1 << 15, 128 << 16
    y = (fix(0.29900, 16) * r + fix(0.58700, 16) * g + fix(0.11400, 16) * b + half) >> 16
    cb = (-fix(0.16874, 16) * r - fix(0.33126, 16) * g + fix(0.50000, 16) * b + off + half - 1) >> 16
    cr = (fix(0.50000, 16) * r - fix(0.41869, 16) * g - fix(0.08131, 16) * b + off + half - 1) >> 16
    return y, cb, cr


def downsample_h2v2(c: np.ndarray) -> np.ndarray:
    """jcsample.c h2v2_downsample: 2x2 box sum, bias 1, 2, 1, 2 ... along each output row, >> 2."""
    s = c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2]
    bias = 1 + (np.arange(s.shape[1]) & 1)
    return (s + bias[None, :]) >> 2


_C = {k: fix(v, 13) for k, v in dict(c0_298=0.298631336, c0_390=0.390180644, c0_541=0.541196100, c0_765=0.765366865,
                                     c0_899=0.899976223, c1_175=1.175875602, c1_501=1.501321110, c1_847=1.847759065,
                                     c1_961=1.961570560, c2_053=2.053119869, c2_562=2.562915447, c3_072=3.072711026).items()}


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _dct_1d(d, first: bool):
    """One pass of jfdctint.c over the last axis of d [..., 8]."""
    t0, t7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    t1, t6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    t2, t5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    t3, t4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    n = 13 - 2 if first else 13 + 2
    out = [None] * 8
    out[0] = (t10 + t11) << 2 if first else _descale(t10 + t11, 2)
    out[4] = (t10 - t11) << 2 if first else _descale(t10 - t11, 2)
    z1 = (t12 + t13) * _C["c0_541"]
    out[2] = _descale(z1 + t13 * _C["c0_765"], n)
    out[6] = _descale(z1 - t12 * _C["c1_847"], n)
    z1, z2, z3, z4 = t4 + t7, t5 + t6, t4 + t6, t5 + t7
    z5 = (z3 + z4) * _C["c1_175"]
    t4, t5, t6, t7 = t4 * _C["c0_298"], t5 * _C["c2_053"], t6 * _C["c3_072"], t7 * _C["c1_501"]
    z1, z2 = -z1 * _C["c0_899"], -z2 * _C["c2_562"]
    z3, z4 = -z3 * _C["c1_961"] + z5, -z4 * _C["c0_390"] + z5
    out[7] = _descale(t4 + z1 + z3, n)
    out[5] = _descale(t5 + z2 + z4, n)
    out[3] = _descale(t6 + z2 + z3, n)
    out[1] = _descale(t7 + z1 + z4, n)
    return np.stack(out, -1)


def fdct_islow(blocks: np.ndarray) -> np.ndarray:
    """blocks int [N,8,8] (level-shifted samples) -> coefficients scaled by 8, natural order."""
    p1 = _dct_1d(blocks.astype(np.int64), True)                      # rows
    return np.swapaxes(_dct_1d(np.swapaxes(p1, 1, 2), False), 1, 2)   # columns


def quantize(coef: np.ndarray, qtab: np.ndarray) -> np.ndarray:
    """jcdctmgr.c forward_DCT: divide by 8 q, round to nearest, ties away from zero.  coef [N,8,8], qtab [64] natural."""
    qv = (qtab.reshape(8, 8).astype(np.int64) << 3)[None]
    mag = (np.abs(coef) + (qv >> 1)) // qv
    return np.where(coef < 0, -mag, mag)


def _blocks(plane: np.ndarray) -> np.ndarray:
    """[h,w] -> [h/8, w/8, 8, 8]"""
    h, w = plane.shape
    return plane.reshape(h // 8, 8, w // 8, 8).swapaxes(1, 2)


def coefficients(rgb: np.ndarray, quality: int) -> np.ndarray:
    """Quantised coefficients int16 [mcu_rows, mcu_cols, 6, 64] in zigzag order, blocks Y00 Y01 Y10 Y11 Cb Cr: the device's
    scratch layout after step 1."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3 and rgb.shape[0] >= 1 and rgb.shape[1] >= 1
    H, W = rgb.shape[:2]
    my, mx = (H + 15) // 16, (W + 15) // 16
    pad = np.pad(rgb, ((0, my * 16 - H), (0, mx * 16 - W), (0, 0)), mode="edge")
    y, cb, cr = rgb_to_ycc(pad)
    ql, qc = quant_tables(quality)
    out = np.empty((my, mx, 6, 64), np.int16)
    yb = quantize(fdct_islow(_blocks(y - 128).reshape(-1, 8, 8)), ql).reshape(my, 2, mx, 2, 64)
    out[:, :, :4] = yb.transpose(0, 2, 1, 3, 4).reshape(my, mx, 4, 64)[..., ZIGZAG]
    for k, c in ((4, cb), (5, cr)):
        out[:, :, k] = quantize(fdct_islow(_blocks(downsample_h2v2(c) - 128).reshape(-1, 8, 8)), qc).reshape(my, mx, 64)[..., ZIGZAG]
    return out


def _segment(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def header(H: int, W: int, quality: int) -> bytes:
    """SOI, APP0 (JFIF 1.01, density 1:1), DQT x2, SOF0, DHT x4, DRI, SOS."""
    ql, qc = quant_tables(quality)
    mx = (W + 15) // 16
    h = b"\xff\xd8" + _segment(0xE0, b"JFIF\0" + bytes([1, 1, 0, 0, 1, 0, 1, 0, 0]))
    h += _segment(0xDB, bytes([0]) + bytes(ql[ZIGZAG].tolist())) + _segment(0xDB, bytes([1]) + bytes(qc[ZIGZAG].tolist()))
    h += _segment(0xC0, bytes([8]) + H.to_bytes(2, "big") + W.to_bytes(2, "big") + bytes([3, 1, 0x22, 0, 2, 0x11, 1, 3, 0x11, 1]))
    for tc_th, bits, vals in ((0x00, DC_LUMA_BITS, DC_VALS), (0x10, AC_LUMA_BITS, AC_LUMA_VALS),
                              (0x01, DC_CHROMA_BITS, DC_VALS), (0x11, AC_CHROMA_BITS, AC_CHROMA_VALS)):
        h += _segment(0xC4, bytes([tc_th]) + bytes(bits) + bytes(vals))
    h += _segment(0xDD, mx.to_bytes(2, "big"))
    h += _segment(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return h


def _category(v: int) -> int:
    return int(abs(v)).bit_length()


def encode_stats(rgb: np.ndarray, quality: int = 90):
    """(bytes, stats): stats = {"zrl", "eob", "eob_only_blocks", "stuffed", "max_category", "intervals", "max_interval_blocks"}."""
    rgb = np.asarray(rgb)
    coef = coefficients(rgb, quality)
    H, W = rgb.shape[:2]
    my, mx = coef.shape[:2]
    dc = (huff_codes(DC_LUMA_BITS, DC_VALS), huff_codes(DC_CHROMA_BITS, DC_VALS))
    ac = (huff_codes(AC_LUMA_BITS, AC_LUMA_VALS), huff_codes(AC_CHROMA_BITS, AC_CHROMA_VALS))
    st = {"zrl": 0, "eob": 0, "eob_only_blocks": 0, "stuffed": 0, "max_category": 0, "intervals": my, "max_interval_blocks": mx * 6}
    out = bytearray(header(H, W, quality))
    for r in range(my):
        acc, nbits = 0, 0
        pred = [0, 0, 0]                                   # every interval starts with DC predictors 0
        for m in range(mx):
            for k in range(6):
                comp = 0 if k < 4 else k - 3
                tab = 0 if k < 4 else 1
                blk = coef[r, m, k].tolist()
                diff = blk[0] - pred[comp]
                pred[comp] = blk[0]
                s = _category(diff)
                st["max_category"] = max(st["max_category"], s)
                code, ln = dc[tab][s]
                acc, nbits = (acc << ln) | code, nbits + ln
                if s:
                    acc, nbits = (acc << s) | ((diff if diff > 0 else diff - 1) & ((1 << s) - 1)), nbits + s
                run = 0
                for v in blk[1:]:
                    if v == 0:
                        run += 1
                        continue
                    while run > 15:
                        code, ln = ac[tab][0xF0]
                        acc, nbits = (acc << ln) | code, nbits + ln
                        run -= 16
                        st["zrl"] += 1
                    s = _category(v)
                    assert s <= 10
                    st["max_category"] = max(st["max_category"], s)
                    code, ln = ac[tab][(run << 4) | s]
                    acc, nbits = (acc << ln) | code, nbits + ln
                    acc, nbits = (acc << s) | ((v if v > 0 else v - 1) & ((1 << s) - 1)), nbits + s
                    run = 0
                if run:
                    code, ln = ac[tab][0x00]
                    acc, nbits = (acc << ln) | code, nbits + ln
                    st["eob"] += 1
                    st["eob_only_blocks"] += run == 63
        fill = -nbits % 8
        acc, nbits = (acc << fill) | ((1 << fill) - 1), nbits + fill
        raw = acc.to_bytes(nbits // 8, "big")
        st["stuffed"] += raw.count(b"\xff")
        out += raw.replace(b"\xff", b"\xff\x00")
        out += bytes([0xFF, 0xD0 + (r & 7)]) if r < my - 1 else b"\xff\xd9"
    return bytes(out), st


def encode(rgb: np.ndarray, quality: int = 90) -> bytes:
    return encode_stats(rgb, quality)[0]


def worst_case_bytes(H: int, W: int) -> int:
    """The out_cap poco_jpeg_encode asks for: header + per interval (27 bits per coefficient, doubled by stuffing) + marker."""
    my, mx = (H + 15) // 16, (W + 15) // 16
    return len(header(H, W, 90)) + my * (mx * 6 * 432 + 2)


# ---- the fixture set of tests/test_jpeg_gpu.py (its coverage is asserted in tests/test_jpeg_cpu.py) ---------------------------
FIXTURE_SHAPES = [(16, 16), (8, 8), (33, 17), (40, 56), (160, 48), (48, 208)]
FIXTURE_FILLS = ["noise", "white", "black", "gradient", "checker"]
FIXTURE_QUALITIES = [50, 100]


def fixture(fill: str, H: int, W: int) -> np.ndarray:
    """uint8 [H,W,3]: uniform noise, all 255, all 0, a horizontal gradient, a saturated-colour checkerboard of period 3."""
    if fill == "noise":
        return np.random.default_rng(1000 * H + W).integers(0, 256, (H, W, 3), dtype=np.uint8)
    if fill == "white":
        return np.full((H, W, 3), 255, np.uint8)
    if fill == "black":
        return np.zeros((H, W, 3), np.uint8)
    if fill == "gradient":
        g = (np.arange(W) * 255 // max(W - 1, 1)).astype(np.uint8)
        return np.ascontiguousarray(np.broadcast_to(g[None, :, None], (H, W, 3)))
    if fill == "checker":
        y, x = np.mgrid[0:H, 0:W]
        k = ((y // 3) + (x // 3)) % 3
        cols = np.array([[255, 0, 0], [0, 255, 0], [0, 0, 255]], np.uint8)
        return np.ascontiguousarray(cols[k])
    raise ValueError(fill)
