"""Numpy restatement of the baseline JPEG decoder contract of csrc/jpeg_dec.hip (include/poco_hip.h): a sequential
decoder in integer arithmetic whose pixels are libjpeg's with jpeg_decompress defaults - what PIL gives - so the device must
produce these BYTES.

    decode(data) -> uint8 [H,W,3]         raises JpegError on a damaged stream
    decode_stats(data) -> (pixels, stats) stats: what the fixture sets are asserted to contain (new_stats lists the counters)
    sync_rounds(data) -> int              a model of the device's self-synchronising subsequences: the rounds a stream needs

The marker walk is poco_amd.jpeg.parse_jpeg (host code, tested here against PIL through the pixels).  Entropy decoding follows
T.81 F.2.2 with the device's bit reader: a position is (byte, bit) in the STUFFED stream, an 0xFF data byte is followed by a
skipped 0x00, bytes past the restart interval read as zero.  Dequantisation and the "islow" inverse DCT are jidctint.c's, chroma
upsampling is jdsample.c's "fancy" triangle filter over the component's own width and height, colour is jdcolor.c's."""
from __future__ import annotations

import numpy as np

from poco_amd.jpeg import SUBSEQ_BYTES, parse_jpeg

LOOKAHEAD = 9                          # bits of the device's lookahead table (JD_LOOKAHEAD)


class JpegError(ValueError):
    pass


def fix(x: float, bits: int) -> int:
    return int(x * (1 << bits) + 0.5)


class HuffTable:
    """T.81 F.2.2.3 / jdhuff.c: a lookahead table for codes of up to LOOKAHEAD bits, maxcode / valptr for longer ones."""

    def __init__(self, bits, vals):
        self.vals = list(vals)
        self.look = [0] * (1 << LOOKAHEAD)                 # length << 8 | symbol, 0 = no code this short
        self.maxcode = [-1] * 18                           # maxcode[l]: largest code of length l (-1 = none)
        self.delta = [0] * 17                              # valptr[l] - mincode[l]
        code, k = 0, 0
        for ln in range(1, 17):
            self.delta[ln] = k - code
            for _ in range(bits[ln - 1]):
                if ln <= LOOKAHEAD:
                    lo = code << (LOOKAHEAD - ln)
                    for j in range(lo, lo + (1 << (LOOKAHEAD - ln))):
                        self.look[j] = (ln << 8) | self.vals[k]
                code += 1
                k += 1
            self.maxcode[ln] = code - 1 if bits[ln - 1] else -1
            code <<= 1
        self.maxcode[17] = 1 << 20

    def lookup(self, w16: int):
        """(length, symbol) of the code at the top of the 16-bit window, or (0, 0)."""
        e = self.look[w16 >> (16 - LOOKAHEAD)]
        if e:
            return e >> 8, e & 255
        for ln in range(LOOKAHEAD + 1, 17):
            c = w16 >> (16 - ln)
            if c <= self.maxcode[ln]:
                i = c + self.delta[ln]
                return (ln, self.vals[i]) if 0 <= i < len(self.vals) else (0, 0)
        return 0, 0


def _window(d, end, bp, bo):
    """32 bits from position (bp, bo), the byte index after each of the 5 data bytes read, and the index of each of them."""
    w, q, steps, pos = 0, bp, [], []
    for _ in range(5):
        b = d[q] if q < end else 0
        w = (w << 8) | b
        pos.append(q)
        q += 2 if b == 0xFF else 1
        steps.append(q)
    return ((w << bo) >> 8) & 0xFFFFFFFF, steps, pos


def decode_span(d, end, state, stop, tabs, comp_of, strict, sink=None, blk=0, max_blk=1 << 30, stats=None, lo=0, later=False):
    """Decode symbols from `state` = (bp, bo, block within the MCU, zigzag index) while bp < stop (symbols that START before
    `stop`) and blk < max_blk.  Returns (exit state, blocks finished).  sink(blk, zigzag index, value) receives coefficients
    (DC as differences).  strict: a damaged stream raises; otherwise it is decoded by the device's fixed rule (a window that
    holds no code counts as a 16-bit code of symbol 0, a zigzag index past 63 ends the block).  stats: the counters of
    decode_stats; `lo` is then the start of the restart interval, from which subsequence boundaries are counted, and `later`
    says that it is not the file's first one."""
    bp, bo, b, z = state
    nblk = 0
    bpm = len(comp_of)
    zrls = 0                                                   # ZRLs in a row just before this symbol
    while bp < stop and blk < max_blk:
        w, steps, pos = _window(d, end, bp, bo)
        dc, ac = tabs[comp_of[b]]
        ln, sym = (dc if z == 0 else ac).lookup(w >> 16)
        if ln == 0:
            if strict:
                raise JpegError("no Huffman code at byte %d" % bp)
            ln, sym = 16, 0
        elif stats is not None:
            stats["long_codes"] += ln > LOOKAHEAD
            stats["max_code_len"] = max(stats["max_code_len"], ln)
            stats["dc_code_lens" if z == 0 else "ac_code_lens"].add(ln)
            stats["sym_fa"] += z != 0 and sym == 0xFA
        s = sym & 15
        r = sym >> 4 if z else 0
        val = None
        if z == 0:
            s = sym
            if s > 15:
                raise JpegError("DC category")
            val, k = 0, 0
            z = 1
        elif s == 0:
            if r == 15:
                z += 16
                if stats is not None:
                    stats["zrl"] += 1
            else:
                z = 64
                if stats is not None:
                    stats["eob"] += 1
        else:
            z += r
            if z > 63:
                if strict:
                    raise JpegError("zigzag index past 63 at byte %d" % bp)
                s = 0                                          # (the device consumes the code only and ends the block)
            else:
                k = z
                val = 0
                z += 1
        if s:
            v = (w >> (32 - ln - s)) & ((1 << s) - 1) if ln + s <= 32 else 0
            val = v if v >= (1 << (s - 1)) else v - (1 << s) + 1
            if stats is not None:
                stats["max_category"] = max(stats["max_category"], s)
        if val is not None and sink is not None and (val or k == 0):
            sink(blk, k, val)
        n = bo + ln + s
        if stats is not None:
            if val is not None and k == 0:
                stats["max_dc_category"] = max(stats["max_dc_category"], s)
                if s == 11:
                    stats["dc11_signs"].add(1 if val > 0 else -1)
            if val is not None and k == 63:
                stats["full_blocks"] += 1
                stats["zrl3_then_63"] += zrls == 3
            zrls = zrls + 1 if (z > 1 and val is None and sym == 0xF0) else 0
            # the symbol's first bit lies in byte bp, its last one in byte pos[(n - 1) >> 3]
            if ln + s >= 20 and (bp - lo) // SUBSEQ_BYTES != (pos[(n - 1) >> 3] - lo) // SUBSEQ_BYTES:
                _count(stats, "long_symbol_straddles", later)
        if n >= 8:
            bp = steps[(n >> 3) - 1]
        bo = n & 7
        if z >= 64:
            if stats is not None and bo == 0 and bp > lo and bp < end and (bp - lo) % SUBSEQ_BYTES == 0:
                _count(stats, "aligned_block_ends", later)
            z = 0
            b = (b + 1) % bpm
            blk += 1
            nblk += 1
    return (bp, bo, b, z), nblk


def _count(stats, key, later):
    stats[key] += 1
    if later:
        stats["later_intervals"][key] += 1


def boundary_ff(info, stats):
    """Stuffed FF 00 pairs at the subsequence boundaries of every restart interval: across one, and just before one."""
    d = info.data
    for si, (off, ln, _) in enumerate(info.segments.tolist()):
        lo = info.scan_offset + off
        for bnd in range(lo + SUBSEQ_BYTES, lo + ln, SUBSEQ_BYTES):
            if d[bnd - 1] == 0xFF and d[bnd] == 0:
                _count(stats, "ff_straddles", si > 0)
            if d[bnd - 2] == 0xFF and d[bnd - 1] == 0:
                _count(stats, "ff_before_boundary", si > 0)


BOUNDARY_COUNTERS = ("ff_straddles", "ff_before_boundary", "long_symbol_straddles", "aligned_block_ends")


def new_stats() -> dict:
    """The counters of decode_stats.  A subsequence boundary is a multiple of SUBSEQ_BYTES from its restart interval's start
    that lies inside the interval, as jdec_sync computes it.
    ff_straddles           an 0xFF is the last byte before a boundary, its stuffed 0x00 the first one after it
    ff_before_boundary     the stuffed 0x00 is the last byte before a boundary
    long_symbol_straddles  a symbol of 20 bits or more (code + value bits) starts before a boundary and ends after it
    aligned_block_ends     a block ends with bit offset 0 exactly on a boundary
    later_intervals        the four above again, counted in restart intervals other than the file's first
    full_blocks            blocks whose last symbol writes coefficient 63: no EOB
    zrl3_then_63           blocks in which three ZRLs are followed by a non-zero coefficient 63
    sym_fa                 AC symbols 0xFA (run 15, size 10)
    max_code_len, dc_code_lens, ac_code_lens   the code lengths the stream uses
    max_dc_category, dc11_signs                DC differences (the signs of those of category 11)"""
    st = {k: 0 for k in ("zrl", "eob", "long_codes", "max_category", "max_code_len", "max_dc_category", "sym_fa", "full_blocks",
                         "zrl3_then_63") + BOUNDARY_COUNTERS}
    st.update(dc_code_lens=set(), ac_code_lens=set(), dc11_signs=set(), later_intervals={k: 0 for k in BOUNDARY_COUNTERS})
    return st


def _geometry(info):
    """components' (h, v), blocks per MCU and the component of each block of an MCU"""
    samp = [(info.hsamp, info.vsamp)] + [(1, 1)] * (info.ncomp - 1)
    comp_of = [c for c, (h, v) in enumerate(samp) for _ in range(h * v)]
    return samp, comp_of


def coefficients(info, stats=None):
    """int32 [MCUs * blocks per MCU, 64]: quantised coefficients in natural order, DC prediction undone, in scan order."""
    samp, comp_of = _geometry(info)
    bpm = len(comp_of)
    mcuy, mcux = info.mcus
    nmcu = mcuy * mcux
    tabs = [(HuffTable(*info.dc[c]), HuffTable(*info.ac[c])) for c in range(info.ncomp)]
    coef = np.zeros((nmcu * bpm, 64), np.int32)
    from poco_amd.jpeg import _ZIGZAG
    zz = _ZIGZAG.tolist()

    def sink(blk, k, val):
        coef[blk, zz[k]] = val

    d = info.data
    segs = info.segments.tolist()
    for si, (off, ln, mcu0) in enumerate(segs):
        n_mcu = (segs[si + 1][2] if si + 1 < len(segs) else nmcu) - mcu0
        if n_mcu <= 0 or mcu0 + n_mcu > nmcu:
            raise JpegError("restart intervals do not match the picture")
        lo, hi = info.scan_offset + off, info.scan_offset + off + ln
        b0, b1 = mcu0 * bpm, (mcu0 + n_mcu) * bpm
        _, got = decode_span(d, hi, (lo, 0, 0, 0), hi, tabs, comp_of, True, sink, b0, b1, stats, lo, si > 0)
        if got != b1 - b0:
            raise JpegError("restart interval %d ends after %d of %d blocks" % (si, got, b1 - b0))
        # DC differences -> values, per component, from 0 at the start of the interval
        blocks = coef[b0:b1].reshape(n_mcu, bpm, 64)
        for c in range(info.ncomp):
            ks = [k for k in range(bpm) if comp_of[k] == c]
            dcv = np.cumsum(blocks[:, ks, 0].reshape(-1)).reshape(n_mcu, len(ks))
            blocks[:, ks, 0] = dcv.astype(np.int16)            # (int16 storage, as on the device)
    return coef


_C = {k: fix(v, 13) for k, v in dict(c0_298=0.298631336, c0_390=0.390180644, c0_541=0.541196100, c0_765=0.765366865,
                                     c0_899=0.899976223, c1_175=1.175875602, c1_501=1.501321110, c1_847=1.847759065,
                                     c1_961=1.961570560, c2_053=2.053119869, c2_562=2.562915447, c3_072=3.072711026).items()}


def _idct_1d(d, n):
    """One pass of jidctint.c jpeg_idct_islow over the last axis of d [..., 8], descaled by n bits."""
    d = [d[..., i] for i in range(8)]
    z1 = (d[2] + d[6]) * _C["c0_541"]
    t2 = z1 - d[6] * _C["c1_847"]
    t3 = z1 + d[2] * _C["c0_765"]
    t0, t1 = (d[0] + d[4]) << 13, (d[0] - d[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    t0, t1, t2, t3 = d[7], d[5], d[3], d[1]
    z1, z2, z3, z4 = t0 + t3, t1 + t2, t0 + t2, t1 + t3
    z5 = (z3 + z4) * _C["c1_175"]
    t0, t1, t2, t3 = t0 * _C["c0_298"], t1 * _C["c2_053"], t2 * _C["c3_072"], t3 * _C["c1_501"]
    z1, z2 = -z1 * _C["c0_899"], -z2 * _C["c2_562"]
    z3, z4 = -z3 * _C["c1_961"] + z5, -z4 * _C["c0_390"] + z5
    t0, t1, t2, t3 = t0 + z1 + z3, t1 + z2 + z4, t2 + z2 + z3, t3 + z1 + z4
    out = [t10 + t3, t11 + t2, t12 + t1, t13 + t0, t13 - t0, t12 - t1, t11 - t2, t10 - t3]
    r = 1 << (n - 1)
    return np.stack([(o + r) >> n for o in out], -1)


def idct_islow(blocks: np.ndarray) -> np.ndarray:
    """blocks int [N,8,8] dequantised coefficients -> samples 0..255 (columns first: 13 - 2 bits, then rows: 13 + 2 + 3)."""
    ws = np.swapaxes(_idct_1d(np.swapaxes(blocks.astype(np.int64), 1, 2), 11), 1, 2)
    return np.clip(_idct_1d(ws, 18) + 128, 0, 255)


def planes(info, coef):
    """The components' sample planes, whole blocks wide and high."""
    samp, comp_of = _geometry(info)
    bpm = len(comp_of)
    mcuy, mcux = info.mcus
    blocks = coef.reshape(mcuy, mcux, bpm, 8, 8)
    out, k0 = [], 0
    for c, (h, v) in enumerate(samp):
        q = info.qt[c].astype(np.int64).reshape(8, 8)
        # ISLOW_MULT_TYPE is a 16-bit type: the product is formed in int, from int16 coefficients
        px = idct_islow((blocks[:, :, k0:k0 + h * v].reshape(-1, 8, 8).astype(np.int16).astype(np.int64) * q))
        px = px.reshape(mcuy, mcux, v, h, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(mcuy * v * 8, mcux * h * 8)
        out.append(px)
        k0 += h * v
    return out


def upsample_h2v1(c: np.ndarray) -> np.ndarray:
    """jdsample.c h2v1_fancy_upsample over a plane of the component's own width: 3/4 1/4, roundings + 1 (even) / + 2 (odd
    columns), the first and the last column copied."""
    c = c.astype(np.int64)
    left = np.concatenate([c[:, :1], c[:, :-1]], 1)
    right = np.concatenate([c[:, 1:], c[:, -1:]], 1)
    out = np.empty((c.shape[0], 2 * c.shape[1]), np.int64)
    out[:, 0::2] = (3 * c + left + 1) >> 2
    out[:, 1::2] = (3 * c + right + 2) >> 2
    out[:, 0], out[:, -1] = c[:, 0], c[:, -1]
    return out


def upsample_h2v2(c: np.ndarray) -> np.ndarray:
    """jdsample.c h2v2_fancy_upsample: vertically 3/4 of the nearer and 1/4 of the farther row (the first / last row repeated
    at the picture's edge), horizontally the same on the column sums, roundings + 8 (even) / + 7 (odd columns), >> 4."""
    c = c.astype(np.int64)
    up = np.concatenate([c[:1], c[:-1]], 0)
    down = np.concatenate([c[1:], c[-1:]], 0)
    out = np.empty((2 * c.shape[0], 2 * c.shape[1]), np.int64)
    for par, far in ((0, up), (1, down)):
        s = 3 * c + far
        left = np.concatenate([s[:, :1], s[:, :-1]], 1)
        right = np.concatenate([s[:, 1:], s[:, -1:]], 1)
        out[par::2, 0::2] = (3 * s + left + 8) >> 4
        out[par::2, 1::2] = (3 * s + right + 7) >> 4
        out[par::2, 0] = (4 * s[:, 0] + 8) >> 4
        out[par::2, -1] = (4 * s[:, -1] + 7) >> 4
    return out


def ycc_to_rgb(y, cb, cr) -> np.ndarray:
    """jdcolor.c ycc_rgb_convert: SCALEBITS 16."""
    y, cb, cr = y.astype(np.int64), cb.astype(np.int64) - 128, cr.astype(np.int64) - 128
    half = 1 << 15
    r = y + ((fix(1.40200, 16) * cr + half) >> 16)
    g = y + ((-fix(0.34414, 16) * cb + half - fix(0.71414, 16) * cr) >> 16)
    b = y + ((fix(1.77200, 16) * cb + half) >> 16)
    return np.clip(np.stack([r, g, b], -1), 0, 255).astype(np.uint8)


def decode_stats(data: bytes):
    info = parse_jpeg(data)
    if info is None:
        raise JpegError("not a baseline JPEG this decoder takes")
    stats = new_stats()
    stats.update(stuffed=data[info.scan_offset:info.scan_offset + info.scan_length].count(b"\xff\x00"),
                 segments=len(info.segments), max_segment_bytes=int(info.segments[:, 1].max()))
    boundary_ff(info, stats)
    pl = planes(info, coefficients(info, stats))
    H, W = info.height, info.width
    if info.ncomp == 1:
        y = pl[0][:H, :W]
        return np.stack([y, y, y], -1).astype(np.uint8), stats
    cw, ch = -(-W // info.hsamp), -(-H // info.vsamp)
    chroma = []
    for p in pl[1:]:
        p = p[:ch, :cw]
        if info.hsamp == 2 and cw > 2:                        # jdsample.c: the fancy filters need more than 2 columns
            p = upsample_h2v2(p) if info.vsamp == 2 else upsample_h2v1(p)
        else:
            p = np.repeat(np.repeat(p, info.vsamp, 0), info.hsamp, 1)
        chroma.append(p[:H, :W])
    return ycc_to_rgb(pl[0][:H, :W], chroma[0], chroma[1]), stats


def decode(data: bytes) -> np.ndarray:
    return decode_stats(data)[0]


def sync_rounds(data: bytes, subseq: int = SUBSEQ_BYTES) -> int:
    """The device's scheme on the host: every restart interval is cut into subsequences of `subseq` bytes; in round 1 every
    lane decodes from the guessed state (its first byte - one later when that is a stuffed 0x00 -, block 0, zigzag index 0), in
    later rounds from its predecessor's exit state; the loop ends after the first round in which no exit state changed.
    Returns the number of rounds in which one did (1 = every guess was right or there was nothing to guess)."""
    info = parse_jpeg(data)
    samp, comp_of = _geometry(info)
    tabs = [(HuffTable(*info.dc[c]), HuffTable(*info.ac[c])) for c in range(info.ncomp)]
    d = info.data
    worst = 1
    for off, ln, _ in info.segments.tolist():
        lo, hi = info.scan_offset + off, info.scan_offset + off + ln
        nsub = max(1, -(-ln // subseq))
        start = [lo + j * subseq for j in range(nsub)]
        stop = [min(lo + (j + 1) * subseq, hi) for j in range(nsub)]
        entry = [(s + (1 if j and d[s - 1] == 0xFF and d[s] == 0 else 0), 0, 0, 0) for j, s in enumerate(start)]
        memo = {}                                              # (lane, entry state) -> exit state: chains meet again and again

        def span(j):
            key = (j, entry[j])
            if key not in memo:
                memo[key] = decode_span(d, hi, entry[j], stop[j], tabs, comp_of, False)[0]
            return memo[key]

        exits = [span(j) for j in range(nsub)]
        rounds = 1
        for _ in range(nsub):
            changed = False
            new = list(exits)
            for j in range(1, nsub):
                if entry[j] != exits[j - 1]:
                    entry[j] = exits[j - 1]
                    new[j] = span(j)
                    changed |= new[j] != exits[j]
            exits = new
            if not changed:
                break
            rounds += 1
        worst = max(worst, rounds)
    return worst
