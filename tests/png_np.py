"""Numpy restatement of the PNG encoder contract of csrc/png_enc.hip (include/poco_hip.h): the definition of every
byte, so the device must produce these BYTES.

    encode(rgb uint8 [H,W,3], lz=True) -> bytes          analyse(rgb, lz=True) -> (bytes, info)

Container: signature, IHDR (8 bit, colour type 2, no interlace), one IDAT per segment, IEND.  Rows are filtered with the filter
libpng's heuristic picks (smallest sum of |signed byte|, ties to the lowest type).  The filtered stream is cut into segments of
32 768 bytes; each is coded on its own as one deflate block (dynamic Huffman, or stored when that is shorter) followed by an
empty stored block, which puts the next segment on a byte boundary.  zlib header 78 01, Adler-32 behind.

The match finder (lz=True).  Position p of a segment of n bytes has up to three candidates q < p:
    p - 3                    (the pixel to the left)
    p - (1 + 3 W)            (the same byte one row up), when that is >= 0
    the largest q < p - p % 1024 with hash(q) == hash(p), hash(x) = (le32(s[x..x+4)) * 2654435761 mod 2^32) >> 19, defined for
                             x + 4 <= n: the table of positions is filled chunk by chunk of 1024, a chunk sees the chunks before it
The length of a candidate is the number of equal bytes from (q, p) on, at most min(258, n - p); the best is the longest, ties to
the smallest distance; below 3 there is no match.  The parse is greedy from the segment's start.

The Huffman codes.  Symbols with a non-zero count, sorted by (count, symbol), are merged with two queues (leaves, internal nodes
in the order made; on equal weight the leaf is taken first).  The depths give a count per length; lengths above 15 are counted at
15 and, while the Kraft sum over 2^-15 exceeds 2^15, one code moves from 15 to the longest shorter length in use, whose place
takes two (count[15] -= 1, count[l] -= 1, count[l + 1] += 2).  Lengths are then handed out by rank: the rarest symbols get the
longest.  Codes are canonical.  The end-of-block symbol counts once; a distance histogram with fewer than two non-zero counts
has the counts of symbols 0 and 1 raised to 1."""
from __future__ import annotations

import struct
import zlib

import numpy as np

SEGMENT = 32768
CHUNK = 1024
HASH_BITS = 13
MAX_MATCH = 258
SIGNATURE = b"\x89PNG\r\n\x1a\n"
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]


def worst_case_bytes(H: int, W: int) -> int:
    """signature 8 + IHDR 25 + IEND 12 + zlib header 2 + Adler 4 + the filtered stream + per segment (5 of a stored block or of
    a dynamic block's allowance, 5 of the empty stored block, 12 of its IDAT chunk)."""
    S = H * (1 + 3 * W)
    return 51 + S + 22 * (-(-S // SEGMENT))


# ---- row filters -----------------------------------------------------------------------------------------------------------------
def filter_rows(rgb: np.ndarray):
    """(filtered stream uint8 [H * (1 + 3W)], filter types [H], rows with a tie for the smallest sum)."""
    rgb = np.asarray(rgb)
    assert rgb.dtype == np.uint8 and rgb.ndim == 3 and rgb.shape[2] == 3 and rgb.shape[0] >= 1 and rgb.shape[1] >= 1
    H, W = rgb.shape[:2]
    cur = rgb.reshape(H, 3 * W).astype(np.int32)
    up = np.concatenate([np.zeros((1, 3 * W), np.int32), cur[:-1]], 0)
    left = np.concatenate([np.zeros((H, 3), np.int32), cur[:, :-3]], 1)
    ul = np.concatenate([np.zeros((H, 3), np.int32), up[:, :-3]], 1)
    p = left + up - ul
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    cand = np.stack([cur, cur - left, cur - up, cur - ((left + up) >> 1), cur - paeth], 0) & 255          # [5, H, 3W]
    sums = np.where(cand < 128, cand, 256 - cand).sum(2)                                                # [5, H]
    ftype = np.argmin(sums, 0)                                                                          # first of equal minima
    ties = np.flatnonzero((sums == sums.min(0, keepdims=True)).sum(0) > 1)
    out = np.empty((H, 1 + 3 * W), np.uint8)
    out[:, 0] = ftype
    out[:, 1:] = cand[ftype, np.arange(H)]
    return out.reshape(-1), ftype, ties


# ---- LZ77 ------------------------------------------------------------------------------------------------------------------------
def _fixed_distance_lengths(s: np.ndarray, d: int) -> np.ndarray:
    """Length of the match at distance d per position (0 where p < d), not yet limited to 258."""
    n = s.size
    out = np.zeros(n, np.int64)
    if d >= n:
        return out
    mis = np.full(n + 1, n, np.int64)                        # index of the next mismatch at or after p
    idx = np.arange(d, n)
    mis[d:n] = np.where(s[d:] != s[:-d], idx, n)
    nxt = np.minimum.accumulate(mis[::-1])[::-1]
    out[d:] = nxt[d:n] - idx
    return out


def hashes(s: np.ndarray) -> np.ndarray:
    """hash(x) for x + 4 <= n."""
    n = s.size
    if n < 4:
        return np.zeros(0, np.int64)
    v = s[:n - 3].astype(np.uint64) | (s[1:n - 2].astype(np.uint64) << 8) | (s[2:n - 1].astype(np.uint64) << 16) | (s[3:].astype(np.uint64) << 24)
    return (((v * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - HASH_BITS)).astype(np.int64)


def best_matches(s: np.ndarray, W: int):
    """(length [n], distance [n]) of the best candidate per position; length 0 = none."""
    n = s.size
    pos = np.arange(n)
    room = np.minimum(MAX_MATCH, n - pos)
    best_len = np.zeros(n, np.int64)
    best_dist = np.zeros(n, np.int64)
    h = hashes(s)
    q = np.full(n, -1, np.int64)
    table = np.full(1 << HASH_BITS, -1, np.int64)
    for lo in range(0, h.size, CHUNK):
        hi = min(lo + CHUNK, h.size)
        q[lo:hi] = table[h[lo:hi]]
        np.maximum.at(table, h[lo:hi], pos[lo:hi])
    hl = np.zeros(n, np.int64)
    act = np.flatnonzero(q >= 0)
    k = 0
    while act.size and k < MAX_MATCH:
        act = act[(act + k < n)]
        act = act[s[q[act] + k] == s[act + k]]
        hl[act] += 1
        k += 1
    cands = [(np.minimum(_fixed_distance_lengths(s, 3), room), np.full(n, 3, np.int64)),
             (np.minimum(_fixed_distance_lengths(s, 1 + 3 * W), room), np.full(n, 1 + 3 * W, np.int64)),
             (hl, pos - q)]
    for ln, dist in cands:
        ln = np.where(ln >= 3, ln, 0)
        take = (ln > best_len) | ((ln == best_len) & (ln > 0) & (dist < best_dist))
        best_len = np.where(take, ln, best_len)
        best_dist = np.where(take, dist, best_dist)
    return best_len, best_dist


def tokens(s: np.ndarray, W: int, lz: bool = True):
    """The greedy parse: a list of (position, length, distance), length 1 and distance 0 for a literal."""
    n = s.size
    if not lz:
        return [(p, 1, 0) for p in range(n)]
    bl, bd = best_matches(s, W)
    bl, bd = bl.tolist(), bd.tolist()
    out, p = [], 0
    while p < n:
        if bl[p] >= 3:
            out.append((p, bl[p], bd[p]))
            p += bl[p]
        else:
            out.append((p, 1, 0))
            p += 1
    return out


def length_symbol(ln: int):
    """(symbol, extra bits, extra value) of a match length 3..258."""
    x = ln - 3
    if x < 8:
        return 257 + x, 0, 0
    if ln == 258:
        return 285, 0, 0
    eb = x.bit_length() - 3
    return 261 + 4 * eb + ((x >> eb) & 3), eb, x & ((1 << eb) - 1)


def distance_symbol(d: int):
    x = d - 1
    if x < 4:
        return x, 0, 0
    eb = x.bit_length() - 2
    return 2 * (eb + 1) + ((x >> eb) & 1), eb, x & ((1 << eb) - 1)


# ---- Huffman ---------------------------------------------------------------------------------------------------------------------
def limit_counts(depth_counts, max_len: int = 15):
    """Count of codes per length [0 .. max_len] from the counts per tree depth: the stated repair of lengths above max_len."""
    cnt = [0] * (max_len + 1)
    for d, c in enumerate(depth_counts):
        cnt[min(d, max_len)] += c
    total = sum(c << (max_len - l) for l, c in enumerate(cnt) if l)
    while total > (1 << max_len):
        cnt[max_len] -= 1
        for l in range(max_len - 1, 0, -1):
            if cnt[l]:
                cnt[l] -= 1
                cnt[l + 1] += 2
                break
        total -= 1
    return cnt


def code_lengths(counts, max_len: int = 15):
    """Length per symbol (0 for a count of 0) of the length-limited Huffman code of `counts`."""
    counts = [int(c) for c in counts]
    order = sorted((c, s) for s, c in enumerate(counts) if c > 0)
    n = len(order)
    lens = [0] * len(counts)
    if n == 0:
        return lens
    if n == 1:
        lens[order[0][1]] = 1
        return lens
    w = [c for c, _ in order]
    iw, ipar, lpar = [0] * (n - 1), [0] * (n - 1), [0] * n
    i = j = 0
    for k in range(n - 1):
        tot = 0
        for _ in range(2):
            if i < n and (j >= k or w[i] <= iw[j]):
                tot += w[i]
                lpar[i] = k
                i += 1
            else:
                tot += iw[j]
                ipar[j] = k
                j += 1
        iw[k] = tot
    idep = [0] * (n - 1)
    for k in range(n - 3, -1, -1):
        idep[k] = idep[ipar[k]] + 1
    depth_counts = [0] * (n + 1)
    for i in range(n):
        depth_counts[idep[lpar[i]] + 1] += 1
    cnt = limit_counts(depth_counts, max_len)
    r = n                                                    # by rank: the most frequent symbols get the shortest lengths
    for l in range(1, max_len + 1):
        for _ in range(cnt[l]):
            r -= 1
            lens[order[r][1]] = l
    return lens


def canonical_codes(lens):
    """Code per symbol, bit-reversed for deflate's LSB-first packing."""
    max_len = max(max(lens), 1)
    cnt = [0] * (max_len + 2)
    for l in lens:
        cnt[l] += 1
    cnt[0] = 0
    nxt, code = [0] * (max_len + 2), 0
    for l in range(1, max_len + 1):
        code = (code + cnt[l - 1]) << 1
        nxt[l] = code
    out = []
    for l in lens:
        if l == 0:
            out.append(0)
            continue
        c = nxt[l]
        nxt[l] += 1
        out.append(int(format(c, "0%db" % l)[::-1], 2))
    return out


def _cl_code(v: int):
    """The fixed code-length code: 0..12 in 4 bits (codes 0..12), 13..18 in 5 bits (codes 26..31); bit-reversed."""
    c, l = (v, 4) if v <= 12 else (26 + v - 13, 5)
    return int(format(c, "0%db" % l)[::-1], 2), l


def _pack(vals, lens) -> np.ndarray:
    """LSB-first packing of (value, bit length) pairs into bytes (the last byte padded with zeros)."""
    vals = np.asarray(vals, np.uint64)
    lens = np.asarray(lens, np.int64)
    off = np.cumsum(lens) - lens
    total = int(lens.sum())
    bits = np.zeros(total, np.uint8)
    for b in range(int(lens.max()) if lens.size else 0):
        m = lens > b
        bits[off[m] + b] = ((vals[m] >> np.uint64(b)) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits, bitorder="little")


def code_segment(s: np.ndarray, W: int, last: bool, lz: bool = True):
    """(bytes of the segment's blocks, info): the dynamic or stored block, then the empty stored block."""
    n = s.size
    toks = tokens(s, W, lz)
    lcount, dcount = [0] * 286, [0] * 30
    lcount[256] = 1
    items = []                                               # (litlen symbol, extra bits, extra, dist symbol, extra bits, extra)
    for p, ln, d in toks:
        if d == 0:
            lcount[int(s[p])] += 1
            items.append((int(s[p]), 0, 0, -1, 0, 0))
        else:
            ls, leb, lev = length_symbol(ln)
            ds, deb, dev = distance_symbol(d)
            lcount[ls] += 1
            dcount[ds] += 1
            items.append((ls, leb, lev, ds, deb, dev))
    if sum(c > 0 for c in dcount) < 2:
        dcount[0], dcount[1] = max(dcount[0], 1), max(dcount[1], 1)
    llen, dlen = code_lengths(lcount), code_lengths(dcount)
    lcode, dcode = canonical_codes(llen), canonical_codes(dlen)
    vals, lens = [0 | 2 << 1, 286 - 257, 30 - 1, 19 - 4], [3, 5, 5, 4]       # BFINAL 0, BTYPE 2; HLIT, HDIST, HCLEN
    for v in CL_ORDER:
        vals.append(4 if v <= 12 else 5)
        lens.append(3)
    for l in llen + dlen:
        c, b = _cl_code(l)
        vals.append(c)
        lens.append(b)
    for ls, leb, lev, ds, deb, dev in items:
        v, b = lcode[ls], llen[ls]
        v |= lev << b
        b += leb
        if ds >= 0:
            v |= dcode[ds] << b
            b += dlen[ds]
            v |= dev << b
            b += deb
        vals.append(v)
        lens.append(b)
    vals.append(lcode[256])
    lens.append(llen[256])
    dyn_bits = sum(lens)
    stored = (dyn_bits + 7) // 8 > 5 + n
    if stored:
        body = b"\x00" + struct.pack("<HH", n & 0xFFFF, ~n & 0xFFFF) + s.tobytes()
        body += bytes([1 if last else 0]) + b"\x00\x00\xff\xff"
    else:
        vals.append(1 if last else 0)                        # the empty stored block: BFINAL, BTYPE 00, pad, LEN 0, NLEN FFFF
        lens.append(3)
        body = _pack(vals, lens).tobytes() + b"\x00\x00\xff\xff"
    info = {"tokens": toks, "stored": stored, "max_len": max(llen + dlen), "matches": sum(1 for t in toks if t[2]),
            "lit_lengths": llen, "dist_lengths": dlen}
    return body, info


# ---- the file ----------------------------------------------------------------------------------------------------------------------
def _chunk(kind: bytes, data: bytes) -> bytes:
    return struct.pack(">I", len(data)) + kind + data + struct.pack(">I", zlib.crc32(kind + data))


def analyse(rgb: np.ndarray, lz: bool = True):
    """(bytes of the .png file, info): info = {"filters": types per row, "ties": rows with a filter tie, "segments": [per segment
    {"tokens", "stored", "max_len", "matches", ...}], "filtered": the filtered stream}."""
    rgb = np.asarray(rgb)
    filt, ftype, ties = filter_rows(rgb)
    H, W = rgb.shape[:2]
    out = SIGNATURE + _chunk(b"IHDR", struct.pack(">IIBBBBB", W, H, 8, 2, 0, 0, 0))
    nseg = -(-filt.size // SEGMENT)
    segs = []
    for k in range(nseg):
        body, info = code_segment(filt[k * SEGMENT:(k + 1) * SEGMENT], W, k == nseg - 1, lz)
        if k == 0:
            body = b"\x78\x01" + body
        if k == nseg - 1:
            body += struct.pack(">I", zlib.adler32(filt.tobytes()))
        out += _chunk(b"IDAT", body)
        segs.append(info)
    out += _chunk(b"IEND", b"")
    return out, {"filters": ftype, "ties": ties, "segments": segs, "filtered": filt}


def encode(rgb: np.ndarray, lz: bool = True) -> bytes:
    return analyse(rgb, lz)[0]


# ---- the fixture set of tests/test_png_gpu.py (its coverage is asserted in tests/test_png_cpu.py) -----------------------------
SPECIAL_SHAPES = [(1, 1), (1, 5), (3, 7), (128, 85), (129, 85), (24, 700), (20, 1400), (2, 11000)]


def photo_like(H, W, seed=0):
    """Smooth gradients + hard edges + noise (the picture of tests/test_jpeg_cpu.py)."""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([128 + 100 * np.sin(x / 37.0) * np.cos(y / 23.0), 255.0 * x / W, 255.0 * y / H], -1)
    img[H // 4:H // 2, W // 3:2 * W // 3] = [250, 20, 30]
    img[(x + y) % 40 < 3] = [5, 5, 5]
    img += r.normal(0, 6, (H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def flat_picture(H=240, W=320):
    """One colour with one flat rectangle of another."""
    img = np.full((H, W, 3), (40, 90, 160), np.uint8)
    img[H // 4:H // 2, W // 5:3 * W // 5] = (220, 200, 30)
    return img


def special(H, W):
    """The picture at a special size: a vertical ramp with a repeating 7-pixel texture and a noisy band, so that rows differ
    from their neighbours (every filter has work) and matches exist beside literals."""
    r = np.random.default_rng(7 * H + W)
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([(x * 5 + y * 3) % 256, (x % 7) * 30 + y, (x // 3 + 2 * y) % 256], -1).astype(np.int64)
    band = (x % 50) < 8
    img[band] = r.integers(0, 256, (int(band.sum()), 3))
    return (img % 256).astype(np.uint8)


def fixture_set():
    """[(name, uint8 [H,W,3])]: the pictures the CPU test asserts coverage on and the GPU test compares bytes on."""
    from tests import jpeg_np
    out = []
    for H, W in ((96, 160), (120, 168)):
        for fill in jpeg_np.FIXTURE_FILLS:
            out.append((f"{fill}_{H}x{W}", jpeg_np.fixture(fill, H, W)))
    out.append(("photo_120x168", photo_like(120, 168)))
    out.append(("noise_64x200", np.random.default_rng(5).integers(0, 256, (64, 200, 3), dtype=np.uint8)))
    out.append(("flat_240x320", flat_picture()))
    for H, W in SPECIAL_SHAPES:
        out.append((f"special_{H}x{W}", special(H, W)))
    return out
