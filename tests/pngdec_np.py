"""The device PNG decoder's rules (csrc/png_dec.hip) restated in plain Python and numpy: a bit-exact inflate with the
decoder's status rules, the unfilter and the map to RGB.  Pinned on zlib and PIL in tests/test_pngdec_cpu.py; the reference for the
statuses of damaged streams and the proof that a fixture exercises what its name says (the stats)."""
import numpy as np

from poco_amd.png import PngInfo, parse_png

ERR_CODE, ERR_SHORT, ERR_SIZE, ERR_FILTER = 1, 2, 3, 4
_CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_LEN = [(3 + i, 0) for i in range(8)] + [(3 + ((4 + (i & 3)) << ((i >> 2) - 1)), (i >> 2) - 1) for i in range(8, 28)] + [(258, 0)]
_DIST = [(i + 1, 0) for i in range(4)] + [(1 + ((2 + (i & 1)) << ((i >> 1) - 1)), (i >> 1) - 1) for i in range(4, 30)]


class _Bad(Exception):
    def __init__(self, status):
        self.status = status


def _table(lens, allow_empty):
    """{(length, code): symbol} of the canonical code, or _Bad: over-subscribed, or incomplete other than a single code of one bit
    (allow_empty: no code at all is accepted too - the distance code of a block without matches)."""
    count = [0] * 16
    for l in lens:
        count[l] += 1
    count[0] = 0
    total = sum(count)
    kraft = sum(c << (15 - l) for l, c in enumerate(count) if l)
    if not (kraft == 32768 or (total == 1 and count[1] == 1) or (allow_empty and total == 0)):
        raise _Bad(ERR_CODE)
    code, nxt = 0, [0] * 16
    for l in range(1, 16):
        code = (code + count[l - 1]) << 1
        nxt[l] = code
    out = {}
    for sym, l in enumerate(lens):
        if l:
            out[(l, nxt[l])] = sym
            nxt[l] += 1
    return out


_FIXED = None


def inflate(stream: bytes, expect: int = None):
    """-> (bytes | None, status, stats).  status 0 only for a stream zlib's inflate accepts (and, with `expect`, one that yields
    exactly that many bytes).  stats: max_dist, max_len, block_types (set), blocks, matches, dist1_longer (a match with distance 1
    and length > 1)."""
    global _FIXED
    stats = {"max_dist": 0, "max_len": 0, "block_types": set(), "blocks": 0, "matches": 0, "overlap": False}
    out = bytearray()
    acc, nacc, nxt = 0, 0, 0           # bit accumulator, its bits, the next byte of the stream

    def bits(n):
        nonlocal acc, nacc, nxt
        while nacc < n:
            if nxt >= len(stream):
                raise _Bad(ERR_SHORT)
            acc |= stream[nxt] << nacc
            nacc += 8
            nxt += 1
        v = acc & ((1 << n) - 1)
        acc >>= n
        nacc -= n
        return v

    def symbol(tab):
        code = 0
        for l in range(1, 16):
            code = (code << 1) | bits(1)
            if (l, code) in tab:
                return tab[(l, code)]
        raise _Bad(ERR_CODE)

    try:
        while True:
            final, btype = bits(1), bits(2)
            stats["blocks"] += 1
            stats["block_types"].add(btype)
            if btype == 3:
                raise _Bad(ERR_CODE)
            if btype == 0:
                bits(nacc & 7)
                ln, nln = bits(16), bits(16)
                if ln ^ 0xFFFF != nln:
                    raise _Bad(ERR_CODE)
                nxt -= nacc >> 3           # whole bytes go back to the stream
                acc = nacc = 0
                if nxt + ln > len(stream):
                    raise _Bad(ERR_SHORT)
                out += stream[nxt:nxt + ln]
                nxt += ln
            else:
                if btype == 1:
                    if _FIXED is None:
                        _FIXED = (_table([8] * 144 + [9] * 112 + [7] * 24 + [8] * 8, False), _table([5] * 32, False))
                    lit, dist = _FIXED
                else:
                    hlit, hdist, hclen = bits(5) + 257, bits(5) + 1, bits(4) + 4
                    if hlit > 286 or hdist > 30:
                        raise _Bad(ERR_CODE)
                    cl = [0] * 19
                    for i in range(hclen):
                        cl[_CL_ORDER[i]] = bits(3)
                    if sum(128 >> l for l in cl if l) != 128:          # the code-length code must be complete
                        raise _Bad(ERR_CODE)
                    clt = _table(cl, False)
                    lens = []
                    while len(lens) < hlit + hdist:
                        s = symbol(clt)
                        if s < 16:
                            lens.append(s)
                            continue
                        if s == 16:
                            if not lens:
                                raise _Bad(ERR_CODE)
                            rep, v = 3 + bits(2), lens[-1]
                        elif s == 17:
                            rep, v = 3 + bits(3), 0
                        else:
                            rep, v = 11 + bits(7), 0
                        if len(lens) + rep > hlit + hdist:
                            raise _Bad(ERR_CODE)
                        lens += [v] * rep
                    if lens[256] == 0:
                        raise _Bad(ERR_CODE)
                    lit, dist = _table(lens[:hlit], False), _table(lens[hlit:], True)
                while True:
                    s = symbol(lit)
                    if s < 256:
                        out.append(s)
                    elif s == 256:
                        break
                    else:
                        if s >= 286:
                            raise _Bad(ERR_CODE)
                        base, eb = _LEN[s - 257]
                        ln = base + bits(eb)
                        d = symbol(dist)
                        if d >= 30:
                            raise _Bad(ERR_CODE)
                        base, eb = _DIST[d]
                        d = base + bits(eb)
                        if d > len(out):
                            raise _Bad(ERR_CODE)
                        stats["matches"] += 1
                        stats["max_dist"] = max(stats["max_dist"], d)
                        stats["max_len"] = max(stats["max_len"], ln)
                        stats["overlap"] |= d == 1 and ln > d
                        start = len(out) - d
                        for k in range(ln):
                            out.append(out[start + k % d] if d < ln else out[start + k])
                    if expect is not None and len(out) > expect:
                        raise _Bad(ERR_SIZE)
            if expect is not None and len(out) > expect:
                raise _Bad(ERR_SIZE)
            if final:
                break
        if expect is not None and len(out) != expect:
            raise _Bad(ERR_SIZE)
    except _Bad as e:
        return None, e.status, stats
    return bytes(out), 0, stats


def unfilter(raw: bytes, H: int, W: int, bpp: int):
    """The filtered stream -> uint8 [H, W * bpp], or None for a filter byte above 4."""
    stride = W * bpp
    a = np.frombuffer(raw, np.uint8).reshape(H, 1 + stride)
    out = np.zeros((H, stride), np.uint8)
    up = np.zeros(stride, np.int64)
    for y in range(H):
        ft, line = int(a[y, 0]), a[y, 1:].astype(np.int64)
        if ft > 4:
            return None
        if ft == 0:
            cur = line
        elif ft == 2:
            cur = (line + up) & 255
        elif ft == 1:
            cur = (np.cumsum(line.reshape(W, bpp), 0) & 255).reshape(stride)
        else:
            cur = np.zeros(stride, np.int64)
            for x in range(stride):
                left = cur[x - bpp] if x >= bpp else 0
                ul = up[x - bpp] if x >= bpp else 0
                if ft == 1:
                    p = left
                elif ft == 3:
                    p = (left + up[x]) >> 1
                else:
                    pa, pb, pc = abs(up[x] - ul), abs(left - ul), abs(left + up[x] - 2 * ul)
                    p = left if pa <= pb and pa <= pc else (up[x] if pb <= pc else ul)
                cur[x] = (line[x] + p) & 255
        out[y] = cur
        up = cur
    return out


def to_rgb(px: np.ndarray, info: PngInfo) -> np.ndarray:
    H, W, ct = info.height, info.width, info.colour_type
    p = px.reshape(H, W, info.bpp)
    if ct in (2, 6):
        return np.ascontiguousarray(p[:, :, :3])
    if ct in (0, 4):
        return np.repeat(p[:, :, :1], 3, 2)
    pal = np.frombuffer(info.palette, np.uint8).reshape(256, 3)
    return pal[p[:, :, 0]]


def stream_of(info: PngInfo) -> bytes:
    z = b"".join(info.data[o:o + l] for o, l in info.idat)
    return z[2:len(z) - 4]


def decode(data):
    """-> (uint8 [H,W,3] | None, status, stats) of the bytes of a .png file (or a PngInfo) that parse_png accepts."""
    info = data if isinstance(data, PngInfo) else parse_png(data)
    assert info is not None
    expect = info.height * (1 + info.bpp * info.width)
    raw, st, stats = inflate(stream_of(info), expect)
    if st:
        return None, st, stats
    px = unfilter(raw, info.height, info.width, info.bpp)
    if px is None:
        return None, ERR_FILTER, stats
    return to_rgb(px, info), 0, stats
