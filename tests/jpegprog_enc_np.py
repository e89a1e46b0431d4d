"""A scan-script transcoder for the progressive decoder's tests: the quantised coefficients of a JPEG file PIL wrote, sent again
as a progressive file with ANY scan script, Huffman table shape and table id layout - what PIL (libjpeg's one default script)
never writes.  Plain Python; the four encoders follow ITU-T T.81 G.1.2 (the procedures libjpeg's jcphuff.c implements), the tables
Annex K.2.

    rescan(data, script, tables="optimal", table_ids="per_kind", max_eobrun=0x7FFF) -> bytes

script: [(components, Ss, Se, Ah, Al)], components a tuple of indices into the frame's.  The frame header and DQT are the source
file's (SOF re-marked SOF2); the coefficients are read with the restatements (tests/jpegprog_np.py or tests/jpegdec_np.py).  The
transcoder is pinned on libjpeg alone: PIL's pixels of a rescanned file whose script sends every bit equal PIL's pixels of the
source (tests/test_jpegprog_cpu.py).

tables:    "optimal"  per scan, from the scan's own symbol counts by Annex K.2 (lengths limited to 16, no all-ones code word)
           "flat"     one fixed table per class for every scan: even symbols 8 bits, odd symbols 9 bits
           "deep"     per scan, a prefix code of 10 .. 16 bits whose longest words go to the symbols the scan uses most
table_ids: "per_kind" DC tables in id c of component c, AC tables of first scans in id c, of refinement scans in id 3
           "one"      a fresh DHT with id 0 before every scan"""
from __future__ import annotations

from poco_amd.jpeg import _ZIGZAG, parse_jpeg, parse_progressive_jpeg
from tests import jpegdec_np as J
from tests import jpegprog_np as P

ZZ = _ZIGZAG.tolist()


# ---- Huffman tables ---------------------------------------------------------------------------------------------------------------
def optimal_table(freq: dict):
    """(bits[16], huffval) by T.81 K.2: code sizes with a reserved 257th symbol of frequency 1 (figure K.1), the counts per size
    (K.2), sizes above 16 folded back (K.3), the reserved word taken off the longest size, symbols sorted by size (K.4)."""
    f = [0] * 257
    for s, n in freq.items():
        f[s] = n
    f[256] = 1
    size = [0] * 257
    others = [-1] * 257
    while True:
        v1 = v2 = -1
        for i in range(257):                               # least frequency, the larger value on a tie
            if f[i] and (v1 < 0 or f[i] <= f[v1]):
                v1 = i
        for i in range(257):
            if f[i] and i != v1 and (v2 < 0 or f[i] <= f[v2]):
                v2 = i
        if v2 < 0:
            break
        f[v1] += f[v2]
        f[v2] = 0
        size[v1] += 1
        while others[v1] >= 0:
            v1 = others[v1]
            size[v1] += 1
        others[v1] = v2
        size[v2] += 1
        while others[v2] >= 0:
            v2 = others[v2]
            size[v2] += 1
    bits = [0] * 33
    for i in range(257):
        if size[i]:
            bits[size[i]] += 1
    i = 32
    while i > 16:
        while bits[i] > 0:
            j = i - 2
            while bits[j] == 0:
                j -= 1
            bits[i] -= 2
            bits[i - 1] += 1
            bits[j + 1] += 2
            bits[j] -= 1
        i -= 1
    while bits[i] == 0:
        i -= 1
    bits[i] -= 1
    vals = [s for ln in range(1, 33) for s in range(256) if size[s] == ln]
    return bits[1:17], vals


def flat_table(dc: bool):
    """Every symbol a class can have (DC categories 0 .. 11, all 256 run/size bytes), the even ones 8 bits, the odd ones 9."""
    syms = list(range(12 if dc else 256))
    even, odd = syms[0::2], syms[1::2]
    bits = [0] * 16
    bits[7], bits[8] = len(even), len(odd)
    return bits, even + odd


def deep_table(freq: dict):
    """No word shorter than 10 bits: the most used symbol 16 bits, the next 15 ... the seventh and every other one 10."""
    order = sorted(freq, key=lambda s: (-freq[s], s))
    length = {s: max(16 - i, 10) for i, s in enumerate(order)}
    bits = [0] * 16
    for ln in length.values():
        bits[ln - 1] += 1
    return bits, sorted(length, key=lambda s: (length[s], s))


def code_words(bits, vals) -> dict:
    """symbol -> (code, length), T.81 C.2."""
    out, code, k = {}, 0, 0
    for ln in range(1, 17):
        for _ in range(bits[ln - 1]):
            out[vals[k]] = (code, ln)
            code += 1
            k += 1
        code <<= 1
    return out


# ---- the four encoders: tokens ("S", table slot, symbol) and ("B", value, bits) ---------------------------------------------------
def _nbits(v: int) -> int:
    return int(v).bit_length()


def enc_dc_first(cz, blocks, ncomp_scan, al):
    out, pred = [], [0] * ncomp_scan
    for k, blk in blocks:
        v = int(cz[blk][0]) >> al                          # arithmetic shift: the point transform of DC
        d = v - pred[k]
        pred[k] = v
        n = _nbits(abs(d))
        out.append(("S", k, n))
        if n:
            out.append(("B", (d if d >= 0 else d - 1) & ((1 << n) - 1), n))
    return out


def enc_dc_refine(cz, blocks, al):
    return [("B", (int(cz[blk][0]) >> al) & 1, 1) for _, blk in blocks]


def _eobrun_tokens(run: int):
    n = _nbits(run) - 1
    return [("S", 0, n << 4)] + ([("B", run & ((1 << n) - 1), n)] if n else [])


def enc_ac_first(cz, blocks, ss, se, al, max_eobrun):
    out, eobrun = [], 0
    for _, blk in blocks:
        row = cz[blk]
        r = 0
        for k in range(ss, se + 1):
            t = int(row[k])
            a = abs(t) >> al                               # AC: the magnitude is divided, towards zero
            if a == 0:
                r += 1
                continue
            if eobrun:
                out += _eobrun_tokens(eobrun)
                eobrun = 0
            while r > 15:
                out.append(("S", 0, 0xF0))
                r -= 16
            n = _nbits(a)
            out.append(("S", 0, (r << 4) | n))
            out.append(("B", a if t > 0 else a ^ ((1 << n) - 1), n))
            r = 0
        if r > 0:
            eobrun += 1
            if eobrun == max_eobrun:
                out += _eobrun_tokens(eobrun)
                eobrun = 0
    if eobrun:
        out += _eobrun_tokens(eobrun)
    return out


def enc_ac_refine(cz, blocks, ss, se, al, max_eobrun):
    out, eobrun, be = [], 0, []                            # be: correction bits of the blocks inside the pending end-of-band run

    def flush():
        nonlocal eobrun, be
        if eobrun:
            out.extend(_eobrun_tokens(eobrun))
            eobrun = 0
        out.extend(("B", b, 1) for b in be)
        be = []

    for _, blk in blocks:
        row = cz[blk]
        a = [abs(int(row[k])) >> al for k in range(64)]
        eob = max([k for k in range(ss, se + 1) if a[k] == 1], default=-1)      # the last newly non-zero coefficient
        r, br = 0, []
        for k in range(ss, se + 1):
            if a[k] == 0:
                r += 1
                continue
            while r > 15 and k <= eob:
                flush()
                out.append(("S", 0, 0xF0))
                r -= 16
                out.extend(("B", b, 1) for b in br)
                br = []
            if a[k] > 1:
                br.append(a[k] & 1)
                continue
            flush()
            out.append(("S", 0, (r << 4) | 1))
            out.append(("B", 0 if row[k] < 0 else 1, 1))
            out.extend(("B", b, 1) for b in br)
            br, r = [], 0
        if r > 0 or br:
            eobrun += 1
            be += br
            if eobrun == max_eobrun:
                flush()
    flush()
    return out


# ---- the file ---------------------------------------------------------------------------------------------------------------------
def _segment(marker: int, payload: bytes) -> bytes:
    return bytes([0xFF, marker]) + (len(payload) + 2).to_bytes(2, "big") + payload


def _header(data: bytes):
    """(the source's segments up to its first SOS without DHT, SOF re-marked SOF2; the frame's component ids)"""
    out, ids, i = bytearray(data[:2]), None, 2
    while True:
        m, ln = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        if m == 0xDA:
            return bytes(out), ids
        p = data[i + 4:i + 2 + ln]
        if m in (0xC0, 0xC2):
            ids = [p[6 + 3 * c] for c in range(p[5])]
            out += _segment(0xC2, p)
        elif m != 0xC4:
            out += data[i:i + 2 + ln]
        i += 2 + ln


def _entropy_bytes(tokens, codes) -> bytes:
    parts, acc, n = [], 0, 0
    for kind, a, b in tokens:
        if kind == "S":
            a, b = codes[a][b]
        acc = (acc << b) | a
        n += b
        if n >= 1024:                                      # whole bytes leave the accumulator
            keep = n & 7
            parts.append((acc >> keep).to_bytes(n >> 3, "big"))
            acc &= (1 << keep) - 1
            n = keep
    pad = -n % 8                                           # the last byte is filled with ones
    parts.append(((acc << pad) | ((1 << pad) - 1)).to_bytes((n + pad) // 8, "big"))
    return b"".join(parts).replace(b"\xff", b"\xff\x00")


def rescan(data: bytes, script, tables: str = "optimal", table_ids: str = "per_kind", max_eobrun: int = 0x7FFF) -> bytes:
    assert tables in ("optimal", "flat", "deep") and table_ids in ("one", "per_kind") and 1 <= max_eobrun <= 0x7FFF
    info = parse_progressive_jpeg(data)
    if info is not None:
        coef, status = P.coefficients(info)
        assert status == 0
    else:
        info = parse_jpeg(data)
        coef = J.coefficients(info)
    cz = coef[:, ZZ].tolist()                              # zigzag order
    g = P.Geometry(info)
    head, ids = _header(data)
    out = bytearray(head)
    for comps, ss, se, ah, al in script:
        comps = tuple(comps)
        blocks = g.scan_blocks(comps)
        dc = ss == 0
        if dc and ah == 0:
            tokens = enc_dc_first(cz, blocks, len(comps), al)
        elif dc:
            tokens = enc_dc_refine(cz, blocks, al)
        elif ah == 0:
            tokens = enc_ac_first(cz, blocks, ss, se, al, max_eobrun)
        else:
            tokens = enc_ac_refine(cz, blocks, ss, se, al, max_eobrun)
        # table ids: slot k of a first DC scan is component comps[k]'s table; AC scans have the one slot 0
        if table_ids == "one":
            tid = {k: 0 for k in range(len(comps))}
        elif dc:
            tid = {k: c for k, c in enumerate(comps)}
        else:
            tid = {0: comps[0] if ah == 0 else 3}
        freq = {}
        for kind, a, b in tokens:
            if kind == "S":
                f = freq.setdefault(tid[a], {})
                f[b] = f.get(b, 0) + 1
        codes_by_id = {}
        for t, f in sorted(freq.items()):
            bits, vals = flat_table(dc) if tables == "flat" else optimal_table(f) if tables == "optimal" else deep_table(f)
            out += _segment(0xC4, bytes([(0 if dc else 16) | t]) + bytes(bits) + bytes(vals))
            codes_by_id[t] = code_words(bits, vals)
        sel = b"".join(bytes([ids[c], (tid.get(k, 0) << 4) if dc else tid[0]]) for k, c in enumerate(comps))
        out += _segment(0xDA, bytes([len(comps)]) + sel + bytes([ss, se, (ah << 4) | al]))
        out += _entropy_bytes(tokens, {k: codes_by_id[t] for k, t in tid.items() if t in codes_by_id})
    return bytes(out) + b"\xff\xd9"
