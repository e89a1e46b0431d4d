"""An entropy-coding transcoder for the baseline decoder's tests: the quantised coefficients of a baseline JPEG file PIL wrote, sent
again as a baseline (SOF0) file with the same frame and DQT but with ANY Huffman table shape, table id layout, restart interval
and - through `edit` - bit phase: what libjpeg's writer never makes.  Plain Python over the tables, code words and segment writer
of tests/jpegprog_enc_np.py; the symbols follow ITU-T T.81 F.1.2.

    recode(data, tables="optimal", table_ids="shared", restart_interval=0, edit=(), dht="each") -> bytes

tables:    "optimal"  from the stream's own symbol counts by Annex K.2
           "flat"     every symbol a class can have: the even ones 8 bits, the odd ones 9
           "deep"     no word shorter than 10 bits: the most used symbol 16 bits, the next 15 ...  Symbols the stream does not
                      use fill the table up to seven, so that it always holds words of every length 10 .. 16
table_ids: "shared"         Y -> 0, chroma -> 1, as PIL writes
           "swapped"        Y -> 1, chroma -> 0
           "per_component"  three distinct pairs: ids 0, 1 and 3
restart_interval: MCUs per interval (0 = none): DRI, RSTm markers that wrap mod 8, 1-bits up to the byte at every interval's end
edit:      [(block in scan order, zigzag index, value)] overwrites of the coefficients (DC as the value, not the difference)
           before coding.  One changed size category in block 0 shifts every later bit by one, new coefficients shift by bytes.
           DC differences must stay within +-2047 and AC coefficients within +-1023: baseline's ranges
dht:       "each"   one DHT segment per table
           "joined" all tables in one DHT segment, AC before DC and the highest id first

The transcoder is pinned on libjpeg alone: PIL decodes what it writes, and without `edit` to the source's pixels."""
from __future__ import annotations

import functools

from poco_amd.jpeg import _ZIGZAG, parse_jpeg
from tests import jpegdec_np as J
from tests.jpegprog_enc_np import _entropy_bytes, _segment, code_words, deep_table, flat_table, optimal_table

ZZ = _ZIGZAG.tolist()
TABLE_IDS = {"shared": (0, 1, 1), "swapped": (1, 0, 0), "per_component": (0, 1, 3)}
_DEEP_FILL = {True: list(range(12)), False: [0x00, 0xF0] + list(range(1, 11))}     # symbols that fill a deep table up


def _header(data: bytes):
    """(the source's segments before its SOS without DHT and DRI, the frame's component ids)"""
    out, ids, i = bytearray(data[:2]), None, 2
    while True:
        m, ln = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        if m == 0xDA:
            return bytes(out), ids
        p = data[i + 4:i + 2 + ln]
        if m == 0xC0:
            ids = [p[6 + 3 * c] for c in range(p[5])]
        if m not in (0xC4, 0xDD):
            out += data[i:i + 2 + ln]
        i += 2 + ln


def _value_bits(v: int):
    n = abs(v).bit_length()
    return (v if v >= 0 else v - 1) & ((1 << n) - 1), n


def block_tokens(row, c: int, pred: int):
    """T.81 F.1.2 for one block in zigzag order: ("S", (class, component), symbol) and ("B", value, bits) tokens."""
    d = row[0] - pred
    assert -2047 <= d <= 2047, "a DC difference outside baseline's range"
    bits, n = _value_bits(d)
    out = [("S", (0, c), n)]
    if n:
        out.append(("B", bits, n))
    r = 0
    for k in range(1, 64):
        v = row[k]
        if v == 0:
            r += 1
            continue
        assert -1023 <= v <= 1023, "an AC coefficient outside baseline's range"
        while r > 15:
            out.append(("S", (1, c), 0xF0))
            r -= 16
        bits, n = _value_bits(v)
        out += [("S", (1, c), (r << 4) | n), ("B", bits, n)]
        r = 0
    if r:
        out.append(("S", (1, c), 0x00))
    return out


@functools.lru_cache(maxsize=16)
def _source(data: bytes):
    """(parse_jpeg's info, the coefficients in zigzag order as rows of a tuple) of a source file"""
    info = parse_jpeg(data)
    assert info is not None, "the source must be a baseline file parse_jpeg takes"
    return info, tuple(map(tuple, J.coefficients(info)[:, ZZ].tolist()))


def recode(data: bytes, tables: str = "optimal", table_ids: str = "shared", restart_interval: int = 0, edit=(),
           dht: str = "each") -> bytes:
    assert tables in ("optimal", "flat", "deep") and table_ids in TABLE_IDS and dht in ("each", "joined")
    assert 0 <= restart_interval <= 0xFFFF
    info, cz = _source(data)
    cz = list(cz)
    for blk, k, v in edit:
        if isinstance(cz[blk], tuple):
            cz[blk] = list(cz[blk])
        cz[blk][k] = int(v)
    _, comp_of = J._geometry(info)
    bpm = len(comp_of)
    nmcu = len(cz) // bpm
    tid = TABLE_IDS[table_ids][:info.ncomp] if info.ncomp == 3 else (TABLE_IDS[table_ids][0],)
    # tokens per restart interval; a symbol's slot is (class, table id)
    step = restart_interval or nmcu
    intervals = []
    for m0 in range(0, nmcu, step):
        pred = [0] * info.ncomp
        toks = []
        for blk in range(m0 * bpm, min(m0 + step, nmcu) * bpm):
            c = comp_of[blk % bpm]
            toks += [(kind, (a[0], tid[a[1]]), b) if kind == "S" else (kind, a, b) for kind, a, b in block_tokens(cz[blk], c, pred[c])]
            pred[c] = cz[blk][0]
        intervals.append(toks)
    freq = {}
    for toks in intervals:
        for kind, a, b in toks:
            if kind == "S":
                f = freq.setdefault(a, {})
                f[b] = f.get(b, 0) + 1
    segs, codes = {}, {}
    for (tc, th), f in sorted(freq.items()):
        if tables == "flat":
            bits, vals = flat_table(tc == 0)
        elif tables == "optimal":
            bits, vals = optimal_table(f)
        else:
            fill = [s for s in _DEEP_FILL[tc == 0] if s not in f][:max(0, 7 - len(f))]
            bits, vals = deep_table({**f, **{s: 0 for s in fill}})
        segs[(tc, th)] = bytes([(tc << 4) | th]) + bytes(bits) + bytes(vals)
        codes[(tc, th)] = code_words(bits, vals)
    head, ids = _header(data)
    out = bytearray(head)
    if dht == "each":
        for key in sorted(segs):
            out += _segment(0xC4, segs[key])
    else:
        out += _segment(0xC4, b"".join(segs[key] for key in sorted(segs, reverse=True)))
    if restart_interval:
        out += _segment(0xDD, restart_interval.to_bytes(2, "big"))
    sel = b"".join(bytes([ids[c], (tid[c] << 4) | tid[c]]) for c in range(info.ncomp))
    out += _segment(0xDA, bytes([info.ncomp]) + sel + bytes([0, 63, 0]))
    for i, toks in enumerate(intervals):
        if i:
            out += bytes([0xFF, 0xD0 + (i - 1) % 8])
        out += _entropy_bytes(toks, codes)
    return bytes(out) + b"\xff\xd9"
