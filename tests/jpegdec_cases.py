"""The baseline JPEG files the decoder tests share beyond tests/test_jpegdec_cpu.py's fixture_set(): streams libjpeg's writer never
makes, transcoded (tests/jpegbase_enc_np.py) from small files PIL wrote.  hand_cases() -> {name: bytes}, cached.

    tables-*     {optimal, flat, deep} tables x {shared, swapped, per_component} table ids on 4:2:0 and 4:4:4 (33x47 all nine, 17x13
                 a rotation), three on 4:2:2, {flat, deep} on grey; DHT segments alternate between one per table and one for all
    dri*         restart intervals of 1 MCU (9, 192 and 375 intervals), of 7 MCUs (RSTm wraps), of the whole picture (declared, no
                 marker), and of 1 MCU under deep tables per component
    boundary-*   one stream per property of a subsequence boundary (BOUNDARY: counter -> case), found by a bounded search over the
                 noise source's seed and an edit of block 0 that shifts the phase of every later bit
    extreme-*    DC differences of category 11 of both signs (a checkerboard), and edited blocks: symbol 0xFA, three ZRLs in front
                 of coefficient 63, blocks whose 63 AC coefficients are all non-zero
    slow-sync    the flat-table recoding of the noise source that needs the most rounds of jdec_sync's loop (SLOW_SYNC_ROUNDS)
Nothing is larger than 200x150.  Edits with large values go to quality-100 sources, where every quantiser step is 1 and the
samples stay inside libjpeg's range-limit table."""
from __future__ import annotations

import functools
import io
import itertools

import numpy as np
from PIL import Image

from poco_amd import jpeg
from tests import jpegdec_np as J
from tests.jpegbase_enc_np import recode
from tests.test_jpeg_cpu import photo_like

SAMPLINGS = {"420": "4:2:0", "422": "4:2:2", "444": "4:4:4", "grey": "gray"}
TABLES = ("optimal", "flat", "deep")
IDS = ("shared", "swapped", "per_component")
NOISE_SEEDS = (7, 8, 9)
PHASES = 24                                             # phase m: the first m AC coefficients of block 0 are zeroed
BOUNDARY = {"ff_straddles": "boundary-ff-straddles-dri48", "ff_before_boundary": "boundary-ff-before",
            "long_symbol_straddles": "boundary-long-symbol-deep-dri16", "aligned_block_ends": "boundary-aligned-block-end"}
LATER_INTERVAL = ("ff_straddles", "long_symbol_straddles")      # these must hold in a restart interval that is not the first
# jpegdec_np.sync_rounds of "slow-sync" as found when the case was written: quality-100 noise has no EOB and flat tables are the same
# for every component, so a lane that starts from a guess never finds the zigzag index - every lane waits for its predecessor
SLOW_SYNC_ROUNDS = 494


def pil_jpeg(img: np.ndarray, sampling: str, quality: int) -> bytes:
    buf = io.BytesIO()
    if sampling == "gray":
        Image.fromarray(np.ascontiguousarray(img[..., 1])).save(buf, "JPEG", quality=quality)
    else:
        Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling=sampling)
    return buf.getvalue()


@functools.lru_cache(maxsize=None)
def source(kind: str, H: int = 0, W: int = 0, seed: int = 0) -> bytes:
    if kind == "noise":
        return pil_jpeg(np.random.default_rng(seed).integers(0, 256, (96, 128, 3), dtype=np.uint8), "4:4:4", 100)
    if kind == "checker":
        y, x = np.mgrid[:64, :64]
        a = (((y // 8 + x // 8) & 1) * 255).astype(np.uint8)
        return pil_jpeg(np.stack([a, a, a], -1), "4:4:4", 100)
    return pil_jpeg(photo_like(H, W, seed=H * 1000 + W), SAMPLINGS[kind], 95)


def clear_block(blk: int, keep=()):
    """Edits that zero the AC coefficients of a block and then set `keep` = [(zigzag index, value)]."""
    keep = dict(keep)
    return [(blk, k, keep.get(k, 0)) for k in range(1, 64)]


def extreme_edits():
    """Blocks 2 .. 7 of the noise source (4:4:4: luma, Cb and Cr of MCUs 0 .. 2)."""
    full = [(k, (1 + k % 3) * (-1 if k & 1 else 1)) for k in range(1, 64)]
    return (clear_block(2, [(1, 5), (17, 600), (33, -512), (49, 512), (63, -1)])        # 0xFA three times, then run 13 to 63
            + clear_block(3, [(63, 3)]) + clear_block(4, [(63, -1023)])                   # three ZRLs and coefficient 63
            + clear_block(5, full) + clear_block(6, full) + clear_block(7, [(16, 1023), (63, 1)]))


def _boundary_case(prop: str, tables: str, ids: str, dri: int):
    """The first stream of the candidate list (seed x phase) in which `prop` is counted - in a later restart interval
    where LATER_INTERVAL asks for it.  The two FF properties are read off the bytes, the others need the symbols."""
    for seed, m in itertools.product(NOISE_SEEDS, range(PHASES)):
        data = recode(source("noise", seed=seed), tables, ids, dri, edit=[(0, k, 0) for k in range(1, m + 1)])
        if prop.startswith("ff_"):
            st = J.new_stats()
            J.boundary_ff(jpeg.parse_jpeg(data), st)
        else:
            st = J.new_stats()
            J.coefficients(jpeg.parse_jpeg(data), st)
        if (st["later_intervals"] if prop in LATER_INTERVAL else st)[prop] > 0:
            return data
    raise AssertionError(f"no candidate has {prop}")


def _slow_sync():
    cands = [recode(source("noise", seed=NOISE_SEEDS[0]), "flat", "shared", 0, edit=e) for e in ([], [(0, 1, 1)])]
    return max(cands, key=J.sync_rounds)


@functools.lru_cache(maxsize=None)
def hand_cases() -> dict:
    out = {}
    k = 0
    for s, (H, W) in itertools.product(("420", "444"), ((47, 33), (13, 17))):
        for j, (t, ids) in enumerate(itertools.product(TABLES, IDS)):
            if H == 13 and j % 3 != (j // 3 + k) % 3:      # the small picture: three of the nine, every table and id layout once
                continue
            out[f"tables-{t}-{ids}-{s}-{W}x{H}"] = recode(source(s, H, W), t, ids, dht=("each", "joined")[(j + k) & 1])
        k += 1
    for t, ids, (H, W) in (("deep", "per_component", (47, 33)), ("flat", "swapped", (47, 33)), ("optimal", "per_component", (13, 17))):
        out[f"tables-{t}-{ids}-422-{W}x{H}"] = recode(source("422", H, W), t, ids, dht="joined")
    for t, ids, (H, W) in (("flat", "shared", (47, 33)), ("deep", "swapped", (47, 33)), ("deep", "shared", (13, 17))):
        out[f"tables-{t}-{ids}-grey-{W}x{H}"] = recode(source("grey", H, W), t, ids)
    big = pil_jpeg(photo_like(120, 200, seed=3), "4:4:4", 75)                  # 15 x 25 MCUs
    out["dri1-420-33x47"] = recode(source("420", 47, 33), "optimal", "shared", 1)
    out["dri1-noise"] = recode(source("noise", seed=7), "optimal", "shared", 1)
    out["dri1-444-200x120"] = recode(big, "optimal", "swapped", 1, dht="joined")
    out["dri1-deep-per_component-420-33x47"] = recode(source("420", 47, 33), "deep", "per_component", 1)
    out["dri1-deep-per_component-444-200x120"] = recode(big, "deep", "per_component", 1)
    out["dri7-444-33x47"] = recode(source("444", 47, 33), "flat", "shared", 7)
    out["dri7-noise"] = recode(source("noise", seed=8), "optimal", "per_component", 7)
    out["dri-whole-420-33x47"] = recode(source("420", 47, 33), "optimal", "shared", 9)      # 3 x 3 MCUs: declared, no marker
    out[BOUNDARY["ff_straddles"]] = _boundary_case("ff_straddles", "optimal", "shared", 48)
    out[BOUNDARY["ff_before_boundary"]] = _boundary_case("ff_before_boundary", "optimal", "shared", 0)
    out[BOUNDARY["long_symbol_straddles"]] = _boundary_case("long_symbol_straddles", "deep", "per_component", 16)
    out[BOUNDARY["aligned_block_ends"]] = _boundary_case("aligned_block_ends", "optimal", "swapped", 0)
    out["extreme-dc11-checkerboard"] = recode(source("checker"), "optimal", "shared")
    out["extreme-dc11-checkerboard-deep"] = recode(source("checker"), "deep", "per_component", 3)
    out["extreme-edited-blocks"] = recode(source("noise", seed=9), "optimal", "shared", edit=extreme_edits())
    out["extreme-edited-blocks-deep"] = recode(source("noise", seed=9), "deep", "swapped", 5, edit=extreme_edits(), dht="joined")
    out["slow-sync"] = _slow_sync()
    return out


def unowned_code(data: bytes, after: int = 300):
    """(the stream with the first symbol that starts on a byte, `after` bytes or more into its scan, overwritten by sixteen
    1-bits - stuffed: FF 00 FF 00 -, the index of that byte).  No Huffman code is all ones, so this is a window without a code."""
    info = jpeg.parse_jpeg(data)
    _, comp_of = J._geometry(info)
    tabs = [(J.HuffTable(*info.dc[c]), J.HuffTable(*info.ac[c])) for c in range(info.ncomp)]
    lo, hi = info.scan_offset, info.scan_offset + int(info.segments[0, 1])
    for stop in range(lo + after, hi - 8):
        bp, bo, _, _ = J.decode_span(data, hi, (lo, 0, 0, 0), stop, tabs, comp_of, True)[0]
        if bo == 0:
            q = bp
            for _ in range(2):
                q += 2 if data[q] == 0xFF else 1
            return data[:bp] + b"\xff\x00\xff\x00" + data[q:], bp
    raise AssertionError("no symbol starts on a byte")
