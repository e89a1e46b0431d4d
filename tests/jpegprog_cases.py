"""The progressive JPEG files the decoder tests share, written by PIL at run time: every sampling x quality x size of the matrix,
optimised tables, a flat picture (end-of-band runs over hundreds of blocks) and uniform noise at quality 95 (dense refinement
scans).  cases() -> {name: bytes}; reference(data) -> PIL's pixels.

script_cases() -> {name: ScriptCase}: the coefficients of the smallest of those files that are no whole MCUs, sent again with the
scan scripts PIL never writes (tests/jpegprog_enc_np.py): pure spectral selection, DC scans of one component with refinements,
deep successive approximation, 64 and 65 scans, bands that refinements split or join, component after component, an end-of-band
run cut at 32767, end-of-band runs over blocks that take correction bits, flat and deep Huffman tables, one table id, more
tables than a decoder plans, and files whose script ends above Al = 0."""
from __future__ import annotations

import functools
import io
from dataclasses import dataclass
from typing import Optional

import numpy as np
from PIL import Image

SAMPLINGS = {"grey": None, "444": 0, "422": 1, "420": 2}
SIZES = [(1, 1), (8, 8), (17, 13), (33, 47), (200, 150)]          # (width, height)
QUALITIES = [30, 75, 95]


def picture(w: int, h: int, seed: int = 0) -> np.ndarray:
    """Smooth colour gradients under mild noise: every scan kind gets symbols, no band is empty."""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[:h, :w]
    a = np.stack([128 + 100 * np.sin(x / 7.0) * np.cos(y / 5.0), x * 255.0 / max(w - 1, 1), y * 255.0 / max(h - 1, 1)], -1)
    return np.clip(a + rng.normal(0, 8, (h, w, 3)), 0, 255).astype(np.uint8)


def encode(rgb: np.ndarray, sampling: str = "420", progressive: bool = True, **kw) -> bytes:
    buf = io.BytesIO()
    ss = SAMPLINGS[sampling]
    im = Image.fromarray(rgb[..., 0] if ss is None else rgb)
    im.save(buf, "JPEG", progressive=progressive, **({} if ss is None else {"subsampling": ss}), **kw)
    return buf.getvalue()


def reference(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


@functools.lru_cache(maxsize=None)
def cases() -> dict:
    out = {}
    for name in SAMPLINGS:
        for q in QUALITIES:
            for (w, h) in SIZES:
                out[f"{name}-q{q}-{w}x{h}"] = encode(picture(w, h, seed=w * 1000 + h + q), name, quality=q)
        out[f"{name}-optimize"] = encode(picture(33, 47, seed=5), name, quality=75, optimize=True)
    out["flat-256"] = encode(np.full((256, 256, 3), 77, np.uint8), "420", quality=75)
    out["noise-64-q95"] = encode(np.random.default_rng(1).integers(0, 256, (64, 64, 3), dtype=np.uint8), "444", quality=95)
    return out


def truncated() -> bytes:
    """A 4:2:0 file cut in the middle of its fifth scan."""
    from poco_amd.jpeg import parse_progressive_jpeg
    data = cases()["420-q75-200x150"]
    sc = parse_progressive_jpeg(data).scans[4]
    return data[:sc.offset + sc.length // 2]


# ---- scan scripts PIL never writes ------------------------------------------------------------------------------------------------
@dataclass(frozen=True)
class ScriptCase:
    kind: str
    data: bytes
    source: Optional[bytes]            # the file whose coefficients these are: PIL's pixels of both are equal when `complete`
    script: Optional[tuple]            # ((components, Ss, Se, Ah, Al), ...), None for a file cut out of a PIL file
    parses: bool = True                # parse_progressive_jpeg accepts it
    complete: bool = True              # every bit of every coefficient is sent
    decodable: bool = True             # parses and fits a decoder: the device gives PIL's pixels
    big: bool = False


SMALL_SOURCES = [f"{s}-q95-{w}x{h}" for s in ("420", "422", "444") for (w, h) in ((33, 47), (17, 13))] + ["grey-q95-33x47"]
EOB_CAP_SIDE = 1456                    # 182 x 182 = 33124 blocks: more than one end-of-band run (32767) holds


def _chain(comps, ss, se, first_al):
    """A first scan at Al = first_al and its refinements down to 0."""
    return [(comps, ss, se, 0, first_al)] + [(comps, ss, se, a, a - 1) for a in range(first_al, 0, -1)]


def _all(nc):
    return tuple(range(nc))


def scripts(nc: int) -> dict:
    """{kind: script} for a file of nc components."""
    each = [(c,) for c in range(nc)]
    out = {
        "spectral": [(_all(nc), 0, 0, 0, 0)] + [(c, 1, 63, 0, 0) for c in each],
        "deep": _chain(_all(nc), 0, 0, 3) + [s for c in each for s in _chain(c, 1, 63, 4)],
        "resplit-join": [(_all(nc), 0, 0, 0, 0)] + [(c, a, b, 0, 1) for c in each for a, b in ((1, 2), (3, 9), (10, 63))]
                        + [(c, 1, 63, 1, 0) for c in each],
        "resplit-split": [(_all(nc), 0, 0, 0, 0)] + [(c, 1, 63, 0, 1) for c in each]
                         + [(c, a, b, 1, 0) for c in each for a, b in ((10, 63), (1, 2), (3, 9))],
        # refinements of bands whose blocks keep their history but gain nothing: the run's blocks take correction bits only
        "eob-corrections": [(_all(nc), 0, 0, 0, 0)] + [s for c in each for s in _chain(c, 1, 2, 2) + _chain(c, 3, 63, 1)],
        "stops-at-1": [(_all(nc), 0, 0, 0, 0)] + [(c, 1, 63, 0, 1) for c in each],
    }
    if nc == 3:
        y, cb, cr = each
        out["dc-split"] = [(y, 0, 0, 0, 2), (cb, 0, 0, 0, 2), (y, 1, 63, 0, 0), (cr, 0, 0, 0, 2), (y, 0, 0, 2, 1), (cb, 1, 63, 0, 0),
                           (cb, 0, 0, 2, 1), (cr, 1, 63, 0, 0), (cr, 0, 0, 2, 1), (y, 0, 0, 1, 0), (cb, 0, 0, 1, 0), (cr, 0, 0, 1, 0)]
        out["component-major"] = [s for c in each for s in [(c, 0, 0, 0, 0)] + _chain(c, 1, 5, 1) + _chain(c, 6, 63, 1)]
    else:
        out["bands-64"] = [((0,), 0, 0, 0, 0)] + [((0,), k, k, 0, 0) for k in range(1, 64)]
        out["bands-65"] = _chain((0,), 0, 0, 1) + [((0,), k, k, 0, 0) for k in range(1, 64)]
    return out


def script_of(data: bytes) -> list:
    from poco_amd.jpeg import _parse_progressive
    return [(s.comps, s.ss, s.se, s.ah, s.al) for s in _parse_progressive(data).scans]


def cut_after(data: bytes, nscans: int) -> bytes:
    """The file's first scans and an EOI: complete scans, but the script ends above Al = 0."""
    from poco_amd.jpeg import _parse_progressive
    sc = _parse_progressive(data).scans[nscans - 1]
    return data[:sc.offset + sc.length] + b"\xff\xd9"


def eob_cap_picture() -> np.ndarray:
    a = np.full((EOB_CAP_SIDE, EOB_CAP_SIDE, 3), 128, np.uint8)
    tex = np.random.default_rng(3).integers(0, 256, (8, 8, 1), dtype=np.uint8)
    a[:8, :8] = tex
    a[-8:, -8:] = tex[::-1]
    return a


@functools.lru_cache(maxsize=None)
def script_cases() -> dict:
    from tests.jpegprog_enc_np import rescan
    src = cases()
    out = {}

    def add(name, kind, source, script, **kw):
        rs = {k: kw.pop(k) for k in ("tables", "table_ids", "max_eobrun") if k in kw}
        out[name] = ScriptCase(kind, rescan(source, script, **rs), source, tuple(script), **kw)

    for sname in SMALL_SOURCES:
        data = src[sname]
        nc = 1 if sname.startswith("grey") else 3
        for kind, script in scripts(nc).items():
            if kind == "dc-split" and sname.startswith("444"):
                continue                                   # (luma's raster is the MCU raster there)
            if kind == "bands-64":
                add(f"bands-64-{sname}", kind, data, script, tables="flat")
                add(f"tables-many-{sname}", "tables-many", data, script, decodable=False)
            elif kind == "bands-65":
                add(f"bands-65-{sname}", kind, data, script, tables="flat", parses=False, decodable=False)
            elif kind == "stops-at-1":
                add(f"ends-above-zero-{sname}", "ends-above-zero", data, script, parses=False, complete=False, decodable=False)
            elif kind == "deep":                           # one DC table and 15 AC tables: all a decoder plans per image
                add(f"deep-{sname}", kind, data, script, table_ids="one")
            else:
                add(f"{kind}-{sname}", kind, data, script)
    for sname in ("420-q95-33x47", "grey-q95-33x47"):
        pil = script_of(src[sname])                        # libjpeg's default script, with tables it never writes
        add(f"tables-flat-{sname}", "tables-flat", src[sname], pil, tables="flat")
        add(f"tables-deep-{sname}", "tables-deep", src[sname], pil, tables="deep")
        add(f"tables-one-id-{sname}", "tables-one-id", src[sname], pil, table_ids="one")
    for sname, n in (("420-q75-200x150", 5), ("444-q95-33x47", 5), ("grey-q75-33x47", 3)):
        out[f"ends-above-zero-cut-{sname}"] = ScriptCase("ends-above-zero", cut_after(src[sname], n), src[sname], None, parses=False,
                                                         complete=False, decodable=False)
    big = encode(eob_cap_picture(), "grey", quality=75)
    add("eob-cap", "eob-cap", big, [((0,), 0, 0, 0, 0), ((0,), 1, 63, 0, 1), ((0,), 1, 63, 1, 0)], big=True)
    return out
