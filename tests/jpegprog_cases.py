"""The progressive JPEG files the decoder tests share, written by PIL at run time: every sampling x quality x size of the matrix,
optimised tables, a flat picture (end-of-band runs over hundreds of blocks) and uniform noise at quality 95 (dense refinement
scans).  cases() -> {name: bytes}; reference(data) -> PIL's pixels."""
from __future__ import annotations

import functools
import io

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
