"""The contract of poco_op_corrupt (include/poco_hip.h) in its executable form: plain float64 loops over the taps
and cells of one plane at a time (numpy carries the pixels; every pixel's operations happen in the order written), its own
Philox4x32-10, nothing shared with poco_amd.  A step takes and returns float64 arrays holding fp32 values: it evaluates in float64, clamps to [0, 255] and rounds once to fp32.  The blur is checked against scipy.ndimage.gaussian_filter and
the jpeg step (tests/jpeg_np.py + tests/jpegdec_np.py composed, libjpeg's integer arithmetic on both sides) against PIL's round trip
in tests/test_corrupt_cpu.py."""
import math

import numpy as np

KINDS = ("none", "gaussian_blur", "motion_blur", "pixelate", "contrast", "gamma", "gaussian_noise", "jpeg")
MEAN = np.array([0.485, 0.456, 0.406], np.float32)
STD = np.array([0.229, 0.224, 0.225], np.float32)
M32 = 0xFFFFFFFF


def mirror(i: int, n: int) -> int:
    """scipy.ndimage mode='mirror': the edge sample is not repeated; reflects as often as needed."""
    if n == 1:
        return 0
    period = 2 * (n - 1)
    m = i % period
    return m if m < n else period - m


def store(v) -> np.ndarray:
    """clamp to [0, 255], round once to fp32 (returned as float64 for the next step)"""
    return np.clip(np.asarray(v, np.float64), 0.0, 255.0).astype(np.float32).astype(np.float64)


def blur_weights(sigma: float):
    sigma = float(np.float32(sigma))
    r = int(3.0 * sigma + 0.5)
    w = [math.exp(-(float(k) * float(k)) / (2.0 * sigma * sigma)) for k in range(-r, r + 1)]
    s = 0.0
    for x in w:
        s = s + x
    return r, [x / s for x in w]


def mirror_index(n: int, shift: int) -> np.ndarray:
    return np.array([mirror(i + shift, n) for i in range(n)], np.int64)


def mirror_table(n: int) -> np.ndarray:
    """mirror(i, n) for i = -64 .. n + 63 at index i + 64"""
    return np.array([mirror(i, n) for i in range(-64, n + 64)], np.int64)


def gaussian_blur_plane(p: np.ndarray, sigma: float) -> np.ndarray:
    """float64 result BEFORE the store: horizontal pass, then vertical, both summed in the order k = -r .. r (the loop is over the
    taps; every pixel's additions happen in that order)."""
    H, W = p.shape
    r, w = blur_weights(sigma)
    h = np.zeros((H, W))
    for k in range(-r, r + 1):
        h = h + w[k + r] * p[:, mirror_index(W, k)]
    out = np.zeros((H, W))
    for k in range(-r, r + 1):
        out = out + w[k + r] * h[mirror_index(H, k), :]
    return out


def motion_blur_plane(p: np.ndarray, L: int, dx: float, dy: float) -> np.ndarray:
    H, W = p.shape
    dx, dy = float(np.float32(dx)), float(np.float32(dy))
    half = (L - 1) // 2
    ys, xs = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
    mir = lambda a, n: mirror_table(n)[a.astype(np.int64) + 64]                          # noqa: E731  (|k| <= 15: taps stay within 64)
    s = np.zeros((H, W))
    for k in range(-half, half + 1):
        sx, sy = xs + float(k) * dx, ys + float(k) * dy
        x0, y0 = np.floor(sx), np.floor(sy)
        fx, fy = sx - x0, sy - y0
        xa, xb, ya, yb = mir(x0, W), mir(x0 + 1, W), mir(y0, H), mir(y0 + 1, H)
        top = (1.0 - fx) * p[ya, xa] + fx * p[ya, xb]
        bot = (1.0 - fx) * p[yb, xa] + fx * p[yb, xb]
        s = s + ((1.0 - fy) * top + fy * bot)
    return s / float(L)


def pixelate_plane(p: np.ndarray, f: int) -> np.ndarray:
    H, W = p.shape
    out = np.zeros((H, W))
    for ya in range(0, H, f):
        yb = min(ya + f, H)
        for xa in range(0, W, f):
            xb = min(xa + f, W)
            s = 0.0
            for x in range(xa, xb):
                col = 0.0
                for y in range(ya, yb):
                    col = col + p[y, x]
                s = s + col
            out[ya:yb, xa:xb] = s / float((xb - xa) * (yb - ya))
    return out


def plane_mean(p: np.ndarray) -> float:
    """256 lane-strided sums of the row-major plane (lane t adds elements t, t + 256, ... in order), a halving tree, one division."""
    flat = p.reshape(-1)
    rows = -(-flat.size // 256)
    pad = np.zeros(rows * 256)
    pad[:flat.size] = flat
    red = np.zeros(256)
    for row in pad.reshape(rows, 256):          # adding the padding's +0.0 changes no sum
        red = red + row
    o = 128
    while o > 0:
        red[:o] = red[:o] + red[o:2 * o]
        o >>= 1
    return float(red[0]) / float(flat.size)


def contrast_plane(p: np.ndarray, c: float) -> np.ndarray:
    m = plane_mean(p)
    return m + float(np.float32(c)) * (p - m)


def gamma_plane(p: np.ndarray, g: float) -> np.ndarray:
    return 255.0 * np.power(p / 255.0, float(np.float32(g)))


def philox4x32_10(c, k):
    """c = four uint64 arrays (or ints) holding 32-bit counter words, k = the two key words -> four uint64 arrays of output words."""
    c0, c1, c2, c3 = (np.asarray(v, np.uint64) for v in c)
    k0, k1 = int(k[0]), int(k[1])
    m = np.uint64(M32)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        c0, c1, c2, c3 = ((p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)) & m, p1 & m, ((p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)) & m, p0 & m
        k0, k1 = (k0 + 0x9E3779B9) & M32, (k1 + 0xBB67AE85) & M32
    return c0, c1, c2, c3


def normals(count: int, seed: int, stream: int, pos: int) -> np.ndarray:
    """z of elements 0 .. count - 1 of a crop's [3,res,res] block: counter (q, 0, stream, pos) serves elements 4q .. 4q + 3."""
    quads = (count + 3) // 4
    q = np.arange(quads, dtype=np.uint64)
    zero = np.zeros(quads, np.uint64)
    w = philox4x32_10((q, zero, zero + np.uint64(stream & M32), zero + np.uint64(pos)), (seed & M32, (seed >> 32) & M32))
    z = np.zeros((quads, 4))
    for pr in range(2):
        u1, u2 = (w[2 * pr].astype(np.float64) + 1.0) * 2.0 ** -32, w[2 * pr + 1].astype(np.float64) * 2.0 ** -32
        rad, ang = np.sqrt(-2.0 * np.log(u1)), 6.283185307179586 * u2
        z[:, 2 * pr], z[:, 2 * pr + 1] = rad * np.cos(ang), rad * np.sin(ang)
    return z.reshape(-1)[:count]


def jpeg_round_trip(rgb_u8: np.ndarray, quality: int) -> np.ndarray:
    """uint8 [H,W,3] -> uint8 [H,W,3]: the encoder's restatement, then the decoder's."""
    from tests import jpeg_np, jpegdec_np
    return jpegdec_np.decode(jpeg_np.encode(rgb_u8, int(quality)))


def apply_step(crop: np.ndarray, step: dict, pos: int) -> np.ndarray:
    """crop float64 [3,res,res] of fp32 values; step = dict(kind=name, ival, p0, p1, seed, stream) -> the same form."""
    kind = step["kind"]
    if kind == "none":
        return crop
    if kind == "gaussian_noise":
        z = normals(crop.size, int(step.get("seed", 0)), int(step.get("stream", 0)), pos).reshape(crop.shape)
        return store(crop + float(np.float32(step["p0"])) * z)
    if kind == "jpeg":
        u8 = np.floor(crop + 0.5).clip(0, 255).astype(np.uint8)
        return jpeg_round_trip(np.ascontiguousarray(u8.transpose(1, 2, 0)), step["ival"]).transpose(2, 0, 1).astype(np.float64)
    fn = {"gaussian_blur": lambda p: gaussian_blur_plane(p, step["p0"]), "motion_blur": lambda p: motion_blur_plane(p, step["ival"], step["p0"], step["p1"]),
          "pixelate": lambda p: pixelate_plane(p, step["ival"]), "contrast": lambda p: contrast_plane(p, step["p0"]),
          "gamma": lambda p: gamma_plane(p, step["p0"])}[kind]
    return store(np.stack([fn(crop[c]) for c in range(3)]))


def corrupt(x: np.ndarray, chains, normalize: bool = False) -> np.ndarray:
    """x fp32 [N,3,res,res] raw crops, chains[n] = the list of step dicts of crop n -> fp32 [N,3,res,res]."""
    out = []
    for crop, chain in zip(np.asarray(x, np.float32).astype(np.float64), chains):
        for pos, step in enumerate(chain):
            crop = apply_step(crop, step, pos)
        out.append(crop.astype(np.float32))
    out = np.stack(out)
    return normalize_np(out) if normalize else out


def normalize_np(raw: np.ndarray) -> np.ndarray:
    """oracle/crop_np.normalize_np on NCHW float32: three float32 operations."""
    p = raw.astype(np.float32) / np.float32(255.0)
    return ((p - MEAN[None, :, None, None]) / STD[None, :, None, None]).astype(np.float32)


def from_record(rec) -> dict:
    """A step dict from one ops.CORRUPT_STEP record (the tests build records with poco_amd.corrupt and restate from them)."""
    return dict(kind=KINDS[int(rec["kind"])], ival=int(rec["ival"]), p0=float(rec["p0"]), p1=float(rec["p1"]),
                seed=int(rec["seed"][0]) | (int(rec["seed"][1]) << 32), stream=int(rec["stream"]))


def chains_from_records(recs) -> list:
    return [[from_record(r) for r in row if int(r["kind"]) != 0] for row in recs]
