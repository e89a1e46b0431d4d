"""GPU: poco_op_corrupt / ops.corrupt against tests/corrupt_np.py (include/poco_hip.h).

Shapes: N = 3 crops at res 1, 2, 7, 33 (one tile and its partial forms), 65 (3 x 3 tiles, the last one pixel wide) and N = 2 at 224
(7 x 7 whole tiles).  Every kind alone at both ends of its range; batches in which every crop carries another chain, one of four
steps with a jpeg step inside; poisoned guard bands around both buffers; a crop alone against the same crop inside a batch; the
normalised output.

Tolerances.  pixelate, contrast, gamma, both blurs and the noise: 2^-15 against the restatement rounded to fp32 - both sides evaluate
one fp64 formula, libm's exp / pow / log / sin / cos may differ in the last place of fp64 and so flip the one rounding to fp32.  jpeg:
equal byte for byte.  A chain is checked step by step: the device's own output of the first p - 1 steps (a run with the chain cut
there) is the input the restatement's step p gets, so that a flipped rounding of one step is not amplified by the next (gamma 5, or
a whole grey level through jpeg's byte rounding) into the tolerance of another.
Normalised: device and restatement apply the same three fp32 operations p = v / 255, q = p - mean, r = q / std to raw values at most
d = 2^-15 apart.  |p| <= 1 and |q| < 1, so each side rounds p and q by at most 2^-25; |r| < 4, so r by at most 2^-23; the smallest std is
0.224:  |r_dev - r_ref| <= (d / 255 + 4 * 2^-25) / 0.224 + 2 * 2^-23 = 1.31e-6.  Where the raw words are equal the normalised words are equal.
The jpeg restatement (pure Python entropy coding) serves res <= 33; above, PIL's round trip stands in for it:
tests/test_corrupt_cpu.py holds the two equal byte for byte."""
import io

import numpy as np
import pytest
import torch

from poco_amd import corrupt, ops
from tests import corrupt_np

pytestmark = pytest.mark.gpu
TOL = 2.0 ** -15
NORM_TOL = (TOL / 255.0 + 4 * 2.0 ** -25) / 0.224 + 2 * 2.0 ** -23
SHAPES = [(3, 1), (3, 2), (3, 7), (3, 33), (3, 65), (2, 224)]
WORST = {}


def crops(N, res, seed=0):
    r = np.random.default_rng(1000 * res + seed)
    x = r.uniform(0, 255, (N, 3, res, res)).astype(np.float32)
    flat = x.reshape(-1)
    flat[::7], flat[3::11] = 0.0, 255.0                                   # the ends of the range are there too
    return x


def run(x_np, recs, normalize=False, dev="cuda"):
    """ops.corrupt with the input and both buffers inside poisoned allocations; asserts that nothing outside them was written."""
    n = x_np.size
    guard = 4096
    bufs = []
    for _ in range(3):
        flat = torch.empty(n + 2 * guard, device=dev, dtype=torch.float32)
        flat.view(torch.int32).fill_(ops.POISON_BITS)
        bufs.append(flat)
    view = lambda f: f[guard:guard + n].view(x_np.shape)                 # noqa: E731
    view(bufs[0]).copy_(torch.from_numpy(x_np))
    out = ops.corrupt(view(bufs[0]), recs, normalize, out=view(bufs[1]), tmp=view(bufs[2]))
    torch.cuda.synchronize()
    assert out.data_ptr() == view(bufs[1]).data_ptr()
    for f in bufs:
        g = f.view(torch.int32)
        assert bool((g[:guard] == ops.POISON_BITS).all()) and bool((g[guard + n:] == ops.POISON_BITS).all()), "a guard band was written"
    assert np.array_equal(view(bufs[0]).cpu().numpy(), x_np), "the input was written"
    return out.cpu().numpy()


def pil_round_trip(rgb, q):
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(rgb).save(f, "JPEG", quality=int(q), subsampling=2)
    return np.array(Image.open(io.BytesIO(f.getvalue())).convert("RGB"))


def restate_step(prev, rec_col, pos):
    """One chain position of the restatement on `prev` fp32 [N,3,res,res]."""
    out = []
    for crop, rec in zip(prev.astype(np.float64), rec_col):
        step = corrupt_np.from_record(rec)
        if step["kind"] == "jpeg" and crop.shape[-1] > 33:
            u8 = np.floor(crop + 0.5).clip(0, 255).astype(np.uint8)
            out.append(pil_round_trip(np.ascontiguousarray(u8.transpose(1, 2, 0)), step["ival"]).transpose(2, 0, 1).astype(np.float32))
        else:
            out.append(corrupt_np.apply_step(crop, step, pos).astype(np.float32))
    return np.stack(out)


def check(x, recs):
    """The device's chain against the restatement, step by step (module docstring); returns the device's final output."""
    prev = x
    for p in range(recs.shape[1]):
        if not (recs["kind"][:, p] != 0).any():
            break
        cut = recs.copy()
        cut[:, p + 1:] = np.zeros((), ops.CORRUPT_STEP)
        got, want = run(x, cut), restate_step(prev, recs[:, p], p)
        for n in range(len(x)):
            kind = ops.CORRUPT_KINDS[int(recs["kind"][n, p])]
            dev = float(np.abs(got[n].astype(np.float64) - want[n]).max())
            WORST[kind] = max(WORST.get(kind, 0.0), dev)
            assert dev <= (0.0 if kind in ("jpeg", "none") else TOL), (kind, n, p, dev)
        assert got.min() >= 0.0 and got.max() <= 255.0
        prev = got
    return prev


ENDS = ["gaussian_blur:0.05", "gaussian_blur:0.4", "gaussian_blur:5", "motion_blur:3:0", "motion_blur:31:37", "motion_blur:9:-120", "pixelate:2",
        "pixelate:3", "pixelate:32", "contrast:0", "contrast:2", "gamma:0.2", "gamma:5", "gaussian_noise:0", "gaussian_noise:255", "jpeg:1", "jpeg:100"]


@pytest.mark.parametrize("N,res", SHAPES)
def test_every_kind_alone_at_its_range_ends(N, res, cuda):
    x = crops(N, res)
    for text in ENDS:
        level = corrupt.parse_levels(text)[1]
        got = check(x, corrupt.records([level] * N, list(range(40, 40 + N)), seed=(3 << 32) | 99))
        if text in ("gaussian_blur:0.05", "gaussian_noise:0"):
            assert np.array_equal(got, x)                                 # radius 0 and sigma 0 are the identity
        elif res > 2 and text not in ("contrast:0",):
            assert not np.array_equal(got, x), text
    print(f"res {res}: largest deviation per kind " + ", ".join(f"{k} {v:.3e}" for k, v in sorted(WORST.items())) + f" (tol {TOL:.3e})")


MIXES = ["gaussian_blur:1.5+jpeg:30+gaussian_noise:8+gamma:0.7,pixelate:5,motion_blur:7:45+contrast:1.5",
         "gaussian_noise:20+gaussian_noise:20,jpeg:60+pixelate:4+jpeg:15,gamma:2.2+gaussian_blur:3+motion_blur:5:90+contrast:0.5"]


@pytest.mark.parametrize("N,res", [(3, 7), (3, 33), (3, 65), (2, 224)])
@pytest.mark.parametrize("mix", MIXES)
def test_every_crop_of_a_batch_with_its_own_chain(N, res, mix, cuda):
    levels = corrupt.parse_levels(mix)[1:]
    if N == 2:
        levels = [max(levels, key=len), ()]
    assert max(len(lv) for lv in levels) == 4
    x = crops(N, res, 1)
    recs = corrupt.records(levels, [7, 8, 9][:N], seed=5)
    whole = run(x, recs)
    assert np.array_equal(check(x, recs), whole)                          # the chain cut after its last step is the chain
    if N == 2:
        assert np.array_equal(whole[1], x[1])                             # an empty chain copies
    # the two noise steps of one chain draw from different counters (the chain position is one of its words)
    if N == 3 and mix.startswith("gaussian_noise"):
        one = run(x, corrupt.records([levels[0][:1]] * N, [7, 8, 9][:N], seed=5))
        assert not np.array_equal(whole[0] - one[0], one[0] - x[0])


@pytest.mark.parametrize("N,res", [(3, 33), (2, 224)])
def test_a_crop_alone_and_inside_a_batch_gives_the_same_bits(N, res, cuda):
    x = crops(N, res, 2)
    levels = corrupt.parse_levels("gaussian_blur:2+gaussian_noise:12+contrast:1.3,pixelate:6+jpeg:40,motion_blur:11:20+gamma:1.8")[1:][:N]
    streams = [100, 200, 300][:N]
    batch = run(x, corrupt.records(levels, streams, seed=77))
    for n in reversed(range(N)):
        alone = run(x[n:n + 1], corrupt.records([levels[n]], [streams[n]], seed=77))
        assert np.array_equal(alone[0], batch[n]), n
    other = run(x, corrupt.records(levels, [s + 1 for s in streams], seed=77))
    assert not np.array_equal(other[0], batch[0]) and np.array_equal(other[1], batch[1])      # only the noise knows the stream


@pytest.mark.parametrize("N,res", [(3, 7), (3, 65), (2, 224)])
def test_normalised_output(N, res, cuda):
    x = crops(N, res, 3)
    levels = [(), corrupt.parse_levels("gaussian_blur:1+gamma:0.8")[1], corrupt.parse_levels("jpeg:50")[1]][:N]
    recs = corrupt.records(levels, list(range(N)), seed=1)
    raw, norm = run(x, recs), run(x, recs, normalize=True)
    assert np.array_equal(norm, corrupt_np.normalize_np(raw))             # the same three fp32 operations on the same raw words
    assert np.array_equal(norm[0], corrupt_np.normalize_np(x)[0])         # level 0: the clean crop, normalised as the dataset crop does
    prev = x
    for p in range(recs.shape[1]):
        prev = restate_step(prev, recs[:, p], p)
    dev = float(np.abs(norm.astype(np.float64) - corrupt_np.normalize_np(prev)).max())
    print(f"res {res}: normalised, largest deviation {dev:.3e} (bound {NORM_TOL:.3e})")
    assert dev <= NORM_TOL


def test_bad_records_raise_before_any_gpu_work(cuda):
    x = torch.zeros(1, 3, 8, 8, device=cuda)
    bad = np.zeros((1, 1), ops.CORRUPT_STEP)
    bad[0, 0] = (5, 0, 9.0, 0.0, (0, 0), 0)                               # gamma 9
    with pytest.raises(ops.PocoHipError, match="gamma"):
        ops.corrupt(x, bad)
    with pytest.raises(ops.PocoHipError, match="three buffers"):
        ops.corrupt(x, np.zeros((1, 1), ops.CORRUPT_STEP), out=x)
    with pytest.raises(ops.PocoHipError, match="steps"):
        ops.corrupt(x, np.zeros((2, 1), ops.CORRUPT_STEP))
