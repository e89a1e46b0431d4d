"""GPU: the edges of the inference crop (crop_normalize_kernel, csrc/kernels_misc.hip) and of the dataset crop's tap code, BITWISE
against oracle/crop_np.py and tests/datacrop_np.py, every output inside a poisoned, guard-banded buffer.

  res            1, 5, 27, 28, 29, 57, 224: a block owns CROP_ROWS = 28 rows, so these are one partial block, exactly one, one and a
                 row, two and a row, and the workload's 8 whole blocks; none but 224 lets 256 threads tile a row evenly.
  small frames   (H, W) from 1 x 1 to 4 x 5: the two unaligned 8-byte windows of the fast path need sx <= W - 3 and sy + 1 < H, which
                 W < 3 or H < 2 never allow, W = 3 allows at sx = 0 only, and whose last legal position ends two bytes before the end
                 of the frame.  Integer-aligned scale-1 boxes put output pixels exactly on sx = W - 3, W - 2 and sy = H - 2, H - 1,
                 where fx = fy = 0 switches to the 32767 / 1 weights.  The test derives from the restatement's own coordinates
                 (crop_np.warp_coords) that every branch is taken: it does not trust its boxes.
  clamped index  frame_idx / p.img outside the table read frame 0 or the last frame (include/poco_hip.h) - documented inputs.
  refusals       tester.crop_normalize refuses N = 0, non-contiguous, int32 or CPU boxes and res < 1 before any GPU work.

cv2 is not installed where this suite is developed, so the restatement at res != 224 could not be re-compared with cv2.warpAffine
(tools/validate_assets.py --crop does that where opencv-python imports).  Nothing in oracle/crop_np.py depends on res but the
destination points res / 2 and the extent of the coordinate tables, which are cv2's own for any dsize."""
import ctypes as C

import numpy as np
import pytest
import torch

from oracle import crop_np
from tests import datacrop_np
from tests.crop_seam_cases import Guarded

pytestmark = pytest.mark.gpu
SMALL = [(1, 1), (1, 7), (2, 2), (5, 2), (2, 3), (3, 3), (4, 5)]


def run_crop(frame_d, boxes_np, scale, res, cuda):
    from poco_amd.tester import crop_normalize
    g = Guarded((len(boxes_np), 3, res, res), torch.float32, cuda)
    out = crop_normalize(frame_d, torch.from_numpy(boxes_np).to(cuda), scale, res, out=g.body)
    torch.cuda.synchronize()
    assert out.data_ptr() == g.body.data_ptr()
    g.check(f"res {res}")
    return out.cpu().numpy()


# ---- res -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [1, 5, 27, 28, 29, 57, 224])
def test_crop_normalize_at_other_res(res, cuda):
    r = np.random.default_rng(res)
    frame = r.integers(0, 256, (61, 83, 3), dtype=np.uint8)
    fd = torch.from_numpy(frame).to(cuda)
    boxes = np.array([[41.5, 30.5, 83, 61], [40.3, 29.7, 37.1, 52.9], [3, 4, 30, 22], [80, 58, 25.5, 40], [20, 70, 200, 300]], np.float64)
    for dt in (np.float32, np.float64):
        for scale in (1.0, 1.1):
            b = boxes.astype(dt)
            ref = crop_np.crop_normalize_np(frame, b, scale, res)
            got = run_crop(fd, b, scale, res, cuda)
            bad = np.argwhere(got != ref)
            assert bad.size == 0, (res, dt, scale, len(bad), bad[:4])
            assert len(np.unique(ref)) > 1 or res == 1


# ---- small frames ----------------------------------------------------------------------------------------------------------------
RES_S = 4


def small_frame(H, W):
    return np.random.default_rng(100 * H + W).integers(1, 256, (H, W, 3), dtype=np.uint8)      # no zero byte: a tap outside (0) shows


def offsets(n):
    return sorted({-2, -1, 0, n - 4, n - 3, n - 2, n - 1})


def small_boxes(H, W):
    """(cx, cy, w, h): the whole frame, boxes over each border and corner, and the scale-1 boxes (side = res, centre res / 2 + an
    integer) that map output pixel (x, y) to source pixel (x + ox, y + oy) exactly."""
    b = [[W / 2, H / 2, W, H], [0, 0, W + 1, H + 1], [W, H, W + 1, H + 1], [W / 2, -0.5, W, H + 0.5], [-0.5, H / 2, W + 0.5, H],
         [W + 0.5, H / 2, W, H], [W / 2, H + 0.5, W + 2, H], [W / 2 + 0.3, H / 2 + 0.2, 1.7 * W, 1.3 * H]]
    b += [[RES_S / 2 + ox, RES_S / 2 + oy, RES_S, RES_S] for oy in offsets(H) for ox in offsets(W)]
    return np.array(b, np.float64)


def branch_counts(coords, H, W):
    """Pixels per branch of the tap code, from the restatement's coordinates [(sx, sy, fx, fy)]."""
    n = dict(fast=0, fast_last=0, slow_x1=0, slow_y1=0, slow_inside=0, zero_fast=0, zero_slow=0, on_cols=set(), on_rows=set())
    for sx, sy, fx, fy in coords:
        fast = (sx >= 0) & (sy >= 0) & (sx <= W - 3) & (sy + 1 < H)
        x0ok, x1ok = (sx >= 0) & (sx < W), (sx + 1 >= 0) & (sx + 1 < W)
        y0ok, y1ok = (sy >= 0) & (sy < H), (sy + 1 >= 0) & (sy + 1 < H)
        zero = (fx | fy) == 0
        n["fast"] += int(fast.sum())
        n["fast_last"] += int((fast & (sx == W - 3) & (sy == H - 2)).sum())        # the windows that end 2 bytes before the frame does
        n["slow_x1"] += int((~fast & ~x1ok & x0ok & y0ok).sum())
        n["slow_y1"] += int((~fast & ~y1ok & x0ok & y0ok).sum())
        n["slow_inside"] += int((~fast & x0ok & x1ok & y0ok & y1ok).sum())          # sx = W - 2: all four taps inside, no window
        n["zero_fast"] += int((zero & fast).sum())
        n["zero_slow"] += int((zero & ~fast & x0ok & y0ok).sum())
        inside = x0ok & y0ok & zero
        n["on_cols"] |= set(sx[inside].tolist())
        n["on_rows"] |= set(sy[inside].tolist())
    return n


def assert_branches(n, H, W):
    assert n["slow_x1"] > 0 and n["slow_y1"] > 0 and n["zero_slow"] > 0, (H, W, n)
    assert {W - 1} <= n["on_cols"] and {H - 1} <= n["on_rows"], (H, W, n)            # integer-aligned pixels on the last column and row
    if W >= 2:
        assert W - 2 in n["on_cols"]
    if H >= 2:
        assert H - 2 in n["on_rows"]
    if W >= 3 and H >= 2:
        assert n["fast"] > 0 and n["fast_last"] > 0 and n["zero_fast"] > 0 and n["slow_inside"] > 0 and W - 3 in n["on_cols"], (H, W, n)
    else:
        assert n["fast"] == 0, (H, W, n)                                            # the windows can never be read


@pytest.mark.parametrize("H,W", SMALL)
def test_crop_normalize_on_small_frames(H, W, cuda):
    frame = small_frame(H, W)
    boxes = small_boxes(H, W)
    coords = [crop_np.warp_coords(crop_np.gen_trans_from_patch(*b, RES_S, 1.0), RES_S) for b in boxes.astype(np.float32)]
    assert_branches(branch_counts(coords, H, W), H, W)
    fd = torch.from_numpy(frame).to(cuda)
    for dt in (np.float32, np.float64):
        for scale in (1.0, 1.1):
            b = boxes.astype(dt)
            ref = crop_np.crop_normalize_np(frame, b, scale, RES_S)
            got = run_crop(fd, b, scale, RES_S, cuda)
            bad = np.argwhere(got != ref)
            assert bad.size == 0, (H, W, dt, scale, len(bad), bad[:4], b[bad[0][0]])


def test_dataset_crop_on_small_frames(cuda):
    """The same frames through poco_dataset_crop (plain), all in ONE launch of mixed image sizes, against tests/datacrop_np.py."""
    from poco_amd import datacrop
    frames = [small_frame(H, W) for H, W in SMALL]
    img, centers, bbs, rots, flips = [], [], [], [], []
    for k, (H, W) in enumerate(SMALL):
        coords, first = [], len(img)
        for oy in offsets(H):                              # integer-aligned scale-1 crops: bb = res, centre res / 2 + offset
            for ox in offsets(W):
                img.append(k), centers.append((RES_S // 2 + ox, RES_S // 2 + oy)), bbs.append(RES_S), rots.append(0.0), flips.append((ox + oy) & 1)
        for c, bb, rot in (((W // 2, H // 2), max(H, W), 0.0), ((0, 0), W + H, 30.0), ((W, H), W + H + 1, -45.0), ((W // 2, H), 3, 90.0),
                           ((W, H // 2), 2 * W + 1, 0.0), ((W // 2, H // 2), 1, 0.0)):
            img.append(k), centers.append(c), bbs.append(bb), rots.append(rot), flips.append(len(img) & 1)
        for i in range(first, len(img)):
            M = crop_np.get_affine_transform_cv(*datacrop_np.patch_points(centers[i][0], centers[i][1], bbs[i], RES_S, rots[i]))
            coords.append(crop_np.warp_coords(M, RES_S))
        assert_branches(branch_counts(coords, H, W), H, W)
    n = len(img)
    scales = np.asarray(bbs) / 200.0
    assert all(datacrop_np.py_round(s * 200.0) == bb for s, bb in zip(scales, bbs))
    pns = 1.0 + 0.1 * ((np.arange(n)[:, None] + np.arange(3)) % 5 - 2)
    params = datacrop.batch_params(centers, scales, rots, flips, pns, np.ones(n), RES_S)
    images = [torch.from_numpy(f).to(cuda) for f in frames]
    for normalize in (True, False):
        ref = datacrop_np.dataset_crop_np(frames, img, centers, scales, rots, flips, pns, RES_S, normalize)
        g = Guarded((n, 3, RES_S, RES_S), torch.float32, cuda)
        datacrop.dataset_crop(images, img, params, RES_S, normalize, out=g.body)
        torch.cuda.synchronize()
        g.check("dataset crop")
        got = g.body.cpu().numpy()
        bad = np.argwhere(got != ref)
        assert bad.size == 0, (normalize, len(bad), bad[:4], img[bad[0][0]], centers[bad[0][0]], bbs[bad[0][0]])


# ---- clamped indices ---------------------------------------------------------------------------------------------------------------
def test_frame_index_outside_the_table_reads_the_first_or_last_frame(cuda):
    from poco_amd._lib import check, lib
    r = np.random.default_rng(5)
    H, W, res, nf = 20, 30, 9, 3
    frames = [r.integers(0, 256, (H, W, 3), dtype=np.uint8) for _ in range(nf)]
    fidx = np.array([-7, nf + 3, 1, 0, 2, -2 ** 31, 2 ** 31 - 1, -1, nf], np.int32)
    boxes = np.stack([r.uniform(0, W, len(fidx)), r.uniform(0, H, len(fidx)), r.uniform(8, 40, len(fidx)), r.uniform(8, 40, len(fidx))], 1).astype(np.float32)
    ref = np.concatenate([crop_np.crop_normalize_np(frames[min(max(int(f), 0), nf - 1)], boxes[i:i + 1], 1.0, res) for i, f in enumerate(fidx)])
    assert not np.array_equal(ref[0], crop_np.crop_normalize_np(frames[1], boxes[0:1], 1.0, res)[0])      # the frame matters
    fds = [torch.from_numpy(f).to(cuda) for f in frames]
    ptrs = torch.tensor([f.data_ptr() for f in fds], dtype=torch.int64, device=cuda)
    g = Guarded(ref.shape, torch.float32, cuda)
    fn = lib().poco_crop_normalize_multi
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    fd, bd = torch.from_numpy(fidx).to(cuda), torch.from_numpy(boxes).to(cuda)       # named: they must outlive the launch
    check(fn(ptrs.data_ptr(), nf, fd.data_ptr(), H, W, bd.data_ptr(), len(fidx), 1.0, res, g.body.data_ptr(), None), "poco_crop_normalize_multi")
    torch.cuda.synchronize()
    g.check("multi")
    assert np.array_equal(g.body.cpu().numpy(), ref)


def test_image_index_outside_the_table_reads_the_first_or_last_image(cuda):
    from poco_amd import datacrop
    r = np.random.default_rng(6)
    sizes = [(20, 30), (11, 17), (25, 9)]
    frames = [r.integers(0, 256, hw + (3,), dtype=np.uint8) for hw in sizes]
    idx = np.array([-7, len(frames) + 3, 1, 0, 2, -2 ** 31, 2 ** 31 - 1, 2 ** 40, -1, len(frames)], np.int64)
    n, res = len(idx), 9
    centers = [(int(r.integers(0, 20)), int(r.integers(0, 15))) for _ in range(n)]
    scales, rots, flips, pns = r.uniform(0.05, 0.2, n), r.uniform(-40, 40, n), r.integers(0, 2, n), r.uniform(0.8, 1.2, (n, 3))
    clamped = np.clip(idx, 0, len(frames) - 1)
    ref = datacrop_np.dataset_crop_np(frames, clamped, centers, scales, rots, flips, pns, res, True)
    g = Guarded(ref.shape, torch.float32, cuda)
    datacrop.dataset_crop([torch.from_numpy(f).to(cuda) for f in frames], idx, datacrop.batch_params(centers, scales, rots, flips, pns, np.ones(n), res),
                          res, True, out=g.body)
    torch.cuda.synchronize()
    g.check("dataset crop")
    assert np.array_equal(g.body.cpu().numpy(), ref)


# ---- refusals ------------------------------------------------------------------------------------------------------------------------
def test_crop_normalize_refuses_bad_arguments_before_any_gpu_work(cuda):
    from poco_amd._lib import lib
    from poco_amd.tester import crop_normalize
    frame = torch.from_numpy(np.random.default_rng(9).integers(0, 256, (12, 16, 3), dtype=np.uint8)).to(cuda)
    good = torch.tensor([[8.0, 6.0, 10.0, 10.0], [3.0, 3.0, 5.0, 5.0]], device=cuda)
    g = Guarded((2, 3, 4, 4), torch.float32, cuda)
    wide, tall = torch.zeros(2, 8, device=cuda), torch.zeros(4, 2, device=cuda)
    bad = {"N = 0": (frame, good[:0], 4), "non-contiguous boxes": (frame, wide[:, :4], 4), "transposed boxes": (frame, tall.t(), 4),
           "int32 boxes": (frame, good.to(torch.int32), 4), "float16 boxes": (frame, good.half(), 4), "CPU boxes": (frame, good.cpu(), 4),
           "CPU frame": (frame.cpu(), good, 4), "[N,3] boxes": (frame, good[:, :3].contiguous(), 4), "res 0": (frame, good, 0),
           "res -4": (frame, good, -4), "float frame": (frame.float(), good, 4)}
    assert not wide[:, :4].is_contiguous() and tuple(tall.t().shape) == (2, 4) and not tall.t().is_contiguous()
    for what, (f, b, res) in bad.items():
        with pytest.raises(ValueError, match="crop_normalize"):
            crop_normalize(f, b, 1.0, res, out=g.body)
        with pytest.raises(ValueError, match="crop_normalize"):
            crop_normalize(f, b, 1.0, res)
    with pytest.raises(ValueError, match="out must be"):
        crop_normalize(frame, good, 1.0, 4, out=g.flat[:96].view(2, 3, 4, 4).to(torch.float64))
    with pytest.raises(ValueError, match="out must be"):
        crop_normalize(frame, good, 1.0, 4, out=g.flat[:48].view(1, 3, 4, 4))
    # the C entries refuse res < 1 and null pointers themselves, and take N = 0 as nothing to do
    L = lib()
    for fn in (L.poco_crop_normalize, L.poco_crop_normalize_f64):
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
        assert fn(frame.data_ptr(), 12, 16, good.data_ptr(), 2, 1.0, 0, g.body.data_ptr(), None) != 0
        assert fn(frame.data_ptr(), 12, 16, None, 2, 1.0, 4, g.body.data_ptr(), None) != 0
        assert fn(frame.data_ptr(), 12, 16, good.data_ptr(), -1, 1.0, 4, g.body.data_ptr(), None) != 0
        assert fn(frame.data_ptr(), 12, 16, good.data_ptr(), 0, 1.0, 4, g.body.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert bool((g.bits == g.poison).all()), "a refused call wrote to the output"
    out = crop_normalize(frame, good, 1.0, 4, out=g.body)                  # and the good call goes through
    torch.cuda.synchronize()
    g.check("good call")
    assert np.array_equal(out.cpu().numpy(), crop_np.crop_normalize_np(frame.cpu().numpy(), good.cpu().numpy(), 1.0, 4))
