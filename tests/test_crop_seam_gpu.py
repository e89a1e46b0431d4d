"""GPU: the second launch of a chunked batch.  Five host loops split a batch at the gridDim.y / z limit of 65 535 and advance every
per-crop pointer for the second launch: launch_crop_t (float32 and float64 boxes), launch_crop_normalize_multi, poco_dataset_crop,
crop_occ_entry (with and without the mask) and poco_op_corrupt.  Each is run here on N = 65 535 + 5 crops at res = 4 (12.6 MB of
output), with the inputs of tests/crop_seam_cases.py, and

  1. the one-call result is BITWISE the concatenation of two calls on [0, 40 000) and [40 000, N), each below the limit - the whole
     array, and mask and cover where there are any;
  2. rows 0..4 and 65 531..65 539 (the last two of the batch among them) are BITWISE the numpy restatement;
  3. a guard band of poison around out (mask, cover, and corrupt's second buffer) is intact and every element inside was written.

tests/test_crop_seam_cpu.py holds, from the restatements alone, that the crops around the seam differ from one another and from crops
0..4, so a pointer that is not advanced, advanced by the wrong stride, or wrapped to the start cannot pass 2.

The dataset crop runs with groups = 1: a second group of 32 x 32 pixels needs res >= 33, which is 856 MB of output at this N, so the
`groups * groups` stride of `cover` is 1 here (its own offset `+ n0` is still exercised, with a 4-byte stride no other array has).

corrupt: pixelate, contrast and the motion blur are IEEE operations in a fixed order on both sides; gamma, the Gaussian blur and the
noise go through libm (pow, exp, log, sin, cos), whose last fp64 place may differ between the device and numpy.  Such a difference
reaches the fp32 store only if the fp64 value lies within an ulp of an fp32 rounding boundary, about 2^-28 per element; 14 rows of 48
elements and two steps are compared, and the inputs are fixed, so the rows are compared bitwise like everything else here."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import crop_seam_cases as cases
from tests.crop_seam_cases import N, REF_ROWS, RES, SPLIT, Guarded

pytestmark = pytest.mark.gpu
PARTS = ((0, SPLIT), (SPLIT, N))


def rows_of(t):
    return t[torch.from_numpy(REF_ROWS).to(t.device)].cpu().numpy()


def same(a, b, what):
    """bitwise on the device (the words, so that a NaN would count too)"""
    assert a.shape == b.shape and a.dtype == b.dtype
    va, vb = (a.view(torch.int32), b.view(torch.int32)) if a.dtype == torch.float32 else (a, b)
    assert torch.equal(va, vb), f"{what}: {int((va != vb).sum())} words differ, first crop {int((va != vb).reshape(len(a), -1).any(1).nonzero()[0])}"


# ---- launch_crop_t -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["f32", "f64"])
def test_crop_normalize_across_the_seam(kind, cuda):
    from poco_amd.tester import crop_normalize
    ref = cases.crop_reference(kind)
    cases.assert_seam_rows_distinct(ref)
    frame = torch.from_numpy(cases.crop_frames()[0]).to(cuda)
    boxes = torch.from_numpy(cases.crop_boxes(np.float64 if kind == "f64" else np.float32)).to(cuda)
    one, two = Guarded((N, 3, RES, RES), torch.float32, cuda), Guarded((N, 3, RES, RES), torch.float32, cuda)
    crop_normalize(frame, boxes, 1.1, RES, out=one.body)
    for lo, hi in PARTS:
        crop_normalize(frame, boxes[lo:hi], 1.1, RES, out=two.body[lo:hi])
    torch.cuda.synchronize()
    one.check("one call"), two.check("two calls")
    same(one.body, two.body, kind)
    assert np.array_equal(rows_of(one.body), ref)


# ---- launch_crop_normalize_multi -----------------------------------------------------------------------------------------------
def test_crop_normalize_multi_across_the_seam(cuda):
    from poco_amd._lib import check, lib
    ref = cases.crop_reference("multi")
    cases.assert_seam_rows_distinct(ref)
    frames = [torch.from_numpy(f).to(cuda) for f in cases.crop_frames()]
    ptrs = torch.tensor([f.data_ptr() for f in frames], dtype=torch.int64, device=cuda)
    boxes = torch.from_numpy(cases.crop_boxes(np.float32)).to(cuda)
    fidx = torch.from_numpy(cases.frame_index()).to(cuda)
    H, W = cases.CROP_HW
    fn = lib().poco_crop_normalize_multi
    fn.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    one, two = Guarded((N, 3, RES, RES), torch.float32, cuda), Guarded((N, 3, RES, RES), torch.float32, cuda)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    check(fn(ptrs.data_ptr(), len(frames), fidx.data_ptr(), H, W, boxes.data_ptr(), N, 1.1, RES, one.body.data_ptr(), stream), "multi")
    for lo, hi in PARTS:
        check(fn(ptrs.data_ptr(), len(frames), fidx[lo:hi].data_ptr(), H, W, boxes[lo:hi].data_ptr(), hi - lo, 1.1, RES,
                 two.body[lo:hi].data_ptr(), stream), "multi")
    torch.cuda.synchronize()
    one.check("one call"), two.check("two calls")
    same(one.body, two.body, "multi")
    assert np.array_equal(rows_of(one.body), ref)


# ---- poco_dataset_crop and crop_occ_entry --------------------------------------------------------------------------------------
def dataset_crop_call(mode, images, params, occ, atlas, normalize, out, cover, mask):
    """poco_dataset_crop (mode 'plain'), poco_dataset_crop_occ ('occ') or poco_dataset_crop_occ_mask ('mask') on the records given,
    into the caller's out / cover / mask tensors: the upload of datacrop.dataset_crop, with the outputs in the test's hands."""
    from poco_amd import datacrop
    from poco_amd._lib import check
    dev = images[0].device
    n, n_img = len(params), len(images)
    params = np.ascontiguousarray(params)
    host = np.zeros(16 * n_img + 48 * n + (144 * n if occ is not None else 0), np.uint8)
    host[:8 * n_img].view(np.int64)[:] = [im.data_ptr() for im in images]
    host[8 * n_img:16 * n_img].view(np.int32)[:] = [v for im in images for v in (im.shape[0], im.shape[1])]
    host[16 * n_img:16 * n_img + 48 * n] = params.view(np.uint8)
    if occ is not None:
        occ = np.ascontiguousarray(occ)
        host[16 * n_img + 48 * n:] = occ.view(np.uint8)
    d = torch.from_numpy(host).to(dev)
    base = d.data_ptr()
    stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    head = [C.c_void_p(base), C.c_void_p(base + 8 * n_img), n_img, C.c_void_p(base + 16 * n_img), C.c_void_p(params.ctypes.data), n, RES,
            int(normalize)]
    if mode == "plain":
        check(datacrop._bind().poco_dataset_crop(*head, C.c_void_p(out.data_ptr()), stream), "poco_dataset_crop")
        return d
    mid = [C.c_void_p(atlas.d_atlas.data_ptr()), atlas.texels, C.c_void_p(atlas.d_table.data_ptr()), C.c_void_p(atlas.table.ctypes.data),
           len(atlas.table), C.c_void_p(base + 16 * n_img + 48 * n), C.c_void_p(occ.ctypes.data), C.c_void_p(out.data_ptr()),
           C.c_void_p(cover.data_ptr())]
    if mode == "occ":
        check(datacrop._bind_occ().poco_dataset_crop_occ(*head, *mid, stream), "poco_dataset_crop_occ")
    else:
        check(datacrop._bind_occ().poco_dataset_crop_occ_mask(*head, *mid, C.c_void_p(mask.data_ptr()), stream), "poco_dataset_crop_occ_mask")
    return d                                              # the upload stays alive until the caller has synchronised


@pytest.mark.parametrize("mode,normalize", [("plain", True), ("occ", False), ("mask", True)])
def test_dataset_crop_across_the_seam(mode, normalize, cuda):
    from poco_amd import datacrop
    occ = mode != "plain"
    ref_out, ref_mask, ref_cover = cases.dc_reference(occ, normalize)
    cases.assert_seam_rows_distinct(ref_out)
    images = [torch.from_numpy(a).to(cuda) for a in cases.dc_images()]
    params = cases.dc_params()
    recs = cases.occ_records() if occ else None
    atlas = datacrop.OccluderAtlas(cases.occluders(), cuda) if occ else None

    def buffers():
        return (Guarded((N, 3, RES, RES), torch.float32, cuda), Guarded((N, 1), torch.int32, cuda) if occ else None,
                Guarded((N, RES, RES), torch.uint8, cuda) if mode == "mask" else None)
    one, two = buffers(), buffers()
    body = lambda g, lo, hi: None if g is None else g.body[lo:hi]          # noqa: E731
    keep = [dataset_crop_call(mode, images, params, recs, atlas, normalize, *(body(g, 0, N) for g in one))]
    for lo, hi in PARTS:
        keep.append(dataset_crop_call(mode, images, params[lo:hi], recs[lo:hi] if occ else None, atlas, normalize, *(body(g, lo, hi) for g in two)))
    torch.cuda.synchronize()
    for name, a, b in zip(("out", "cover", "mask"), one, two):
        if a is not None:
            a.check(f"{name}, one call"), b.check(f"{name}, two calls")
            same(a.body, b.body, f"{mode} {name}")
    assert np.array_equal(rows_of(one[0].body), ref_out)
    if occ:
        assert np.array_equal(rows_of(one[1].body)[:, 0], ref_cover)
    if mode == "mask":
        assert np.array_equal(rows_of(one[2].body), ref_mask)


# ---- poco_op_corrupt -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("normalize", [False, True])
def test_corrupt_across_the_seam(normalize, cuda):
    from poco_amd import ops
    ref = cases.corrupt_reference(normalize)
    cases.assert_seam_rows_distinct(ref)
    x_np, recs = cases.corrupt_input(), cases.corrupt_records()
    x = torch.from_numpy(x_np).to(cuda)
    shape = (N, 3, RES, RES)
    one, one_tmp, two, two_tmp = (Guarded(shape, torch.float32, cuda) for _ in range(4))
    ops.corrupt(x, recs, normalize, out=one.body, tmp=one_tmp.body)
    for lo, hi in PARTS:
        ops.corrupt(x[lo:hi], recs[lo:hi], normalize, out=two.body[lo:hi], tmp=two_tmp.body[lo:hi])
    torch.cuda.synchronize()
    for g, what in ((one, "out, one call"), (one_tmp, "tmp, one call"), (two, "out, two calls"), (two_tmp, "tmp, two calls")):
        g.check(what)                                     # two chain positions: the first launch writes tmp, the second out
    same(one.body, two.body, "corrupt out")
    same(one_tmp.body, two_tmp.body, "corrupt tmp")
    assert torch.equal(x.cpu(), torch.from_numpy(x_np)), "the input was written"
    assert np.array_equal(rows_of(one.body), ref)
