"""CPU: the inputs of tests/test_crop_seam_gpu.py do what that test needs of them, shown from the restatements alone: around the
65 535 seam every crop's reference output differs from its neighbours' and from the crops at the start of the batch, for each of the
seven kernel variants; the vectorised records are the records the project's own record builders make."""
import numpy as np
import pytest

from tests import crop_seam_cases as cases


@pytest.mark.parametrize("kind", ["f32", "f64", "multi"])
def test_inference_crops_around_the_seam_differ(kind):
    ref = cases.crop_reference(kind)
    assert ref.shape == (len(cases.REF_ROWS), 3, cases.RES, cases.RES) and ref.dtype == np.float32
    cases.assert_seam_rows_distinct(ref)


def test_float64_boxes_are_not_the_float32_boxes():
    b32, b64 = cases.crop_boxes(np.float32), cases.crop_boxes(np.float64)
    assert (b32[:, 0].astype(np.float64) != b64[:, 0]).mean() > 0.5
    assert not np.array_equal(cases.crop_reference("f32"), cases.crop_reference("multi"))     # the frame index matters


@pytest.mark.parametrize("occ,normalize", [(False, True), (True, False), (True, True)])
def test_dataset_crops_around_the_seam_differ(occ, normalize):
    out, mask, cover = cases.dc_reference(occ, normalize)
    cases.assert_seam_rows_distinct(out)
    if occ:
        assert len({m.tobytes() for m in mask}) > 4 and len(set(cover.tolist())) > 2 and mask.max() == 1 and mask.min() == 0


def test_dataset_records_are_crop_params_records():
    rec = cases.dc_params()                               # asserts equality with datacrop.crop_params at REF_ROWS
    assert len(rec) == cases.N and len({r.tobytes() for r in rec[cases.SEAM_ROWS]}) == len(cases.SEAM_ROWS)
    occ = cases.occ_records()
    assert len({r.tobytes() for r in occ[cases.SEAM_ROWS]}) == len(cases.SEAM_ROWS)
    assert all(occ[n].tobytes() != occ[n - cases.LIMIT].tobytes() for n in range(cases.LIMIT, cases.N))


@pytest.mark.parametrize("normalize", [False, True])
def test_corrupt_crops_around_the_seam_differ(normalize):
    from poco_amd import ops
    rec = cases.corrupt_records()
    assert rec.shape == (cases.N, 2) and (rec["kind"] != 0).all()                      # both chain positions populated
    noise = ops.CORRUPT_KINDS.index("gaussian_noise")
    assert ((rec["kind"] == noise).sum(1) == 1).all()                                  # every crop draws noise once, under its own stream
    assert len(set(rec["stream"][rec["kind"] == noise].tolist())) == cases.N
    assert set(rec["kind"][cases.SEAM_ROWS, 0].tolist()) == set(range(1, 7))           # every kind but jpeg sits on the seam
    cases.assert_seam_rows_distinct(cases.corrupt_reference(normalize))
