"""GPU: the body-part label rasteriser, the crop camera and the segmentation scorer (csrc/part_labels.hip, csrc/segm_metrics.hip)
against tests/segm_np.py, on the smallest shapes at which they can still go wrong.  Labels, counts and the argmax must equal the
float32 restatement exactly; the cross-entropy is compared per crop with the float64 restatement."""
import functools
from pathlib import Path

import numpy as np
import pytest
import torch

from poco_amd import ops, segm
from tests import render_np, segm_np

pytestmark = pytest.mark.gpu
GOLD = Path(__file__).resolve().parent / "golden" / "segm.npz"
POISON = 0xA5

# Tolerance of the per-crop cross-entropy sum against the float64 restatement.  CE_F32_DEVIATION is the largest relative deviation,
# over every crop of the five SCORE_SHAPES fixtures, of a float32 numpy evaluation of the same formula (per-pixel losses in float32,
# np.sum in float32: segm_np.segm_score(..., np.float32)) from the float64 one: 1.455e-07, reached by crop 1 of the [3,25,56,56] case
# (the others lie between 1.9e-09 and 1.41e-07).  The device may differ from float64 by 8 times that: the factor covers its expf / logf
# and its summation tree (it sums the float32 losses in fp64, so it usually stays well inside).  DESIGN.md section 21 has the same numbers.
CE_F32_DEVIATION = 1.455e-07
CE_REL_TOL = 8 * CE_F32_DEVIATION


# ---- rasteriser ----------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _mesh_case(kind: str, res: int):
    """(verts [3,V,3], cam_t [3,3], faces, face_part, focal, expected labels [3,res,res]) - the restatement is computed once."""
    far = 224.0 / res
    if kind == "sphere":
        vs = [render_np.deformed_sphere(seed)[0] for seed in (0, 1, 2)]
        faces = render_np.deformed_sphere(0)[1]
        verts = np.stack(vs)
        focal = 5000.0
        cam_t = np.array([[0.02, -0.03, 33.0 * far], [0.31, 0.1, 41.5 * far], [-0.05, 0.42, 27.25 * far]], np.float32)   # two reach over the border
        part = (np.arange(len(faces)) * 7 % 24).astype(np.uint8)
    else:
        v, faces, part = segm_np.hand_mesh()
        verts = np.stack([v, v, v])
        focal = 4096.0
        # crop 0 of res 224 sees the mesh exactly as it was laid out in screen space; the others from generic positions
        cam_t = np.array([[0.0, 0.0, 64.0 * (far - 1)], [0.013, -0.021, 3.7 + 64.0 * (far - 1)], [-0.4, 0.25, -9.3 + 64.0 * (far - 1)]], np.float32)
    want = segm_np.part_labels(verts, cam_t, faces, part, focal, res)
    return verts.astype(np.float32), cam_t, faces, part, focal, want


def test_hand_mesh_puts_centres_on_edges_and_vertices():
    """The fixture does what it says (CPU arithmetic only): crop 0 projects the fan's hub onto the pixel centre (40.5, 40.5) and its
    spokes through pixel centres, bit for bit; the coplanar pair ties exactly and the lower face wins; the faces that must cover
    nothing cover nothing; the back-facing triangle is filled."""
    verts, cam_t, faces, part, focal, want = _mesh_case("hand", 224)
    x, y, z = segm_np.project(verts[0], cam_t[0], focal, 224)
    assert (x[0], y[0]) == (40.5, 40.5) and (x[1], y[1]) == (56.5, 40.5) and (x[2], y[2]) == (56.5, 56.5)
    lab = want[0]
    # a centre exactly on a vertex and on shared edges gets exactly one owner: every pixel of the fan's square is a fan part
    assert np.all((lab[25:56, 25:56] >= 1) & (lab[25:56, 25:56] <= 8))
    keys = segm_np.part_keys(verts[0], cam_t[0], faces, focal, 224)
    f32_, f33 = 32, 33
    both = (keys & np.uint64(0xFFFFFFFF)) == np.uint64(f32_)
    assert both.any() and part[f32_] != part[f33]
    solo33 = segm_np.part_keys(verts[0], cam_t[0], faces[[f33]], focal, 224) != segm_np.EMPTY
    solo32 = segm_np.part_keys(verts[0], cam_t[0], faces[[f32_]], focal, 224) != segm_np.EMPTY
    overlap = solo32 & solo33
    assert overlap.sum() > 100 and np.all(lab[overlap] == part[f32_] + 1)          # equal depth: the lower face index wins
    assert np.any(lab[solo33 & ~solo32] == part[f33] + 1)
    assert (lab == part[34] + 1).sum() > 300                                        # the back-facing triangle is filled
    for f in (36, 37):                                                              # behind Z = 0.1; a NaN vertex
        assert not (segm_np.part_keys(verts[0], cam_t[0], faces[[f]], focal, 224) != segm_np.EMPTY).any()
    assert (lab[:, 0] == part[35] + 1).any() and (lab[-1] == part[35] + 1).any()    # the straddling triangle reaches two borders


@pytest.mark.parametrize("res", [224, 17])
@pytest.mark.parametrize("kind", ["sphere", "hand"])
def test_part_labels_equal_the_restatement_bit_for_bit(cuda, kind, res):
    verts, cam_t, faces, part, focal, want = _mesh_case(kind, res)
    assert len(np.unique(want)) > (3 if res == 17 else 10) and (kind == "hand" or (want == 0).any())
    dev = torch.device("cuda")
    mesh = segm.PartMesh(faces, part, dev)
    got = segm.part_labels(verts, cam_t, mesh, focal, res).cpu().numpy()
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{len(bad)} pixels differ, first {bad[:5].tolist()}: got {got[tuple(bad[0])]}, want {want[tuple(bad[0])]}"
    # every crop but the last into a poisoned buffer: the last crop's slot and the guard bytes stay as they were
    n, g = res * res, 4096
    buf = torch.full((g + 3 * n + g,), POISON, dtype=torch.uint8, device=dev)
    out = buf[g:g + 2 * n].view(2, res, res)
    segm.part_labels(verts[:2], cam_t[:2], mesh, focal, res, out=out)
    host = buf.cpu().numpy()
    assert np.array_equal(host[g:g + 2 * n].reshape(2, res, res), want[:2])
    assert np.all(host[:g] == POISON) and np.all(host[g + 2 * n:] == POISON)


def test_projection_agrees_with_perspective_projection(cuda):
    """A one-pixel triangle centred on a 3-D point lands on the pixel where perspective_projection (geometry.py:480-508: K [f, f, res / 2],
    identity rotation) puts that point - the convention smpl_joints2d uses, y down."""
    res, focal = 224, 5000.0
    r = np.random.default_rng(4)
    B = 3
    pts = np.stack([r.uniform(-0.6, 0.6, B), r.uniform(-0.6, 0.6, B), r.uniform(-0.2, 0.2, B)], -1)
    cam_t = np.stack([r.uniform(-0.1, 0.1, B), r.uniform(-0.1, 0.1, B), r.uniform(30, 40, B)], -1)
    P = pts + cam_t
    xy = focal * P[:, :2] / P[:, 2:] + res / 2.0                      # perspective_projection in float64
    col, row = np.floor(xy[:, 0]).astype(int), np.floor(xy[:, 1]).astype(int)
    assert np.all((col >= 0) & (col < res) & (row >= 0) & (row < res))
    # centre the triangle on the centre of that pixel, 0.45 pixels to each corner, at the point's depth
    px = (np.stack([col, row], -1) + 0.5 - res / 2.0) * P[:, 2:] / focal - cam_t[:, :2]
    d = 0.45 * P[:, 2] / focal
    verts = np.zeros((B, 3, 3), np.float32)
    for k, (dx, dy) in enumerate([(-1, -1), (1, -1), (0, 1)]):
        verts[:, k, 0], verts[:, k, 1], verts[:, k, 2] = px[:, 0] + dx * d, px[:, 1] + dy * d, pts[:, 2]
    mesh = segm.PartMesh([[0, 1, 2]], [6], "cuda")
    lab = segm.part_labels(verts, cam_t.astype(np.float32), mesh, focal, res).cpu().numpy()
    for b in range(B):
        assert np.argwhere(lab[b] != 0).tolist() == [[row[b], col[b]]] and lab[b, row[b], col[b]] == 7, b


# ---- scorer --------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _score_case(shape):
    logits, labels = segm_np.score_fixture(shape)
    ce64, _, _ = segm_np.segm_score(logits, labels, np.float64)
    _, counts32, arg32 = segm_np.segm_score(logits, labels, np.float32)
    return logits, labels, ce64, counts32, arg32


@pytest.mark.parametrize("shape", segm_np.SCORE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_segm_score_counts_exact_ce_within_tolerance_and_reproducible(cuda, shape):
    B, C, h, w, H, W = shape
    logits, labels, ce64, counts, arg = _score_case(shape)
    if C > 2:
        assert counts[:, 3 + 3 * (C - 1)].sum() == 0 and counts[:, 2 + 3 * 1].sum() == 0      # a class never present, one never predicted
        assert counts[:, 3 + 3 * 1].sum() > 0 and np.all(arg[:, 0, 0] == 0)                  # ... that is present; the tie goes to channel 0
    dl, db = torch.from_numpy(logits).cuda(), torch.from_numpy(labels).cuda()
    words = ops.segm_record_words(C)
    # records of the B crops inside a larger, poisoned block: the rows around them stay as they were
    block = torch.full((B + 2, words), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda")
    rec = ops.segm_score(dl, db, out=block[1:1 + B])
    again = ops.segm_score(dl, db)
    host = block.cpu()
    assert torch.equal(host[1:1 + B], again.cpu())                                   # the same bits on every run, CE included
    assert bool((host[0] == 0x5A5A5A5A5A5A5A5A).all()) and bool((host[-1] == 0x5A5A5A5A5A5A5A5A).all())
    got_counts = rec[:, 1:].cpu().numpy()
    assert np.array_equal(got_counts, counts), np.argwhere(got_counts != counts)[:5]
    got_ce = rec[:, 0].contiguous().view(torch.float64).cpu().numpy()
    dev = np.abs(got_ce - ce64) / np.abs(ce64)
    print(f"CE per crop, relative deviation from float64: {dev} (tolerance {CE_REL_TOL:.3e})")
    assert np.all(dev <= CE_REL_TOL), (got_ce, ce64)
    assert np.array_equal(ops.segm_argmax(dl, H, W).cpu().numpy(), arg)


def test_accumulator_summary(cuda):
    shape = segm_np.SCORE_SHAPES[1]
    logits, labels, ce64, counts, _ = _score_case(shape)
    acc = segm.SegmAccumulator(capacity=3)
    dl, db = torch.from_numpy(logits).cuda(), torch.from_numpy(labels).cuda()
    acc.step(dl[:2], db[:2])
    acc.step(dl[2:], db[2:])
    with pytest.raises(Exception, match="capacity"):
        acc.step(dl[:1], db[:1])
    got = acc.finish(return_records=True)
    want = segm_np.summarize(ce64, counts, 224 * 224, 25)
    assert got["val_segm_ce"] == pytest.approx(want["val_segm_ce"], rel=CE_REL_TOL)
    gold = float(np.load(GOLD)["ce"])                                                 # the reference's own CrossEntropy, float32
    assert got["val_segm_ce"] == pytest.approx(gold, rel=1e-6)
    assert got["val_segm_pixel_acc"] == want["val_segm_pixel_acc"] and got["val_segm_miou"] == pytest.approx(want["val_segm_miou"], rel=1e-12)
    assert np.array_equal(got["val_segm_iou"], want["val_segm_iou"], equal_nan=True)
    assert got["val_segm_iou"][1] == 0 and got["val_segm_iou"][24] == 0              # present but never predicted; predicted but never present
    assert got["val_segm_miou_fg"] == pytest.approx(want["val_segm_miou_fg"], rel=1e-12) and got["segm_N"] == 3
    assert np.array_equal(got["segm_counts"], counts)
    acc.reset()
    acc.step(dl[:1], db[:1])
    assert acc.finish()["segm_N"] == 1


# ---- camera --------------------------------------------------------------------------------------------------------------------------
def test_estimate_translation_matches_the_reference(cuda):
    g = np.load(GOLD)
    got = segm.estimate_translation(torch.from_numpy(g["S"]).cuda(), torch.from_numpy(g["joints2d"]).cuda()).cpu().numpy()
    want = g["cam_t"]
    assert got.dtype == np.float32 and np.array_equal(got[-1], [1, 1, 1])            # the singular row
    rel = np.abs(got[:-1].astype(np.float64) - want[:-1]) / np.abs(want[:-1])
    print(f"cam_t relative deviation from the reference: {rel.max():.3e}")
    assert rel.max() <= 1e-5
    f64 = segm_np.estimate_translation(g["S"], g["joints2d"])
    assert np.abs(got[:-1] - f64[:-1]).max() <= 1e-5 * np.abs(f64[:-1]).max()
