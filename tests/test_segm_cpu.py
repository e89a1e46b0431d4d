"""CPU: the numpy restatement of the body-part segmentation contract (tests/segm_np.py) reproduces what the reference's own
CrossEntropy and estimate_translation gave (tests/golden/segm.npz, tools/gen_segm_golden.py); face_parts and the bucketize identity
hold for all 24 parts; the mapping loaders; the new entries are declared, exported and refuse bad arguments; the argument checks of
eval.py --segm and demo.py --save_segm."""
import ctypes as C
import importlib.util
import pickle
import zlib
from pathlib import Path

import numpy as np
import pytest
import torch

from poco_amd import _lib, segm
from tests import segm_np

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "segm.npz"
NEW = ["poco_op_part_labels", "poco_op_estimate_translation", "poco_op_segm_score", "poco_op_segm_score_partials", "poco_op_segm_argmax"]
FAKE, NULL = C.c_void_p(4096), C.c_void_p(0)


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def test_restatement_reproduces_the_reference_cross_entropy(gold):
    logits, labels = segm_np.golden_logits()
    assert zlib.crc32(logits.tobytes()) == int(gold["logits_crc"]) and zlib.crc32(labels.tobytes()) == int(gold["labels_crc"])
    ce64, counts, _ = segm_np.segm_score(logits, labels, np.float64)
    mean64 = ce64.sum() / labels.size
    # the reference evaluates in float32 (torch): its distance from the float64 formula is float32 rounding of a mean of 150528 terms
    assert abs(mean64 - float(gold["ce"])) <= 1e-6 * abs(mean64)
    ce32, counts32, _ = segm_np.segm_score(logits, labels, np.float32)
    assert np.array_equal(counts, counts32)                          # no argmax flips between the two precisions on this fixture
    s = segm_np.summarize(ce64, counts, 224 * 224, 25)
    assert s["val_segm_ce"] == pytest.approx(mean64) and 0.3 < s["val_segm_pixel_acc"] < 0.95
    assert np.isnan(s["val_segm_iou"][24]) or s["val_segm_iou"][24] == 0     # class 24 is never the label
    assert counts[:, 3 + 3 * 24].sum() == 0 and counts[:, 2 + 3 * 1].sum() == 0   # ... and class 1 never the prediction
    # the tie at pixel (0, 0): channels 0 and 2 are equal and maximal, the lowest wins
    up = segm_np.upsample(logits, 224, 224, np.float32)
    assert np.all(up[:, 0, 0, 0] == up[:, 2, 0, 0]) and np.all(up[:, :, 0, 0].max(1) == up[:, 0, 0, 0])
    assert np.all(segm_np.segm_score(logits, labels)[2][:, 0, 0] == 0)
    # product code agrees with the restatement's summary
    p = segm.summarize(ce64.sum(), counts.sum(0), labels.size, 25)
    for k in ("val_segm_ce", "val_segm_pixel_acc", "val_segm_miou", "val_segm_miou_fg"):
        assert p[k] == pytest.approx(s[k], rel=1e-12), k
    assert np.array_equal(np.isnan(p["val_segm_iou"]), np.isnan(s["val_segm_iou"]))


def test_upsample_equals_torch_interpolate():
    logits, _ = segm_np.score_fixture(segm_np.SCORE_SHAPES[4])
    want = torch.nn.functional.interpolate(torch.from_numpy(logits).double(), size=(223, 221), mode="bilinear", align_corners=True).numpy()
    assert np.abs(segm_np.upsample(logits, 223, 221, np.float64) - want).max() < 1e-12
    assert np.abs(segm_np.upsample(logits, 223, 221, np.float32) - want).max() < 2e-5
    same, _ = segm_np.score_fixture(segm_np.SCORE_SHAPES[3])
    assert np.array_equal(segm_np.upsample(same, 5, 3, np.float32), same)     # no resampling: the identity, bit for bit


def test_restatement_reproduces_the_reference_translation(gold):
    got = segm_np.estimate_translation(gold["S"], gold["joints2d"])
    S, k = segm_np.translation_fixture()
    assert np.array_equal(S, gold["S"]) and np.array_equal(k, gold["joints2d"])
    assert np.array_equal(got[-1], [1, 1, 1]) and np.array_equal(gold["cam_t"][-1], [1, 1, 1])
    assert np.abs(got[:-1] - gold["cam_t"][:-1]).max() <= 1e-6 * np.abs(gold["cam_t"][:-1]).max()


def test_crop_keypoints_follow_the_reference_transform():
    r = np.random.default_rng(3)
    part = np.concatenate([r.uniform(0, 640, (4, 24, 2)), r.uniform(0, 1, (4, 24, 1))], -1).astype(np.float32)
    center, scale = r.uniform(100, 500, (4, 2)).astype(np.float32), r.uniform(0.5, 2.5, 4).astype(np.float32)
    got = segm.crop_keypoints24(part, center, scale)
    assert got.dtype == np.float32 and np.array_equal(got, segm_np.crop_keypoints24(part, center, scale))
    assert np.array_equal(got[:, :, 2], part[:, :, 2])


def test_face_parts_and_the_bucketize_identity():
    r = np.random.default_rng(0)
    w = r.random((500, 24)).astype(np.float32)
    vp = segm.vertex_parts_from_weights(w)
    assert vp.dtype == np.uint8 and np.array_equal(vp, w.argmax(1)) and set(vp.tolist()) == set(range(24))
    faces = r.integers(0, 500, (900, 3))
    fp = segm.face_parts(vp, faces)
    colors = np.ones((500, 4))
    colors[:, :3] = vp[:, None]
    assert np.array_equal(fp, colors[faces].min(axis=1)[:, 0].astype(np.uint8))   # get_body_part_texture's face colour
    with pytest.raises(ValueError):
        segm.face_parts(vp, [[0, 1, 500]])
    with pytest.raises(ValueError):
        segm.vertex_parts_from_weights(np.zeros((5, 23)))
    # generate_part_labels: texture p / 24 rendered with ambient light 1, * 255, bucketize(right=True) into arange(24) / 24 * 255 + 1,
    # + 1, * mask -> p + 1 on the body and 0 elsewhere, for every part
    bins = (torch.arange(24) / 24.0 * 255.0) + 1
    tex = torch.from_numpy((np.arange(24, dtype=np.float64) / 24.0).astype(np.float32))
    assert torch.equal(torch.bucketize(tex * 255.0, bins, right=True) + 1, torch.arange(24) + 1)
    assert int((torch.bucketize(torch.zeros(1), bins, right=True) + 1) * 0) == 0


def test_mapping_loaders(tmp_path):
    idx = (np.arange(40) % 24).astype(np.int64)
    np.save(tmp_path / "m.npy", idx)
    np.savez(tmp_path / "m.npz", smpl_index=idx.astype(np.float64))
    np.savez(tmp_path / "one.npz", anything=idx)
    with open(tmp_path / "m.pkl", "wb") as f:
        pickle.dump({"smpl_index": idx, "other": 1}, f)
    for n in ("m.npy", "m.npz", "one.npz", "m.pkl"):
        got = segm.load_part_mapping(str(tmp_path / n))
        assert got.dtype == np.uint8 and np.array_equal(got, idx), n
    np.save(tmp_path / "bad.npy", np.array([0, 24]))
    np.save(tmp_path / "frac.npy", np.array([0.5, 1.0]))
    np.savez(tmp_path / "two.npz", a=idx, b=idx)
    with open(tmp_path / "bad.pkl", "wb") as f:
        pickle.dump([1, 2], f)
    for n in ("bad.npy", "frac.npy", "two.npz", "bad.pkl", "missing.npy"):
        with pytest.raises(ValueError):
            segm.load_part_mapping(str(tmp_path / n))
    pal = segm.palette()
    assert pal.shape == (25, 3) and pal.dtype == np.uint8 and not pal[0].any() and len({tuple(c) for c in pal}) == 25
    assert np.array_equal(pal, segm.palette())
    lab = torch.tensor([[0, 3], [24, 1]], dtype=torch.uint8)
    assert np.array_equal(segm.colorize(lab).numpy(), pal[lab.numpy()])


def test_new_entries_are_declared_exported_and_check_their_arguments():
    L = _lib.lib()
    syms = _lib.header_symbols()
    for s in NEW:
        assert s in syms and hasattr(L, s), s
    msg = lambda: L.poco_last_error().decode()   # noqa: E731
    f = C.c_float(5000.0)

    def labels(v=FAKE, B=1, V=10, t=FAKE, fc=FAKE, F=4, fp=FAKE, focal=f, res=224, keys=FAKE, out=FAKE):
        return L.poco_op_part_labels(v, B, V, t, fc, F, fp, focal, res, keys, out, NULL)
    for kw in (dict(v=NULL), dict(t=NULL), dict(fc=NULL), dict(fp=NULL), dict(keys=NULL), dict(out=NULL), dict(B=0), dict(V=0), dict(F=0),
               dict(res=0), dict(res=5000), dict(focal=C.c_float(0.0)), dict(focal=C.c_float(float("nan"))), dict(keys=C.c_void_p(4100))):
        assert labels(**kw) == 1 and "part_labels" in msg(), kw

    def trans(a=FAKE, b=FAKE, B=1, J=24, focal=f, res=224, out=FAKE):
        return L.poco_op_estimate_translation(a, b, B, J, focal, res, out, NULL)
    for kw in (dict(a=NULL), dict(b=NULL), dict(out=NULL), dict(B=0), dict(J=0), dict(J=65), dict(res=0), dict(focal=C.c_float(-1.0))):
        assert trans(**kw) == 1 and "estimate_translation" in msg(), kw

    def score(lg=FAKE, B=1, Cc=25, h=56, w=56, lb=FAKE, H=224, W=224, rec=FAKE, part=FAKE):
        return L.poco_op_segm_score(lg, B, Cc, h, w, lb, H, W, rec, part, NULL)
    for kw in (dict(lg=NULL), dict(lb=NULL), dict(rec=NULL), dict(part=NULL), dict(B=0), dict(Cc=0), dict(Cc=33), dict(h=0), dict(W=0),
               dict(rec=C.c_void_p(4100)), dict(Cc=32, w=200)):
        assert score(**kw) == 1 and "segm_score" in msg(), kw
    assert L.poco_op_segm_argmax(NULL, 1, 25, 56, 56, 224, 224, FAKE, NULL) == 1 and "segm_argmax" in msg()
    assert L.poco_op_segm_argmax(FAKE, 1, 33, 56, 56, 224, 224, FAKE, NULL) == 1
    # blocks per crop: 8 label rows for the 4x upsample, fewer rows when the source is as dense as the labels
    assert L.poco_op_segm_score_partials(56, 224) == 28 and L.poco_op_segm_score_partials(56, 223) == 28
    assert L.poco_op_segm_score_partials(5, 5) == 3 and L.poco_op_segm_score_partials(2, 5) == 1 and L.poco_op_segm_score_partials(56, 2) == 2


def _load(name):
    spec = importlib.util.spec_from_file_location(f"poco_{name}_cli_segm", ROOT / f"{name}.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_entry_point_argument_checks(tmp_path):
    with pytest.raises(ValueError, match="PARE"):
        segm.check_eval_inputs("hrnet_w48_cls-cliff", ["pose", "shape", "part"])
    with pytest.raises(ValueError, match=r"\['shape', 'part'\]"):
        segm.check_eval_inputs("hrnet_w32-pare", ["pose", "imgname"])
    segm.check_eval_inputs("hrnet_w32-pare", ["pose", "shape", "part", "imgname"])
    ev = _load("eval")
    a = ev.parse_args(["--cfg", "c", "--ckpt", "k", "--j_regressor", "j", "--dataset", "d"])
    assert a.segm is False and a.part_mapping is None
    np.savez(tmp_path / "ds.npz", imgname=np.array(["a"]), center=np.zeros((1, 2)), scale=np.ones(1), pose=np.zeros((1, 72)),
             shape=np.zeros((1, 10)))
    a = ev.parse_args(["--cfg", "configs/demo_poco_pare.yaml", "--ckpt", "k", "--j_regressor", "j", "--dataset", str(tmp_path / "ds.npz"),
                       "--segm"])
    with pytest.raises(SystemExit, match="part"):
        ev.check_segm_inputs(a)
    a.cfg = "configs/demo_poco_cliff.yaml"
    with pytest.raises(SystemExit, match="PARE"):
        ev.check_segm_inputs(a)
    a.cfg, a.part_mapping = "configs/demo_poco_pare.yaml", str(tmp_path / "nope.npy")
    np.savez(tmp_path / "ds.npz", imgname=np.array(["a"]), center=np.zeros((1, 2)), scale=np.ones(1), pose=np.zeros((1, 72)),
             shape=np.zeros((1, 10)), part=np.zeros((1, 24, 3)))
    with pytest.raises(SystemExit, match="part mapping not found"):
        ev.check_segm_inputs(a)
    dm = _load("demo")
    base = ["--cfg", "configs/demo_poco_pare.yaml", "--ckpt", "k", "--image_folder", str(tmp_path), "--smpl", str(tmp_path / "smpl.npz")]
    assert dm.parse_args(base).save_segm is False
    np.savez(tmp_path / "smpl.npz", lbs_weights=np.zeros((4, 24), np.float32))
    with pytest.raises(SystemExit, match="faces"):
        dm._check_segm(dm.parse_args(base + ["--save_segm"]))
    with pytest.raises(SystemExit, match="folder"):
        dm._check_segm(dm.parse_args(base + ["--save_segm", "--mode", "video"]))
    with pytest.raises(SystemExit, match="PARE"):
        dm._check_segm(dm.parse_args(["--cfg", "configs/demo_poco_cliff.yaml"] + base[2:] + ["--save_segm"]))
    dm._check_segm(dm.parse_args(base))                                      # without the flag nothing is looked at
