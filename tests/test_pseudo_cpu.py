"""CPU: the pseudo-labeler's contract - tests/pseudo_np.py against the reference-made fixture tests/golden/pseudo.npz
(tools/gen_pseudo_golden.py), the selection against get_confident_frames' own indices, the dataset file's format, the C ABI's
declarations and argument checks (no GPU: poco_pseudo_create is host only and every argument error is raised before any GPU work)
and the refusals of the demo.py / eval.py flags."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from poco_amd import _lib, evaluate, postproc, pseudo
from tests import pseudo_np

ROOT = Path(__file__).resolve().parent.parent
GOLD = ROOT / "tests" / "golden" / "pseudo.npz"
SYMBOLS = ["poco_op_rotmat_to_aa", "poco_pseudo_create", "poco_pseudo_step", "poco_pseudo_finish", "poco_pseudo_reset",
           "poco_pseudo_destroy"]
ERR_ARG = 1


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


def test_fixture_is_data_only_and_covers_every_class(gold):
    assert all(v.dtype.kind in "fi" for v in gold.values())
    assert GOLD.stat().st_size < 1 << 20
    R, cls = pseudo_np.fixture_matrices()
    assert np.array_equal(R.view(np.uint32), gold["rotmat"].view(np.uint32)) and np.array_equal(cls, gold["cls"])
    assert sorted(set(cls.tolist())) == list(range(len(pseudo_np.CLASSES))) and len(R) >= 257
    branch = pseudo_np.quaternion_branch(R)
    assert sorted(set(branch.tolist())) == [0, 1, 2, 3]
    assert sorted(branch[cls == pseudo_np.CLASSES.index("branch")].tolist()) == [0, 1, 2, 3]
    assert np.array_equal(pseudo_np.fixture_var().view(np.uint32), gold["var"].view(np.uint32))
    assert 0 < gold["d_ref_aa"] < 1e-5 and 0 < gold["d_ref_roundtrip"] < 1e-5


@pytest.mark.parametrize("dtype,factor", [(np.float64, 1.0), (np.float32, 8.0)])
def test_pseudo_np_reproduces_golden(gold, dtype, factor):
    """float64: within d_ref (true by construction for a fresh fixture: pins the restatement to the file); float32: within
    8 x d_ref, the margin the GPU test uses."""
    aa = pseudo_np.rotmat_to_aa(gold["rotmat"], dtype)
    err = np.abs(aa.astype(np.float64) - gold["aa"]).max()
    print(f"{dtype.__name__} axis-angle: {err:.3e} (d_ref {gold['d_ref_aa']:.3e})")
    assert aa.dtype == np.float32 and err <= factor * gold["d_ref_aa"]
    cls = gold["cls"]
    ok = ~np.isin(cls, [pseudo_np.CLASSES.index(c) for c in ("zero", "nan")])
    rt = pseudo_np.rodrigues(aa[ok], dtype).astype(np.float64) - gold["rotmat"][ok]
    err = np.abs(rt - (gold["rod_of_aa"][ok].astype(np.float64) - gold["rotmat"][ok])).max()
    print(f"{dtype.__name__} round trip: {err:.3e} (d_ref {gold['d_ref_roundtrip']:.3e})")
    assert err <= factor * gold["d_ref_roundtrip"]
    # the special rows: a NaN gives zeros, the zero matrix (0, pi, 0), the identity zeros, pi about a coordinate axis pi on it
    row = lambda c: aa[cls == pseudo_np.CLASSES.index(c)]          # noqa: E731
    assert np.array_equal(row("nan"), np.zeros((1, 3), np.float32)) and np.array_equal(row("identity"), np.zeros((1, 3), np.float32))
    assert np.array_equal(row("zero"), np.array([[0, np.pi, 0]], np.float32))
    assert np.array_equal(row("pi_coordinate"), np.float32(np.pi) * np.eye(3, dtype=np.float32))
    assert np.allclose(np.linalg.norm(row("pi").astype(np.float64), axis=1), np.pi, atol=1e-5)


def test_selection_equals_get_confident_frames(gold):
    var, thr = gold["var"], float(gold["threshold"])
    assert np.isnan(var[5, 0]) and var[9, 0] == np.float32(thr)
    for fn in (pseudo_np.confident_frames, postproc.confident_frames):
        idx = fn(var.copy(), thr)
        assert np.array_equal(idx, gold["confident_idx"]), fn
        assert 5 not in idx and 9 not in idx                     # a NaN compares false; the comparison is <
    assert 0 < len(gold["confident_idx"]) < len(var)
    kin = pseudo_np.kinematic(var)
    assert np.array_equal(kin.view(np.uint32), gold["var_kinematic"].view(np.uint32))
    assert np.array_equal(postproc.kinematic_uncert(var).view(np.uint32), gold["var_kinematic"].view(np.uint32))
    # the step's flags are that selection; without a threshold (None, NaN, <= 0) every crop is kept
    x = pseudo_np.step_inputs(len(var))
    x["var_pose"] = var
    rec, keep = pseudo_np.step(**x, threshold=thr)
    assert np.array_equal(np.nonzero(keep)[0], gold["confident_idx"]) and len(rec) == len(gold["confident_idx"])
    assert np.array_equal(pseudo_np.split(rec)["source_id"], x["source_id"][keep])            # stable: source order
    for none in (None, float("nan"), 0.0, -1.0):
        assert pseudo_np.step(**x, threshold=none)[1].all()


def test_record_layout_matches_header_and_binding():
    txt = _lib.HEADER.read_text()
    assert f"#define POCO_PSEUDO_RECORD_FLOATS {pseudo_np.RECORD_FLOATS}" in txt and pseudo.RECORD_FLOATS == pseudo_np.RECORD_FLOATS
    assert f"#define POCO_PSEUDO_MAX_TRAILING {pseudo.MAX_TRAILING}" in txt and "#define POCO_PSEUDO_UNWRITTEN 0xFFFFFFFFu" in txt
    names = ("P_SRC", "P_CENTER", "P_SCALE", "P_POSE", "P_SHAPE", "P_VAR", "P_OPENPOSE", "P_PART", "P_S", "P_PAD")
    assert [getattr(pseudo, n) for n in names] == [getattr(pseudo_np, n) for n in names] == [0, 1, 3, 4, 76, 86, 110, 185, 257, 353]
    x = pseudo_np.step_inputs(5, seed=3)
    rec, _ = pseudo_np.step(**x, joints_in_crop=True)
    a, b = pseudo.split_records(rec), pseudo_np.split(rec)
    assert all(np.array_equal(a[k].view(np.uint32) if a[k].dtype == np.float32 else a[k], b[k].view(np.uint32) if b[k].dtype == np.float32 else b[k])
               for k in b)
    assert np.all(rec[:, pseudo_np.P_PAD:] == 0) and np.array_equal(a["source_id"], x["source_id"])
    # crop coordinates -> image coordinates: the host formula, bit for bit
    ref = postproc.convert_crop_coords_to_orig_img(x["boxes"], x["joints2d"].copy(), 224)
    assert np.array_equal(np.concatenate([a["openpose"], a["part"]], 1)[:, :, :2].view(np.uint32), ref.astype(np.float32).view(np.uint32))
    assert np.array_equal(a["scale"], np.maximum(x["boxes"][:, 2], x["boxes"][:, 3]) / 200.0)


def test_write_dataset_round_trip(tmp_path):
    x = pseudo_np.step_inputs(7, seed=5)
    rec, _ = pseudo_np.step(**x)
    arrays = pseudo.split_records(rec)
    arrays["imgname"] = np.asarray([f"im{i}.png" for i in range(7)])
    arrays["person_id"] = np.arange(7)
    path = tmp_path / "sub" / "pseudo.npz"
    assert pseudo.write_dataset(str(path), arrays) == 7
    z = np.load(path, allow_pickle=False)
    assert sorted(z.files) == sorted(pseudo.DATASET_KEYS)
    want = {"imgname": (7,), "center": (7, 2), "scale": (7,), "pose": (7, 72), "shape": (7, 10), "var": (7, 24), "has_smpl": (7,),
            "part": (7, 24, 3), "openpose": (7, 25, 3), "S": (7, 24, 4), "person_id": (7,)}
    for k, shp in want.items():
        assert z[k].shape == shp, (k, z[k].shape)               # every array has N as its leading dimension
    assert z["person_id"].dtype == np.int32 and z["imgname"].dtype.kind == "U" and np.all(z["has_smpl"] == 1)
    assert evaluate.check_dataset_keys(z.files) == "smpl"
    (tmp_path / "imgs").mkdir()
    ds = evaluate.EvalDataset(str(path), str(tmp_path / "imgs"))
    assert len(ds) == 7 and ds.gt_form == "smpl" and np.array_equal(ds.pose, arrays["pose"]) and np.array_equal(ds.shape, arrays["shape"])
    assert ds.imgname[3] == "im3.png" and np.array_equal(ds.person_id, np.arange(7))
    # the reader's selection, on the file: the rows of get_confident_frames, in order; every array is cut
    thr = float(np.median(arrays["var"][:, 0]))
    sel = evaluate.EvalDataset(str(path), str(tmp_path / "imgs"), uncert_threshold=thr)
    idx = pseudo_np.confident_frames(arrays["var"], thr)
    assert 0 < len(idx) < 7 and len(sel) == len(idx) and sel.total == 7
    assert np.array_equal(sel.pose, arrays["pose"][idx]) and sel.imgname == [f"im{i}.png" for i in idx]
    # a scalar or a short array is refused: the reference's reader indexes every array with the selected rows
    for bad in ({**arrays, "scale": arrays["scale"][:3]}, {**arrays, "scale": np.float32(1.0)}, {k: v for k, v in arrays.items() if k != "var"}):
        with pytest.raises(ValueError):
            pseudo.write_dataset(str(tmp_path / "bad.npz"), bad)


def test_demo_argument_refusals(tmp_path, capsys):
    import demo
    base = ["--cfg", "configs/demo_poco_cliff.yaml", "--ckpt", "none.pt", "--image_folder", str(tmp_path)]
    with pytest.raises(SystemExit) as e:
        demo.main(demo.parse_args(base + ["--uncert_threshold", "0.3"]))
    assert "--save_dataset" in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        demo.main(demo.parse_args(base + ["--mode", "video", "--vid_file", str(tmp_path), "--gpus", "2", "--save_dataset", str(tmp_path / "d.npz")]))
    assert "--gpus" in str(e.value.code) and "gather" in str(e.value.code)
    args = demo.parse_args(base)
    assert args.save_dataset is None and args.uncert_threshold is None            # nothing changes without the flag


def test_eval_argument_refusals(tmp_path):
    import eval as eval_cli
    x = pseudo_np.step_inputs(6, seed=9)
    rec, _ = pseudo_np.step(**x)
    arrays = pseudo.split_records(rec)
    arrays["imgname"] = np.asarray([f"im{i}.png" for i in range(6)])
    arrays["person_id"] = np.zeros(6, np.int32)
    pseudo.write_dataset(str(tmp_path / "with_var.npz"), arrays)
    np.savez(tmp_path / "no_var.npz", **{k: v for k, v in arrays.items() if k not in ("var", "source_id")})
    base = ["--cfg", "configs/demo_poco_cliff.yaml", "--ckpt", "none.pt", "--j_regressor", "none.npy"]
    with pytest.raises(SystemExit) as e:
        eval_cli.main(eval_cli.parse_args(base + ["--dataset", str(tmp_path / "no_var.npz"), "--uncert_threshold", "0.3"]))
    assert "`var`" in str(e.value.code)
    with pytest.raises(SystemExit) as e:
        eval_cli.main(eval_cli.parse_args(base + ["--dataset", str(tmp_path / "with_var.npz"), "--uncert_threshold", "0.01"]))
    assert "keeps none" in str(e.value.code)
    assert eval_cli.parse_args(base + ["--dataset", "x.npz"]).uncert_threshold is None          # default off


def test_c_abi_declares_and_exports_the_pseudo_labeler():
    L = _lib.lib()
    syms = _lib.header_symbols()
    for s in SYMBOLS:
        assert s in syms, s
        assert hasattr(L, s), s
    assert "#define POCO_ABI_VERSION 4" in _lib.HEADER.read_text()          # additions only: the ABI version is not bumped


def test_c_abi_argument_errors_before_any_gpu_work():
    L = pseudo._bind()
    msg = lambda: L.poco_last_error().decode()      # noqa: E731
    fake, null = C.c_void_p(4096), C.c_void_p(0)   # never dereferenced: every call below is refused before a pointer is used
    L.poco_op_rotmat_to_aa.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    assert L.poco_op_rotmat_to_aa(null, fake, 4, None) == ERR_ARG and "rotmat_to_aa" in msg()
    assert L.poco_op_rotmat_to_aa(fake, null, 4, None) == ERR_ARG and L.poco_op_rotmat_to_aa(fake, fake, 0, None) == ERR_ARG
    h = C.c_void_p()
    for cap, thr, inc, res in ((0, 0.3, 0, 224), ((1 << 24) + 1, 0.3, 0, 224), (8, 0.3, 2, 224), (8, 0.3, 0, 0), (8, float("inf"), 0, 224)):
        assert L.poco_pseudo_create(cap, thr, inc, res, C.byref(h)) == ERR_ARG and "poco_pseudo_create" in msg() and not h.value
    assert L.poco_pseudo_create(8, 0.3, 0, 224, None) == ERR_ARG
    for thr in (0.3, float("nan"), 0.0, -1.0):      # NaN or <= 0: keep every crop
        assert L.poco_pseudo_create(8, thr, 1, 224, C.byref(h)) == 0 and h.value
        L.poco_pseudo_destroy(h)
    assert L.poco_pseudo_create(8, 0.3, 0, 224, C.byref(h)) == 0
    step = lambda p=h, B=4, ptrs=(fake,) * 7, T=1: L.poco_pseudo_step(p, B, ptrs[0], ptrs[1], ptrs[2], T, *ptrs[3:], None)   # noqa: E731
    assert step(p=null) == ERR_ARG and "poco_pseudo_step" in msg()
    assert step(B=0) == ERR_ARG and step(B=-3) == ERR_ARG and step(T=0) == ERR_ARG and step(T=pseudo.MAX_TRAILING + 1) == ERR_ARG
    for k in range(7):
        assert step(ptrs=tuple(null if i == k else fake for i in range(7))) == ERR_ARG, k
    assert step(B=9) == ERR_ARG and "capacity" in msg()                    # more than the capacity: refused, nothing offered
    kept, offered = C.c_int64(-1), C.c_int64(-1)
    assert L.poco_pseudo_finish(h, None, 0, C.byref(kept), C.byref(offered), None) == 0 and (kept.value, offered.value) == (0, 0)
    assert L.poco_pseudo_finish(null, None, 0, C.byref(kept), C.byref(offered), None) == ERR_ARG
    assert L.poco_pseudo_finish(h, None, 0, None, C.byref(offered), None) == ERR_ARG
    assert L.poco_pseudo_reset(null, None) == ERR_ARG and L.poco_pseudo_reset(h, None) == 0
    L.poco_pseudo_destroy(h)
    L.poco_pseudo_destroy(null)
