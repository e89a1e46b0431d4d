"""CPU: the dataset crop's contract without a GPU - the numpy restatement tests/datacrop_np.py and the host
side of poco_amd/datacrop.py against the reference-made fixture tests/golden/datacrop.npz (tools/gen_datacrop_golden.py), the
geometry of the restated warp derived on paper, the exactness claim, the ground-truth transforms, eval.py's flag refusals and the
C entry's argument checks."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from oracle import crop_np
from poco_amd import _lib, datacrop
from tests import datacrop_cases, datacrop_np

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(ROOT / "tests" / "golden" / "datacrop.npz"))


@pytest.fixture(scope="module")
def img():
    return np.random.default_rng(3).integers(0, 256, (90, 120, 3), dtype=np.uint8)


# ---- restatement and host code against the reference's own functions --------------------------------------------------------------
def test_source_points_equal_the_reference(gold):
    """gen_trans_from_patch_cv's float32 triples, bit for bit, from the restatement and from crop_params."""
    for (c_x, c_y, bb, res, rot), src, dst in zip(gold["pts_in"], gold["pts_src"], gold["pts_dst"]):
        s, d = datacrop_np.patch_points(int(c_x), int(c_y), int(bb), int(res), rot)
        assert np.array_equal(s.view(np.uint32), src.view(np.uint32)) and np.array_equal(d.view(np.uint32), dst.view(np.uint32)), rot
        rec = datacrop.crop_params((c_x, c_y), bb / 200.0, rot, 0, (1, 1, 1), 1.0, int(res))
        assert int(rec["bb"]) == int(bb)
        assert np.array_equal(rec["src"].view(np.uint32), src.reshape(6).view(np.uint32)), rot


def test_augm_params_sequences(gold):
    cfg = dict(NOISE_FACTOR=0.4, ROT_FACTOR=30, SCALE_FACTOR=0.25)
    for fi, flip_on in enumerate((1, 0)):
        for si, seed in enumerate(gold["augm_seeds"]):
            rng = np.random.RandomState(int(seed))
            np.random.seed(int(seed))
            for k in range(12):
                want = gold["augm_train"][fi, si, k]
                for f, pn, r, sc in (datacrop.augm_params(rng, dict(cfg, FLIP=flip_on), True), datacrop_np.augm_params_np(dict(cfg, FLIP=flip_on), True)):
                    assert np.array_equal(np.concatenate([[f], pn, [r], [sc]]), want), (flip_on, seed, k)
    assert gold["augm_train"][0, :, :, 0].any() and not gold["augm_train"][1, :, :, 0].any()       # FLIP off never flips ...
    assert np.array_equal(gold["augm_train"][0, :, :, 1:4], gold["augm_train"][1, :, :, 1:4])      # ... but draws its uniform all the same
    f, pn, r, sc = datacrop.augm_params(np.random.RandomState(5), dict(cfg, FLIP=1), False)
    assert np.array_equal(np.concatenate([[f], pn, [r], [sc]]), gold["augm_eval"]) and (f, r, sc) == (0, 0, 1)
    spec = datacrop.AugSpec(random=True, seed=7, cfg=dict(cfg, FLIP=1))
    flip, pn, rot, sc = spec.draw(12)
    assert np.array_equal(np.column_stack([flip, pn, rot, sc]), gold["augm_train"][0, 1])


def test_ground_truth_transforms_equal_the_reference(gold):
    assert datacrop.SMPL_POSE_FLIP_PERM == list(gold["smpl_pose_flip_perm"]) == datacrop_np.SMPL_POSE_FLIP_PERM
    assert datacrop.J24_FLIP_PERM == list(gold["j24_flip_perm"]) == datacrop_np.J24_FLIP_PERM
    for m in (datacrop, datacrop_np):
        fp, fk = (m.flip_pose, m.flip_kp) if m is datacrop else (m.flip_pose_np, m.flip_kp_np)
        j3, j2 = (m.j3d_processing, m.j2d_processing) if m is datacrop else (m.j3d_processing_np, m.j2d_processing_np)
        tr = m.transform if m is datacrop else m.transform_np
        for i, (r, f) in enumerate(gold["gt_rot_flip"]):
            assert np.array_equal(fp(gold["pose"][i]), gold["flip_pose"][i])
            assert np.array_equal(fk(gold["S"][i]), gold["flip_kp"][i])
            y = j3(gold["S"][i], r, int(f))
            assert y.dtype == np.float32 and np.array_equal(y, gold["j3d"][i]), i
            y = j2(gold["kp"][i], gold["kp_center"][i], gold["kp_scale"][i], r, int(f))
            assert y.dtype == np.float32 and np.array_equal(y, gold["j2d"][i]), i
            assert np.array_equal(tr(gold["kp"][i, 0, :2] + 1, gold["kp_center"][i], gold["kp_scale"][i], [224, 224], rot=r), gold["transform"][i])
    from poco_amd.tester import calculate_bbox_info
    for c, s, hw, want in zip(gold["kp_center"], gold["kp_scale"], gold["bbox_shape"], gold["bbox_info"]):
        assert np.array_equal(datacrop_np.bbox_info_np(c, s, hw), want) and np.array_equal(calculate_bbox_info(c, s, hw), want)


def test_crop_keypoints_without_augmentation_match_the_demo_path(gold):
    """j2d_processing -> back to pixels (float32) == segm.crop_keypoints24, which skips the normalisation, up to float32 rounding."""
    from poco_amd import segm
    a = datacrop.crop_keypoints24(gold["kp"], gold["kp_center"], gold["kp_scale"], np.zeros(4), np.zeros(4, np.int32))
    b = segm.crop_keypoints24(gold["kp"], gold["kp_center"], gold["kp_scale"])
    assert a.dtype == np.float32 and np.abs(a - b).max() <= 224 * 2.0 ** -22


def test_flip_pose_twice_is_identity_and_rot_aa_matches_scipy(gold):
    from scipy.spatial.transform import Rotation
    for p in gold["pose"]:
        assert np.array_equal(datacrop.flip_pose(datacrop.flip_pose(p)), p)
        assert np.array_equal(datacrop_np.flip_pose_np(datacrop_np.flip_pose_np(p)), p)
    r = np.random.default_rng(8)
    aas = list(0.8 * r.standard_normal((20, 3))) + [np.zeros(3), np.array([np.pi - 1e-9, 0, 0]), np.array([0, 0, 3.0]), 1e-9 * np.ones(3)]
    for aa in aas:
        for rot in (30.0, -47.5, 90.0, 180.0, 0.0):
            got, want = datacrop.rot_aa(aa, rot), datacrop_np.rot_aa_np(aa, rot)
            # compare as rotations (at an angle of pi the axis sign is free), in float64: a few ulp of the matrix entries
            d = Rotation.from_rotvec(got).as_matrix() - Rotation.from_rotvec(want).as_matrix()
            assert np.abs(d).max() <= 1e-12, (aa, rot)
            assert np.linalg.norm(got) <= np.pi + 1e-12
    p = gold["pose"][0]
    assert np.array_equal(datacrop.pose_processing(p, 0, 0), p.astype(np.float32))               # rot = 0: the file's bits
    assert np.abs(datacrop.pose_processing(p, 30.0, 1) - datacrop_np.pose_processing_np(p, 30.0, 1)).max() <= 2.0 ** -22


# ---- geometry of the restated warp --------------------------------------------------------------------------------------------------
RES = 32
CX, CY = 60, 45           # integer centre; with scale = RES / 200 the box side equals the crop side


def _crop(img, rot, flip=0, pn=(1, 1, 1), center=(CX, CY), scale=RES / 200.0):
    return datacrop_np.rgb_processing_np(img, center, scale, rot, flip, pn, RES, normalize=False).transpose(1, 2, 0)


def test_identity_returns_the_source_window(img):
    """rot = 0, sc = 1, integer centre, bb == res: dst = src - (c - res/2), so output (x, y) is source (c_x - res/2 + x, c_y - res/2 + y)."""
    h = RES // 2
    assert np.array_equal(_crop(img, 0.0), img[CY - h:CY + h, CX - h:CX + h].astype(np.float32))


def test_flip_is_fliplr_of_the_unflipped_crop(img):
    for rot in (0.0, 30.0):
        assert np.array_equal(_crop(img, rot, flip=1), np.fliplr(_crop(img, rot)))


def test_rot180_is_the_window_reversed_with_its_one_pixel_shift(img):
    """rot = 180: down = (0, -h), right = (-h, 0) (sin(pi) * h = 1e-15 vanishes when added to the centre), so dst (res/2 + u, res/2 + v)
    is src (c_x - u, c_y - v): output x shows source column c_x + res/2 - x, i.e. columns c_x - res/2 + 1 .. c_x + res/2 reversed -
    ONE pixel to the right of the identity window, because dst_center = res/2 is not the middle (res - 1)/2 of the pixel grid."""
    h = RES // 2
    assert np.array_equal(_crop(img, 180.0), img[CY - h + 1:CY + h + 1, CX - h + 1:CX + h + 1][::-1, ::-1].astype(np.float32))


def test_rot90_sign(img):
    """rot = +90: down = (-h, 0), right = (0, h): output (x, y) reads source (c_x + res/2 - y, c_y - res/2 + x) - the window of rows
    c_y - res/2 .., columns c_x - res/2 + 1 .. turned COUNTER-clockwise (np.rot90(w, 1)[y, x] = w[x, n - 1 - y]).  rot = -90 reads
    (c_x - res/2 + y, c_y + res/2 - x): rows shifted by one instead, turned clockwise.  A positive rot therefore turns the image
    content counter-clockwise on the screen (y down), which is why get_transform negates it 'to match the crop'."""
    h = RES // 2
    assert np.array_equal(_crop(img, 90.0), np.rot90(img[CY - h:CY + h, CX - h + 1:CX + h + 1], 1).astype(np.float32))
    assert np.array_equal(_crop(img, -90.0), np.rot90(img[CY - h + 1:CY + h + 1, CX - h:CX + h], -1).astype(np.float32))


def test_raw_values_are_multiples_of_1_1024_and_the_integer_form_is_exact(img):
    """The float blend of byte-valued taps: every value x 1024 is an integer, and equals (sum v_i m_i) / 1024 computed in integers
    - the form the kernel uses."""
    for rot, scale in ((30.0, 0.31), (-47.5, 0.12), (0.0, 0.2037)):
        y = _crop(img, rot, scale=scale, center=(59.6, 44.5))
        k = y.astype(np.float64) * 1024
        assert np.array_equal(k, np.rint(k)) and y.max() <= 255 and y.min() >= 0 and len(np.unique(k % 1024)) > 8
        c_x, c_y, bb = datacrop_np.py_round(59.6), datacrop_np.py_round(44.5), datacrop_np.py_round(scale * 200.0)
        assert (c_x, c_y) == (60, 44)                                                 # round half to even
        src, dst = datacrop_np.patch_points(c_x, c_y, bb, RES, rot)
        Mi = crop_np.invert_affine_cv(crop_np.get_affine_transform_cv(src, dst))
        xs = np.arange(RES, dtype=np.float64)
        X = ((np.rint((Mi[1] * xs + Mi[2]) * 1024).astype(np.int64) + 16)[:, None] + np.rint(Mi[0] * xs * 1024).astype(np.int64)[None, :]) >> 5
        Y = ((np.rint((Mi[4] * xs + Mi[5]) * 1024).astype(np.int64) + 16)[:, None] + np.rint(Mi[3] * xs * 1024).astype(np.int64)[None, :]) >> 5
        sx, sy, fx, fy = X >> 5, Y >> 5, X & 31, Y & 31
        H, W = img.shape[:2]
        f = img.astype(np.int64)

        def px(xx, yy):
            ok = (xx >= 0) & (xx < W) & (yy >= 0) & (yy < H)
            return np.where(ok[..., None], f[np.clip(yy, 0, H - 1), np.clip(xx, 0, W - 1)], 0)
        acc = ((32 - fy) * (32 - fx))[..., None] * px(sx, sy) + ((32 - fy) * fx)[..., None] * px(sx + 1, sy) \
            + (fy * (32 - fx))[..., None] * px(sx, sy + 1) + (fy * fx)[..., None] * px(sx + 1, sy + 1)
        assert np.array_equal(acc, k.astype(np.int64))


def test_outside_taps_are_zero_and_never_an_index_error(img):
    assert not _crop(img, 30.0, center=(-500.0, -500.0)).any()
    assert not _crop(img, 0.0, center=(1e4, 40.0)).any()
    y = _crop(img, 0.0, center=(0.0, 0.0))                                   # the window starts at (-16, -16)
    assert not y[:15].any() and not y[:, :15].any() and np.array_equal(y[16:, 16:], img[:16, :16].astype(np.float32))
    big = _crop(img, -47.5, center=(60.0, 45.0), scale=5.0)                  # a 1000 px box around a 120 x 90 image
    assert big.any() and not big[0].any() and not big[-1].any()
    tiny = np.full((1, 1, 3), 200, np.uint8)
    assert _crop(tiny, 0.0, center=(0.0, 0.0)).max() == 200.0


def test_noise_clamps_and_normalisation_order(img):
    raw = _crop(img, 30.0)
    y = _crop(img, 30.0, pn=(0.6, 1.4, 1.0))
    assert np.array_equal(y[..., 0], raw[..., 0] * np.float32(0.6)) and np.array_equal(y[..., 2], raw[..., 2])
    assert np.array_equal(y[..., 1], np.minimum(np.float32(255), raw[..., 1] * np.float32(1.4))) and (y[..., 1] == 255).any()
    n = datacrop_np.rgb_processing_np(img, (CX, CY), RES / 200.0, 30.0, 0, (0.6, 1.4, 1.0), RES, normalize=True)
    want = ((y / np.float32(255.0) - crop_np.MEAN) / crop_np.STD).transpose(2, 0, 1)
    assert n.dtype == np.float32 and np.array_equal(n, want)
    # byte-valued crops go through the very function the demo path is pinned with
    ident = _crop(img, 0.0)
    assert np.array_equal(datacrop_np.rgb_processing_np(img, (CX, CY), RES / 200.0, 0.0, 0, (1, 1, 1), RES)[None],
                          crop_np.normalize_np(ident.astype(np.uint8)[None]))


def test_float_crop_and_uint8_crop_differ_by_the_byte_rounding_only():
    """The gap --crop dataset closes: on the same integer box the demo's crop is cv2's uint8 path, whose weights are the float ones
    rounded to 2^-15 (each off by at most 2^-16, the (0,0) entry by 2^-15) and whose result is rounded to a byte: at most
    0.5 + 255 * 4 * 2^-16 + 255 * 2^-15 grey levels from the float crop - and on a smooth image nearly that far."""
    yy, xx = np.mgrid[0:200, 0:260].astype(np.float64)
    smooth = np.stack([127 + 120 * np.sin(xx / 23.0) * np.cos(yy / 31.0), xx * 255 / 259, yy * 255 / 199], 2).round().astype(np.uint8)
    f = datacrop_np.rgb_processing_np(smooth, (130, 100), 0.83, 0.0, 0, (1, 1, 1), 224, normalize=False).transpose(1, 2, 0)
    u = crop_np.crop_u8_np(smooth, np.array([[130.0, 100.0, 166.0, 166.0]]), 1.0, 224)[0]
    d = np.abs(f.astype(np.float64) - u.astype(np.float64))
    bound = 0.5 + 255 * 4 * 2.0 ** -16 + 255 * 2.0 ** -15
    print(f"float crop vs uint8 crop: max {d.max():.4f} grey levels (bound {bound:.4f})")
    assert 0.45 < d.max() <= bound


def test_cases_cover_what_the_gpu_test_promises():
    rows = datacrop_cases.catalogue()
    combos = {(r["rot"], r["sc"], r["flip"], r["pn"]) for r in rows}
    assert len(combos) == 60 and len(rows) == 73
    assert {(r["img"], r["center"], r["scale"]) for r in rows} == {(b[0], (b[1], b[2]), b[3]) for b in datacrop_cases.BOXES}
    five = rows[:5]
    assert any(r["rot"] != 0 for r in five) and any(r["flip"] for r in five) and any(r["pn"][1] > 1 for r in five)
    imgs = datacrop_cases.images()
    assert [i.shape for i in imgs] == [(61, 83, 3), (270, 480, 3)]
    # the all-zero case really is all zero and the clamp really clamps, in the restatement
    c = datacrop_cases.columns([r for r in rows if r["center"] == (-200.0, -200.0)][:1])
    assert not datacrop_np.dataset_crop_np(imgs, [0], c["center"], np.multiply(c["sc"], c["scale"]), c["rot"], c["flip"], c["pn"], 32, False).any()


# ---- eval.py ------------------------------------------------------------------------------------------------------------------------
def _cli():
    spec = importlib.util.spec_from_file_location("poco_eval_cli", ROOT / "eval.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_eval_flags_and_refusals(tmp_path):
    cli = _cli()
    base = dict(imgname=np.array(["a.png", "b.png"]), center=np.zeros((2, 2), np.float32), scale=np.ones(2, np.float32),
                pose=np.zeros((2, 72), np.float32), shape=np.zeros((2, 10), np.float32))
    np.savez(tmp_path / "files.npz", **base)
    np.savez(tmp_path / "img.npz", img=np.zeros((2, 3, 224, 224), np.float32), **base)
    (tmp_path / "imgs").mkdir()
    common = ["--cfg", "configs/demo_poco_cliff.yaml", "--ckpt", "none.pt", "--j_regressor", "none.npy"]

    def spec_of(*extra, ds="files.npz", img_dir=True):
        args = cli.parse_args(common + ["--dataset", str(tmp_path / ds)] + (["--img_dir", str(tmp_path / "imgs")] if img_dir else []) + list(extra))
        return args, cli.augmentation_spec(args)

    args, aug = spec_of()
    assert args.crop == "demo" and aug is None                                   # nothing changes without the flags
    args, aug = spec_of("--crop", "dataset")
    assert args.crop == "dataset" and (aug.rot, aug.scale, aug.flip, tuple(aug.noise), aug.random) == (0.0, 1.0, False, (1.0, 1.0, 1.0), False)
    args, aug = spec_of("--aug_rot", "30", "--aug_flip", "--aug_noise", "0.6,1.4,1", "--aug_scale", "1.25")
    assert args.crop == "dataset" and (aug.rot, aug.scale, aug.flip, tuple(aug.noise)) == (30.0, 1.25, True, (0.6, 1.4, 1.0))
    assert "rot 30" in aug.describe() and "flip 1" in aug.describe()
    args, aug = spec_of("--augment", "--aug_seed", "7")
    assert args.crop == "dataset" and aug.random and aug.seed == 7 and aug.cfg.ROT_FACTOR == 30 and aug.cfg.NOISE_FACTOR == 0.4
    for extra, kw, word in ((["--aug_rot", "30"], dict(ds="img.npz"), "`img`"), (["--augment"], dict(ds="img.npz"), "`img`"),
                            (["--crop", "dataset"], dict(ds="img.npz"), "`img`"), (["--aug_flip"], dict(img_dir=False), "--img_dir"),
                            (["--augment", "--aug_rot", "3"], {}, "--aug_rot"), (["--aug_noise", "1,2"], {}, "--aug_noise"),
                            (["--aug_noise", "1,x,2"], {}, "--aug_noise"), (["--aug_noise", "1,nan,2"], {}, "--aug_noise"),
                            (["--aug_scale", "0"], {}, "--aug_scale"), (["--aug_rot", "inf"], {}, "--aug_rot")):
        with pytest.raises(SystemExit) as e:
            spec_of(*extra, **kw)
        assert word in str(e.value.code), (extra, e.value.code)
    # main() refuses before the checkpoint, the regressor or the GPU are looked at
    with pytest.raises(SystemExit) as e:
        cli.main(cli.parse_args(common + ["--dataset", str(tmp_path / "img.npz"), "--aug_rot", "30"]))
    assert "`img`" in str(e.value.code)
    from poco_amd import evaluate
    with pytest.raises(ValueError, match="crop='dataset'"):
        evaluate.EvalDataset(str(tmp_path / "img.npz"), None, crop="demo", augment=datacrop.AugSpec(rot=3))
    with pytest.raises(ValueError, match="ready-made"):
        evaluate.EvalDataset(str(tmp_path / "img.npz"), None, crop="dataset")
    ds = evaluate.EvalDataset(str(tmp_path / "files.npz"), str(tmp_path / "imgs"), crop="dataset", augment=datacrop.AugSpec(scale=1.25, flip=True))
    assert np.array_equal(ds.scale_eff, [1.25, 1.25]) and np.array_equal(ds.scale, [1, 1]) and ds.aug_flip.tolist() == [1, 1]


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_and_exported():
    syms = _lib.header_symbols()
    L = _lib.lib()
    assert "poco_dataset_crop" in syms and hasattr(L, "poco_dataset_crop")
    assert "#define POCO_ABI_VERSION 4" in _lib.HEADER.read_text()                     # an addition: the ABI version is not bumped


def test_argument_errors_without_a_gpu():
    """Refused before any GPU work: the fake device pointers are never dereferenced (as tests/test_ops_capi_cpu.py does)."""
    L = datacrop._bind()
    FAKE, NULL = C.c_void_p(4096), C.c_void_p(0)
    good = datacrop.batch_params([(40, 30)] * 3, [0.2] * 3, [30.0] * 3, [0] * 3, [(1, 1, 1)] * 3, [1.0] * 3, 32)

    def call(images=FAKE, hw=FAKE, n_images=2, d_params=FAKE, h=good, N=3, res=32, out=FAKE):
        hp = NULL if h is None else C.c_void_p(h.ctypes.data)
        return L.poco_dataset_crop(images, hw, n_images, d_params, hp, N, res, 1, out, NULL), L.poco_last_error().decode()

    bad = {}
    for k, v in (("src", np.nan), ("src", np.inf), ("pn", -np.inf), ("pn", np.nan)):
        p = good.copy()
        p[k][1, 2] = v
        bad[(k, v)] = p
    zero = good.copy()
    zero["bb"][2] = 0
    assert int(datacrop.crop_params((40, 30), 0.002, 0, 0, (1, 1, 1), 1.0, 32)["bb"]) == 0          # 0.4 px rounds to 0
    for kw, word in [(dict(images=NULL), "null"), (dict(hw=NULL), "null"), (dict(d_params=NULL), "null"), (dict(h=None), "null"),
                     (dict(out=NULL), "null"), (dict(N=0), "at least 1"), (dict(N=-4), "at least 1"), (dict(n_images=0), "at least 1"),
                     (dict(res=0), "1..4096"), (dict(res=4097), "1..4096"), (dict(h=zero), "rounds to 0")] \
            + [(dict(h=p), "non-finite") for p in bad.values()]:
        rc, msg = call(**kw)
        assert rc == 1 and "poco_dataset_crop" in msg and word in msg, (kw.keys(), rc, msg)
    with pytest.raises(ValueError, match="finite"):
        datacrop.crop_params((np.nan, 3), 1.0, 0, 0, (1, 1, 1), 1.0, 224)
    with pytest.raises(ValueError, match="finite"):
        datacrop.crop_params((1, 3), 1.0, 0, 0, (1, np.inf, 1), 1.0, 224)
