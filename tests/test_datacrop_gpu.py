"""GPU: poco_dataset_crop (csrc/dataset_crop.hip) and what is built on it against the numpy restatement tests/datacrop_np.py, BIT FOR
BIT (as tests/test_demo_gpu.py demands of the demo crop): mixed image sizes, rotation, flip, scale, noise with clamp, boxes across
and outside the borders, half-integer centres, image indices outside the table; the argument errors; EvalDataset(crop='dataset')
with its one upload per distinct image; run_eval on the dataset crop against the `img` path fed with the restatement's crops."""
import ctypes as C

import numpy as np
import pytest
import torch

from poco_amd import datacrop, evaluate, synth
from tests import datacrop_cases, datacrop_np, util

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def world(cuda):
    imgs = datacrop_cases.images()
    return imgs, [torch.from_numpy(i).to(cuda) for i in imgs], datacrop_cases.catalogue()


def _both(world, rows, res, normalize):
    imgs, dimgs, _ = world
    c = datacrop_cases.columns(rows)
    params = datacrop.batch_params(c["center"], c["scale"], c["rot"], c["flip"], c["pn"], c["sc"], res)
    out = datacrop.dataset_crop(dimgs, c["img"], params, res, normalize).cpu().numpy()
    clamped = np.clip(c["img"], 0, len(imgs) - 1)
    ref = datacrop_np.dataset_crop_np(imgs, clamped, c["center"], np.multiply(c["sc"], c["scale"]), c["rot"], c["flip"], c["pn"], res, normalize)
    return out, ref, c


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("res", [32, 224])
@pytest.mark.parametrize("N,first", [(1, 3), (5, 0), (37, 36)])
def test_kernel_equals_restatement_bitwise(world, N, first, res, normalize):
    """Windows of the catalogue at the three batch sizes: rows [first, first + N); (37, 36) ends exactly at the catalogue's last row.
    test_every_setting runs all 73 rows at both sizes."""
    rows = world[2][first:first + N]
    assert len(rows) == N
    out, ref, _ = _both(world, rows, res, normalize)
    bad = np.argwhere(bits(out) != bits(ref))
    assert bad.size == 0, (len(bad), bad[:4], rows[int(bad[0][0])])


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("res", [32, 224])
def test_every_setting(world, res, normalize):
    """All 73 rows in one launch (every rotation x scale x flip x noise combination, every box), at both sizes: bit for bit, and the
    cases do what they are there for."""
    out, ref, c = _both(world, world[2], res, normalize)
    bad = np.argwhere(bits(out) != bits(ref))
    assert bad.size == 0, (len(bad), bad[:4])
    if not normalize:
        outside = [i for i, ctr in enumerate(c["center"]) if ctr == (-200.0, -200.0)]
        assert outside and not out[outside].any()
        assert any((out[i, 1] == 255).any() for i, pn in enumerate(c["pn"]) if pn[1] > 1)          # the clamp is reached
        k = out.astype(np.float64) * 1024
        plain = [i for i, pn in enumerate(c["pn"]) if pn == (1.0, 1.0, 1.0)]
        assert np.array_equal(k[plain], np.rint(k[plain]))                                           # multiples of 1/1024


def test_sizes_that_are_no_multiple_of_the_tile(world):
    """res = 1, 17, 33, 50: crops that are no multiple of the 16-pixel tile or of the 32-pixel group a block walks."""
    for res in (1, 17, 33, 50):
        out, ref, _ = _both(world, world[2][:9], res, True)
        assert np.array_equal(bits(out), bits(ref)), res


def test_argument_errors_leave_the_output_untouched(world, cuda):
    imgs, dimgs, rows = world
    L = datacrop._bind()
    c = datacrop_cases.columns(rows[:4])
    good = datacrop.batch_params(c["center"], c["scale"], c["rot"], c["flip"], c["pn"], c["sc"], 32)
    good["img"] = [0, 1, 0, 1]
    ptrs = torch.tensor([d.data_ptr() for d in dimgs], dtype=torch.int64, device=cuda)
    hw = torch.tensor([[61, 83], [270, 480]], dtype=torch.int32, device=cuda)
    dpar = torch.from_numpy(good.view(np.uint8).copy()).to(cuda)
    out = torch.full((4, 3, 32, 32), -777.0, device=cuda)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(images=ptrs.data_ptr(), hw_=hw.data_ptr(), n_images=2, d_params=dpar.data_ptr(), h=good, N=4, res=32, o=out.data_ptr()):
        hp = None if h is None else C.c_void_p(h.ctypes.data)
        return L.poco_dataset_crop(C.c_void_p(images), C.c_void_p(hw_), n_images, C.c_void_p(d_params), hp, N, res, 1, C.c_void_p(o), st)

    nan, inf, zero = good.copy(), good.copy(), good.copy()
    nan["src"][2, 1], inf["pn"][0, 0], zero["bb"][3] = np.nan, np.inf, 0
    for kw in (dict(images=0), dict(hw_=0), dict(d_params=0), dict(h=None), dict(o=0), dict(N=0), dict(n_images=0), dict(res=0), dict(res=4097),
               dict(h=nan), dict(h=inf), dict(h=zero)):
        assert call(**kw) == 1, kw
        assert "poco_dataset_crop" in L.poco_last_error().decode()
    torch.cuda.synchronize()
    assert bool((out == -777.0).all())
    assert call() == 0                                                     # and the same buffers with good arguments do run
    torch.cuda.synchronize()
    ref = datacrop_np.dataset_crop_np(imgs, [0, 1, 0, 1], c["center"], np.multiply(c["sc"], c["scale"]), c["rot"], c["flip"], c["pn"], 32, True)
    assert np.array_equal(bits(out.cpu().numpy()), bits(ref))


# ---- EvalDataset(crop="dataset") ------------------------------------------------------------------------------------------------------
NAMES = ["a0.png", "b0.png", "a1.png", "b1.png", "a2.png", "b2.png"]
ROWS = [0, 1, 1, 2, 3, 0, 4, 5, 4]                      # 9 rows over 6 images, some shared, not grouped


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from PIL import Image
    tmp = tmp_path_factory.mktemp("datacrop")
    r = np.random.default_rng(17)
    (tmp / "imgs").mkdir()
    frames = {}
    for k, n in enumerate(NAMES):
        frames[n] = r.integers(0, 256, (120, 160, 3) if k % 2 == 0 else (200, 150, 3), dtype=np.uint8)
        Image.fromarray(frames[n]).save(tmp / "imgs" / n)
    base = dict(imgname=np.array([NAMES[i] for i in ROWS]), center=r.uniform(30, 130, (9, 2)).astype(np.float32),
                scale=r.uniform(0.3, 0.8, 9).astype(np.float32), pose=(0.4 * r.standard_normal((9, 72))).astype(np.float32),
                shape=(0.5 * r.standard_normal((9, 10))).astype(np.float32))
    np.savez(tmp / "ds.npz", **base)
    return tmp, frames, base


def _restated_batch(frames, base, ds):
    imgs = [frames[n] for n in NAMES]
    return datacrop_np.dataset_crop_np(imgs, ROWS, base["center"], ds.aug_scale * base["scale"].astype(np.float64), ds.aug_rot, ds.aug_flip,
                                       ds.aug_pn, 224, True)


@pytest.mark.parametrize("aug", [None, datacrop.AugSpec(rot=-47.5, scale=1.25, flip=True, noise=(0.6, 1.4, 1.0)),
                                 datacrop.AugSpec(random=True, seed=3, cfg=dict(FLIP=1, NOISE_FACTOR=0.4, ROT_FACTOR=30, SCALE_FACTOR=0.25))],
                         ids=["plain", "fixed", "random"])
def test_eval_dataset_batch_equals_restatement_and_uploads_each_image_once(folder, cuda, aug):
    tmp, frames, base = folder
    ds = evaluate.EvalDataset(str(tmp / "ds.npz"), str(tmp / "imgs"), crop="dataset", augment=aug)
    seen = []
    datacrop.upload_hook = lambda a: seen.append(a.shape)
    try:
        before = datacrop.upload_count
        b = ds.batch(0, 9, cuda)
        assert datacrop.upload_count - before == 6 and len(seen) == 6                      # 9 rows, 6 distinct images
        seen.clear()
        b2 = ds.batch(2, 6, cuda)                                                          # rows 1, 2, 3, 0: four images
        assert len(seen) == 4
    finally:
        datacrop.upload_hook = None
    ref = _restated_batch(frames, base, ds)
    assert np.array_equal(bits(b["img"].cpu().numpy()), bits(ref))
    assert np.array_equal(bits(b2["img"].cpu().numpy()), bits(ref[2:6]))
    shapes = np.array([frames[NAMES[i]].shape[:2] for i in ROWS], np.float32)
    s_eff = ds.aug_scale * base["scale"].astype(np.float64)
    assert np.array_equal(b["scale"].cpu().numpy(), s_eff.astype(np.float32)) and np.array_equal(b["orig_shape"].cpu().numpy(), shapes)
    info = np.stack([datacrop_np.bbox_info_np(c, s, hw) for c, s, hw in zip(base["center"], s_eff.astype(np.float32), shapes)])
    assert np.array_equal(b["bbox_info"].cpu().numpy(), info)
    assert np.array_equal(b["focal_length"].cpu().numpy(), np.sqrt(shapes[:, 0] ** 2 + shapes[:, 1] ** 2).astype(np.float32))
    if aug is not None and aug.random:
        assert len(set(ds.aug_rot)) > 1 and ds.aug_flip.any() and not ds.aug_flip.all()
    # rot = 0: no Rodrigues round trip - the file's float32 pose, flipped by the restatement where it is flipped
    want_pose = np.stack([datacrop_np.pose_processing_np(p, r, f) if r != 0 else (datacrop_np.flip_pose_np(p) if f else p)
                          for p, r, f in zip(base["pose"], ds.aug_rot, ds.aug_flip)])
    if aug is None or not aug.random:
        assert (aug is not None) == (not np.array_equal(ds.pose, base["pose"]))
    assert np.abs(ds.pose - want_pose).max() <= 2.0 ** -22                                  # float32 rounding of a float64 result


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return util.make_engine("resnet50-cliff", max_batch=8)


@pytest.mark.parametrize("aug", [None, datacrop.AugSpec(rot=30.0, flip=True)], ids=["plain", "rot30_flip"])
def test_run_eval_equals_the_img_path_on_the_restated_crops(folder, cuda, model, aug):
    """run_eval(crop='dataset') == run_eval on a file that carries the restatement's crops as `img` and the host-transformed ground
    truth as `pose`: the same records, bit for bit (the crops are, and everything behind them is the same code on the same input)."""
    tmp, frames, base = folder
    J = synth.synth_j_regressor_h36m(11)
    ds = evaluate.EvalDataset(str(tmp / "ds.npz"), str(tmp / "imgs"), crop="dataset", augment=aug)
    got = evaluate.run_eval(model, ds, J, batch_size=4, return_records=True)
    shapes = np.array([frames[NAMES[i]].shape[:2] for i in ROWS], np.float32)
    tag = "plain" if aug is None else "aug"
    np.savez(tmp / f"ds_img_{tag}.npz", **dict(base, img=_restated_batch(frames, base, ds), orig_shape=shapes, pose=ds.pose,
                                             scale=(ds.aug_scale * base["scale"].astype(np.float64)).astype(np.float32)))
    want = evaluate.run_eval(model, evaluate.EvalDataset(str(tmp / f"ds_img_{tag}.npz")), J, batch_size=4, return_records=True)
    assert got["N"] == want["N"] == 9 and np.isfinite(got["records"][:, :3]).all()
    assert np.array_equal(got["records"].view(np.uint32), want["records"].view(np.uint32))
    if aug is None:
        assert np.array_equal(ds.pose, base["pose"])
        # and the dataset crop is not the demo crop: rounded boxes, no byte rounding
        demo = evaluate.run_eval(model, evaluate.EvalDataset(str(tmp / "ds.npz"), str(tmp / "imgs")), J, batch_size=4, return_records=True)
        assert not np.array_equal(got["records"][:, :3], demo["records"][:, :3])
    else:
        plain = evaluate.EvalDataset(str(tmp / "ds.npz"), str(tmp / "imgs"), crop="dataset")
        assert not np.array_equal(ds.pose, plain.pose)


def test_eval_cli_with_augmentation_flags(folder, cuda, capsys):
    """eval.py --aug_rot 30 --aug_flip on the folder: the setting is printed once, the results file carries the per-sample
    parameters, and the numbers are those of run_eval on the same dataset object."""
    import importlib.util
    from pathlib import Path
    tmp, frames, base = folder
    spec = importlib.util.spec_from_file_location("poco_eval_cli", Path(__file__).resolve().parent.parent / "eval.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    w = util.synth_weights("resnet50-cliff")
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, tmp / "ckpt.pt")
    np.savez(tmp / "smpl.npz", **synth.synth_smpl(7))
    np.save(tmp / "J.npy", synth.synth_j_regressor_h36m(11))
    argv = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(tmp / "ckpt.pt"), "--smpl", str(tmp / "smpl.npz"), "--j_regressor",
            str(tmp / "J.npy"), "--dataset", str(tmp / "ds.npz"), "--img_dir", str(tmp / "imgs"), "--batch_size", "4", "--output_folder",
            str(tmp / "out"), "--aug_rot", "30", "--aug_flip"]
    res = cli.main(cli.parse_args(argv))
    printed = capsys.readouterr().out.splitlines()
    assert sum(line.startswith("Dataset crop:") for line in printed) == 1 and "rot 30 deg" in "\n".join(printed)
    assert printed[-5:] == evaluate.report_lines(res) and res["N"] == 9
    z = dict(np.load(tmp / "out" / "evaluation_results_3dpw.npz"))
    assert np.array_equal(z["aug_rot"], np.full(9, 30, np.float32)) and np.array_equal(z["aug_flip"], np.ones(9, np.int32))
    assert np.array_equal(z["aug_scale"], np.ones(9, np.float32)) and np.array_equal(z["aug_pn"], np.ones((9, 3), np.float32))
    plain = cli.main(cli.parse_args(argv[:-3] + ["--crop", "dataset"]))
    assert not np.array_equal(plain["mpjpe"], res["mpjpe"])
