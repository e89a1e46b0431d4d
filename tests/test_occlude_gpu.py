"""GPU: poco_dataset_crop_occ (csrc/dataset_crop.hip) and what is built on it against the numpy restatement tests/occlude_np.py, BIT FOR
BIT, raw and normalised, with the cover counts: every paste case of tests/occlude_cases.py (all resize paths, every edge, outside,
both orders of an overlap, 0 / 1 / 7 objects) at res 224 and 32 over two image sizes, together with flip, rotation and noise; all
counts zero against poco_dataset_crop; the argument errors; EvalDataset(occlude=...) with its upload count; run_eval on occluded
crops against the `img` path fed with the restatement's crops; eval.py --aug_occlude."""
import ctypes as C

import numpy as np
import pytest
import torch

from poco_amd import datacrop, evaluate, synth
from tests import datacrop_cases, occlude_cases, occlude_np, util
from tests.test_occlude_cpu import bad_occ_calls, good_occ_inputs, occ_call

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def world(cuda):
    imgs, cuts = datacrop_cases.images(), occlude_cases.cutouts()
    return imgs, [torch.from_numpy(i).to(cuda) for i in imgs], cuts, datacrop.OccluderAtlas(cuts, cuda)


# crop settings the paste cases cycle through: (image, centre, scale, rot, flip, pn) - both image sizes, flip, rotation 30, noise with clamp
SETTINGS = [(0, (40.0, 30.0), 0.2, 0.0, 0, (1.0, 1.0, 1.0)), (1, (240.0, 135.0), 0.9, 30.0, 1, (0.6, 1.4, 1.0)),
            (1, (478.0, 268.0), 0.25, 30.0, 0, (1.0, 1.0, 1.0)), (0, (41.0, 30.0), 1.0, 0.0, 1, (0.6, 1.4, 1.0))]


def _columns(n):
    s = [SETTINGS[k % len(SETTINGS)] for k in range(n)]
    return dict(img=[x[0] for x in s], center=[x[1] for x in s], scale=[x[2] for x in s], rot=[x[3] for x in s], flip=[x[4] for x in s],
                pn=[x[5] for x in s])


def _both(world, objects, res, normalize):
    imgs, dimgs, cuts, atlas = world
    c = _columns(len(objects))
    params = datacrop.batch_params(c["center"], c["scale"], c["rot"], c["flip"], c["pn"], np.ones(len(objects)), res)
    out, cover = datacrop.dataset_crop(dimgs, c["img"], params, res, normalize, occlusion=(atlas, datacrop.occ_records(objects)))
    ref, ref_cover = occlude_np.dataset_crop_occ_np(imgs, c["img"], c["center"], c["scale"], c["rot"], c["flip"], c["pn"], cuts, objects, res, normalize)
    return out.cpu().numpy(), cover.cpu().numpy(), ref, ref_cover


@pytest.mark.parametrize("normalize", [False, True])
@pytest.mark.parametrize("res", [32, 224])
def test_kernel_equals_restatement_bitwise(world, res, normalize):
    """Every paste case in one launch, each under a crop setting of its own; the cases do what they are there for."""
    g = occlude_cases.geometry(res)
    names = list(g)
    out, cover, ref, ref_cover = _both(world, [g[k] for k in names], res, normalize)
    bad = np.argwhere(bits(out) != bits(ref))
    assert bad.size == 0, (len(bad), bad[:4], names[int(bad[0][0])])
    assert cover.dtype == np.int32 and np.array_equal(cover, ref_cover), [(n, a, b) for n, a, b in zip(names, cover, ref_cover) if a != b]
    by = dict(zip(names, cover))
    assert by["none"] == by["outside"] == by["outside_far"] == 0 and by["seven"] > by["inside_fast_2x2"] > 0
    assert 0 < by["cut_left"] < by["inside_generic_even"] and 0 < by["corner"]
    assert by["overlap_ab"] == by["overlap_ba"]                                # the same pixels are touched; the order is the next test's


@pytest.mark.parametrize("res", [32, 224])
def test_two_overlapping_objects_in_both_orders(world, res):
    """The same crop setting four times (SETTINGS repeat every 4): rows 0 and 4 hold the two orders.  They differ, each is right."""
    g = occlude_cases.geometry(res)
    objects = [g["overlap_ab"], [], [], [], g["overlap_ba"]]
    out, cover, ref, ref_cover = _both(world, objects, res, False)
    assert np.array_equal(bits(out), bits(ref)) and np.array_equal(cover, ref_cover)
    assert not np.array_equal(out[0], out[4]) and cover[0] == cover[4] > 0 and np.array_equal(out[1], ref[1])


def test_sizes_that_are_no_multiple_of_the_tile(world):
    """res 17, 33, 50: the cover cells of partly filled blocks; seven objects, one per block row and column at least."""
    for res in (17, 33, 50):
        g = occlude_cases.geometry(res)
        out, cover, ref, ref_cover = _both(world, [g["seven"], g["corner"], g["cut_bottom"], g["inside_generic_even"], g["none"]], res, True)
        assert np.array_equal(bits(out), bits(ref)) and np.array_equal(cover, ref_cover), res


def test_all_counts_zero_equals_the_plain_entry(world):
    """With every count 0 poco_dataset_crop_occ gives poco_dataset_crop's output bit for bit (37 catalogue rows, both outputs)."""
    imgs, dimgs, cuts, atlas = world
    c = datacrop_cases.columns(datacrop_cases.catalogue()[:37])
    for res, normalize in ((224, True), (32, False), (33, True)):
        params = datacrop.batch_params(c["center"], c["scale"], c["rot"], c["flip"], c["pn"], c["sc"], res)
        plain = datacrop.dataset_crop(dimgs, c["img"], params, res, normalize)
        assert torch.is_tensor(plain)                                          # the old call returns what it returned
        occ, cover = datacrop.dataset_crop(dimgs, c["img"], params, res, normalize, occlusion=(atlas, datacrop.occ_records([[]] * 37)))
        assert np.array_equal(bits(occ.cpu().numpy()), bits(plain.cpu().numpy())) and not cover.any()


def test_argument_errors_leave_the_outputs_untouched(world, cuda):
    imgs, dimgs, cuts, atlas = world
    L = datacrop._bind_occ()
    _, params, table, recs = good_occ_inputs()
    assert np.array_equal(table, atlas.table)
    params["img"] = [0, 1, 0]
    ptrs = torch.tensor([d.data_ptr() for d in dimgs], dtype=torch.int64, device=cuda)
    hw = torch.tensor([[61, 83], [270, 480]], dtype=torch.int32, device=cuda)
    dpar = torch.from_numpy(params.view(np.uint8).copy()).to(cuda)
    docc = torch.from_numpy(recs.view(np.uint8).copy()).to(cuda)
    out = torch.full((3, 3, 32, 32), -777.0, device=cuda)
    cover = torch.full((3, 1), -5, dtype=torch.int32, device=cuda)
    p = lambda t: C.c_void_p(t.data_ptr())   # noqa: E731
    base = dict(images=p(ptrs), hw=p(hw), n_images=2, d_params=p(dpar), h=params, N=3, res=32, atlas=p(atlas.d_atlas), texels=atlas.texels,
                d_table=p(atlas.d_table), h_table=table, d_occ=p(docc), h_occ=recs, out=p(out), cover=p(cover))
    for label, ch in bad_occ_calls(params, table, recs):
        if label == "atlas alignment":
            ch = dict(atlas=C.c_void_p(atlas.d_atlas.data_ptr() + 2))
        assert occ_call(L, dict(base, **ch)) == 1, label
        assert "poco_dataset_crop_occ" in L.poco_last_error().decode(), label
    torch.cuda.synchronize()
    assert bool((out == -777.0).all()) and bool((cover == -5).all())
    assert occ_call(L, base) == 0                                               # and the same buffers with good arguments do run
    torch.cuda.synchronize()
    g = occlude_cases.geometry(32)
    ref, ref_cover = occlude_np.dataset_crop_occ_np(imgs, [0, 1, 0], [(40, 30)] * 3, [0.2] * 3, [30.0] * 3, [0] * 3, [(1, 1, 1)] * 3, cuts,
                                                    [g["seven"], g["inside_fast_2x2"], g["none"]], 32, True)
    assert np.array_equal(bits(out.cpu().numpy()), bits(ref)) and np.array_equal(cover.cpu().numpy()[:, 0], ref_cover)
    assert occ_call(L, dict(base, cover=C.c_void_p(0))) == 0                    # the cover is optional
    torch.cuda.synchronize()
    assert np.array_equal(bits(out.cpu().numpy()), bits(ref))


# ---- EvalDataset(crop="dataset", occlude=...) -------------------------------------------------------------------------------------------
NAMES = ["a0.png", "b0.png", "a1.png", "b1.png", "a2.png", "b2.png"]
ROWS = [0, 1, 1, 2, 3, 0, 4, 5, 4]                      # 9 rows over 6 images, some shared, not grouped
CFG = dict(FLIP=1, NOISE_FACTOR=0.4, ROT_FACTOR=30, SCALE_FACTOR=0.25)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    from PIL import Image
    tmp = tmp_path_factory.mktemp("occlude")
    r = np.random.default_rng(19)
    (tmp / "imgs").mkdir()
    frames = {}
    for k, n in enumerate(NAMES):
        frames[n] = r.integers(0, 256, (120, 160, 3) if k % 2 == 0 else (200, 150, 3), dtype=np.uint8)
        Image.fromarray(frames[n]).save(tmp / "imgs" / n)
    center = r.uniform(50, 110, (9, 2)).astype(np.float32)
    scale = r.uniform(0.3, 0.8, 9).astype(np.float32)
    # keypoints inside the boxes, a few invisible ones; row 7 has no visible keypoint at all
    part = np.concatenate([center[:, None, :] + r.uniform(-0.8, 0.8, (9, 24, 2)) * 100 * scale[:, None, None],
                           r.choice([0.0, 1.0], (9, 24, 1), p=[0.15, 0.85])], 2)
    part[7, :, 2] = 0
    base = dict(imgname=np.array([NAMES[i] for i in ROWS]), center=center, scale=scale, pose=(0.4 * r.standard_normal((9, 72))).astype(np.float32),
                shape=(0.5 * r.standard_normal((9, 10))).astype(np.float32), part=part)
    np.savez(tmp / "ds.npz", **base)
    np.savez(tmp / "occ.npz", **{f"c{i}": c for i, c in enumerate(occlude_cases.cutouts())})
    return tmp, frames, base


def _objects(ds):
    return [[tuple(int(v) for v in ds.occ_records["obj"][n, k].tolist()) for k in range(int(ds.occ_records["count"][n]))] for n in range(len(ds))]


def _restated_batch(frames, base, ds):
    imgs = [frames[n] for n in NAMES]
    return occlude_np.dataset_crop_occ_np(imgs, ROWS, base["center"], ds.aug_scale * base["scale"].astype(np.float64), ds.aug_rot, ds.aug_flip,
                                          ds.aug_pn, occlude_cases.cutouts(), _objects(ds), 224, True)


@pytest.mark.parametrize("aug", [None, datacrop.AugSpec(rot=30.0, flip=True, noise=(0.6, 1.4, 1.0)), datacrop.AugSpec(random=True, seed=3, cfg=CFG)],
                         ids=["plain", "fixed", "random"])
def test_eval_dataset_batch_equals_restatement_and_uploads_each_image_once(folder, cuda, aug):
    tmp, frames, base = folder
    spec = datacrop.OcclusionSpec(occlude_cases.cutouts(), seed=3)
    ds = evaluate.EvalDataset(str(tmp / "ds.npz"), str(tmp / "imgs"), crop="dataset", augment=aug, occlude=spec)
    assert ds.occ_no_visible == 1 and ds.occ_count[7] == 0 and (np.delete(ds.occ_count, 7) >= 1).all() and ds.occ_count.max() <= 7
    spec.atlas(cuda)                                                            # the atlas goes up once, outside the image uploads
    seen = []
    datacrop.upload_hook = lambda a: seen.append(a.shape)
    try:
        before = datacrop.upload_count
        b = ds.batch(0, 9, cuda)
        assert datacrop.upload_count - before == 6 and len(seen) == 6          # 9 rows, 6 distinct images: unchanged by the occluders
        seen.clear()
        b2 = ds.batch(2, 6, cuda)
        assert len(seen) == 4
    finally:
        datacrop.upload_hook = None
    assert spec.atlas(cuda) is spec.atlas(cuda) and len(spec._atlas) == 1
    ref, ref_cover = _restated_batch(frames, base, ds)
    assert np.array_equal(bits(b["img"].cpu().numpy()), bits(ref))
    assert np.array_equal(bits(b2["img"].cpu().numpy()), bits(ref[2:6]))
    assert np.array_equal(ds.occ_cover, ref_cover / float(224 * 224)) and ds.occ_cover[7] == 0 and ds.occ_cover.max() > 0
    plain = evaluate.EvalDataset(str(tmp / "ds.npz"), str(tmp / "imgs"), crop="dataset", augment=aug)
    if aug is None or not aug.random:                                          # a fixed setting is the same with and without occluders
        pb = plain.batch(0, 9, cuda)["img"].cpu().numpy()
        assert np.array_equal(bits(pb[7]), bits(ref[7])) and not np.array_equal(pb[0], ref[0])
        assert np.array_equal(plain.aug_rot, ds.aug_rot) and np.array_equal(plain.pose, ds.pose)


# ---- end to end -----------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def model():
    return util.make_engine("resnet50-cliff", max_batch=8)


def test_run_eval_equals_the_img_path_on_the_restated_crops(folder, cuda, model):
    """run_eval on occluded crops == run_eval on a file that carries the restatement's occluded crops as `img`: the same records,
    bit for bit; and the occluders change the result."""
    tmp, frames, base = folder
    J = synth.synth_j_regressor_h36m(11)
    aug = datacrop.AugSpec(rot=30.0, flip=True)
    ds = evaluate.EvalDataset(str(tmp / "ds.npz"), str(tmp / "imgs"), crop="dataset", augment=aug,
                              occlude=datacrop.OcclusionSpec(occlude_cases.cutouts(), seed=5))
    got = evaluate.run_eval(model, ds, J, batch_size=4, return_records=True)
    shapes = np.array([frames[NAMES[i]].shape[:2] for i in ROWS], np.float32)
    ref, ref_cover = _restated_batch(frames, base, ds)
    img_base = {k: v for k, v in base.items() if k != "part"}
    np.savez(tmp / "ds_img.npz", **dict(img_base, img=ref, orig_shape=shapes, pose=ds.pose,
                                        scale=(ds.aug_scale * base["scale"].astype(np.float64)).astype(np.float32)))
    want = evaluate.run_eval(model, evaluate.EvalDataset(str(tmp / "ds_img.npz")), J, batch_size=4, return_records=True)
    assert got["N"] == want["N"] == 9 and np.isfinite(got["records"][:, :3]).all()
    assert np.array_equal(got["records"].view(np.uint32), want["records"].view(np.uint32))
    assert np.array_equal(ds.occ_cover, ref_cover / float(224 * 224))
    plain = evaluate.run_eval(model, evaluate.EvalDataset(str(tmp / "ds.npz"), str(tmp / "imgs"), crop="dataset", augment=aug), J, batch_size=4,
                              return_records=True)
    assert not np.array_equal(got["records"][:, :3], plain["records"][:, :3])
    r = evaluate.cover_uncert_corr(ds.occ_cover, got["corr_y"])
    u = np.asarray(got["corr_y"], np.float64).reshape(9, -1).mean(1)
    assert r == pytest.approx(np.corrcoef(ds.occ_cover, u)[0, 1], abs=1e-12)


def test_eval_cli_with_aug_occlude(folder, cuda, capsys):
    """eval.py --aug_occlude FILE --aug_rot 30: the setting is printed once, the report carries the occluder lines, the results file
    gains occ_count and occ_cover, and the numbers are those of the dataset object."""
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
            str(tmp / "out"), "--aug_rot", "30", "--aug_occlude", str(tmp / "occ.npz"), "--aug_seed", "5"]
    res = cli.main(cli.parse_args(argv))
    printed = capsys.readouterr().out.splitlines()
    assert sum(line.startswith("Synthetic occluders:") for line in printed) == 1 and sum(line.startswith("Dataset crop:") for line in printed) == 1
    assert "5 cut-outs" in "\n".join(printed) and "seed 5" in "\n".join(printed)
    assert printed[-8:-3] == evaluate.report_lines(res) and res["N"] == 9
    assert printed[-3].startswith("Occluders per crop: ") and printed[-2].startswith("Occluder cover: ")
    z = dict(np.load(tmp / "out" / "evaluation_results_3dpw.npz"))
    ds = evaluate.EvalDataset(str(tmp / "ds.npz"), str(tmp / "imgs"), crop="dataset", augment=datacrop.AugSpec(rot=30.0),
                              occlude=datacrop.OcclusionSpec(occlude_cases.cutouts(), seed=5))
    assert z["occ_count"].dtype == np.int32 and np.array_equal(z["occ_count"], ds.occ_count) and z["occ_cover"].dtype == np.float32
    assert z["occ_cover"][7] == 0 and (np.delete(z["occ_cover"], 7) > 0).all() and np.array_equal(z["aug_rot"], np.full(9, 30, np.float32))
    assert float(printed[-3].split(": ")[1].split(" ")[0]) == pytest.approx(ds.occ_count.mean())
    assert float(printed[-2].split(": ")[1]) == pytest.approx(z["occ_cover"].astype(np.float64).mean(), abs=1e-6)
    assert printed[-1].startswith("Corr(cover, uncertainty): ")
    corr = float(printed[-1].split(": ")[1])
    assert corr == pytest.approx(evaluate.cover_uncert_corr(z["occ_cover"], res["corr_y"]), abs=1e-6) and -1 <= corr <= 1
