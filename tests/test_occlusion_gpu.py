"""GPU: the occlusion sensitivity sweep (poco_amd/occlusion.py, csrc/occlusion.hip) against its numpy restatement
(tests/occlusion_np.py): the three kernels on their own, OcclusionSweep end to end on the resnet50-cliff engine, and
demo.py --occlusion_map."""
import json

import numpy as np
import pytest
import torch

from poco_amd import occlusion, synth
from tests import occlusion_np as onp
from tests import util

pytestmark = pytest.mark.gpu

VARIANT = "resnet50-cliff"
GRIDS = ((96, 64, 9), (50, 70, 16), (1, 223, 4))          # (patch, stride, positions); 50 / 70 has x0 = 174: edges off the float4 grid


@pytest.fixture(scope="module")
def engine(cuda):
    return util.make_engine(VARIANT, max_batch=8)


def _records_close(got, want, what=""):
    """The kernel-B tolerances.  Columns 0:3 and 28:77 are sums / maxima / norms of positive terms: rtol 1e-5 (derived: a 13-level
    float32 tree over 6890 positive terms plus three roundings per term stays below 2e-6 relative).  Columns 3 and 4:28 are signed
    float32 differences and their mean: atol 1e-6 against the float64 value of the same float32 inputs."""
    got = np.asarray(got, np.float64)
    pos_cols = np.r_[0:3, 28:77]
    rel = np.abs(got[:, pos_cols] - want[:, pos_cols]) / np.maximum(np.abs(want[:, pos_cols]), 1e-300)
    rel = np.where(want[:, pos_cols] == 0, np.abs(got[:, pos_cols]), rel)
    ab = np.abs(got[:, 3:28] - want[:, 3:28])
    print(f"{what} records: worst relative error {rel.max():.2e} (bound 1e-5), worst signed-column error {ab.max():.2e} (bound 1e-6)")
    assert rel.max() <= 1e-5, (what, rel.max())
    assert ab.max() <= 1e-6, (what, ab.max())


@pytest.mark.parametrize("patch,stride,n", GRIDS)
def test_occlude_batch_bit_equal_with_guards(cuda, patch, stride, n):
    r = np.random.default_rng(patch)
    src = r.standard_normal((3, 224, 224)).astype(np.float32)
    pos = occlusion.sweep_positions(224, patch, stride)
    assert len(pos) == n
    fill = (0.25, -1.5, 3.0)
    G = 64                                                  # guard floats on either side (256 bytes: the output stays 16-byte aligned)
    size = n * 3 * 224 * 224
    raw = torch.full((G + size + G,), 0x7FC0DEAD, dtype=torch.int32, device=cuda)          # a NaN pattern
    out = raw.view(torch.float32)[G:G + size].view(n, 3, 224, 224)
    got = occlusion.occlude_batch(torch.from_numpy(src).to(cuda), pos, patch, fill, out=out)
    assert got.data_ptr() == out.data_ptr()
    torch.cuda.synchronize()
    host = raw.cpu().numpy()
    assert (host[:G] == 0x7FC0DEAD).all() and (host[G + size:] == 0x7FC0DEAD).all()
    want = onp.occlude_batch(src, pos, patch, fill)
    assert np.array_equal(host[G:G + size].view(np.float32).reshape(want.shape).view(np.uint32), want.view(np.uint32))
    # the default fill (the dataset mean colour) and a fresh output tensor
    got = occlusion.occlude_batch(torch.from_numpy(src).to(cuda), torch.from_numpy(pos).to(cuda), patch).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), onp.occlude_batch(src, pos, patch).view(np.uint32))


def test_occlusion_records_against_float64(cuda):
    r = np.random.default_rng(11)
    m = 5
    bv = r.standard_normal((6890, 3)).astype(np.float32)
    ba = r.uniform(0.05, 1.0, 24).astype(np.float32)
    bj = r.standard_normal((49, 3)).astype(np.float32)
    mag = np.float32([1e-4, 1e-3, 1e-2, 1e-1, 1.0])[:, None, None]                         # row differences spanning 1e-4 .. 1
    v = (bv[None] + mag * r.standard_normal((m, 6890, 3)).astype(np.float32)).astype(np.float32)
    j = (bj[None] + mag * r.standard_normal((m, 49, 3)).astype(np.float32)).astype(np.float32)
    va = np.abs(ba[None] + mag[:, :, 0] * r.standard_normal((m, 24)).astype(np.float32)).astype(np.float32)
    want = onp.occlusion_records(v, va, j, bv, ba, bj)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)                      # noqa: E731
    args = (t(v), t(va), t(j), t(bv), t(ba), t(bj))
    a = occlusion.occlusion_records(*args)
    b = occlusion.occlusion_records(*args)
    torch.cuda.synchronize()
    assert a.shape == (m, 77) and torch.equal(a.view(torch.int32), b.view(torch.int32))     # two calls: identical bits
    _records_close(a.cpu().numpy(), want, "random rows")
    # rows at an odd offset (8-byte, not 16-byte aligned: how OcclusionSweep passes the rows after the baseline) and identical rows
    c = occlusion.occlusion_records(args[0][1:], args[1][1:], args[2][1:], args[0][:1], args[1][:1], args[2][:1])
    _records_close(c.cpu().numpy(), onp.occlusion_records(v[1:], va[1:], j[1:], v[0], va[0], j[0]), "offset rows")
    z = occlusion.occlusion_records(args[0][:1], args[1][:1], args[2][:1], args[0][:1], args[1][:1], args[2][:1]).cpu().numpy()
    assert z[0, 2] == pytest.approx(va[0].astype(np.float64).mean(), rel=1e-6)
    z[0, 2] = 0
    assert not z.any()


@pytest.mark.parametrize("patch,stride,n", GRIDS[:2])
def test_heat_overlay_byte_equal(cuda, patch, stride, n):
    crop = onp.period_crop(224, 64, seed=5)
    pos = occlusion.sweep_positions(224, patch, stride)
    field = np.random.default_rng(n).uniform(0.0, 0.3, n).astype(np.float32)
    lut = occlusion.jet_lut_u8()
    cd, fd = torch.from_numpy(crop).to(cuda), torch.from_numpy(field).to(cuda)
    for scale in ("auto", float(field.max()) * 0.5):                                        # the fixed scale clips the upper half
        got = occlusion.heat_overlay(fd, pos, patch, cd, scale).cpu().numpy()
        want = onp.heat_overlay(field, pos, patch, crop, lut, scale)
        assert np.array_equal(got, want), (scale, np.argwhere(got != want)[:4])
        assert (got != crop).any()
    if stride > patch:                                                                      # pixels between the squares keep their bytes
        assert np.array_equal(got[60, 60], crop[60, 60])
    # a field without a positive maximum leaves the crop unchanged under "auto"; in place works
    same = occlusion.heat_overlay(torch.zeros_like(fd), pos, patch, cd, "auto")
    assert torch.equal(same, cd)
    buf = cd.clone()
    occlusion.heat_overlay(fd, pos, patch, buf, "auto", out=buf)
    assert np.array_equal(buf.cpu().numpy(), onp.heat_overlay(field, pos, patch, crop, lut, "auto"))


def test_sweep_end_to_end(cuda, engine):
    """patch 96 / stride 64 on one seeded crop: 1 + 9 rows = a full chunk of 8 and a short one of 2.  The records equal the
    restatement applied to the outputs of plain model(batch) calls on the numpy-occluded crops; the baseline is, bit for bit, the
    unoccluded crop's row of such a plain forward.  (A forward of the crop on its own runs other tile configurations than one of
    8 rows - equal to rounding, not bitwise, as tests/test_demo_gpu.py notes - so the comparison is with row 0 of the same chunk.)"""
    bnp = synth.synth_batch(1, 77)
    row = util.cuda_batch(bnp, cuda)
    fill = occlusion.fill_from_grey(128)
    sweep = occlusion.OcclusionSweep(engine, patch=96, stride=64, fill=fill)
    res = sweep.run(row)
    engine.check_status()
    assert res.records.shape == (9, 77) and res.grid == (3, 3) and res.records.is_cuda
    pos = res.positions.cpu().numpy()
    assert np.array_equal(pos, onp.sweep_positions(224, 96, 64))
    imgs = np.concatenate([bnp["img"], onp.occlude_batch(bnp["img"][0], pos, 96, fill)], 0)
    outs = []
    for lo, hi in ((0, 8), (8, 10)):
        b = {k: np.ascontiguousarray(np.repeat(v, hi - lo, 0)) for k, v in bnp.items() if k != "img"}
        b["img"] = np.ascontiguousarray(imgs[lo:hi])
        o = engine(util.cuda_batch(b, cuda), want_segm=False)
        outs.append({k: o[k].cpu().numpy() for k in occlusion.BASELINE_KEYS})
    engine.check_status(sync=True)
    for k in occlusion.BASELINE_KEYS:
        assert np.array_equal(res.baseline[k].cpu().numpy().view(np.uint32), outs[0][k][:1].view(np.uint32)), k
    cat = {k: np.concatenate([outs[0][k][1:], outs[1][k]], 0) for k in ("smpl_vertices", "var_pose", "smpl_joints3d")}
    want = onp.occlusion_records(cat["smpl_vertices"], cat["var_pose"], cat["smpl_joints3d"], outs[0]["smpl_vertices"][0],
                                 outs[0]["var_pose"][0], outs[0]["smpl_joints3d"][0])
    got = res.records.cpu().numpy()
    print("v2v per position:", np.array2string(got[:, 0], precision=5))
    assert (want[:, 0] > 0).all()                                   # the occluder does move the mesh
    _records_close(got, want, "sweep")
    again = sweep.run(row)
    assert torch.equal(again.records.view(torch.int32), res.records.view(torch.int32))


def test_demo_occlusion_map(tmp_path, cuda):
    from PIL import Image
    import demo
    from oracle.crop_np import crop_normalize_np
    w = util.synth_weights(VARIANT)
    ckpt = tmp_path / "poco_synth.pt"
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, ckpt)
    np.savez(tmp_path / "smpl.npz", **synth.synth_smpl(7))
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    r = np.random.default_rng(0)
    frames = {f"im{i}.png": r.integers(0, 256, (240, 320, 3), dtype=np.uint8) for i in range(2)}
    for n, f in frames.items():
        Image.fromarray(f).save(imgs / n)
    dets = {"im0.png": [[160, 120, 150, 150], [80, 100, 90, 120]], "im1.png": [[200, 100, 120, 160]]}
    (tmp_path / "dets.json").write_text(json.dumps(dets))
    base = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(ckpt), "--mode", "folder", "--image_folder", str(imgs),
            "--batch_size", "8", "--smpl", str(tmp_path / "smpl.npz"), "--detections", str(tmp_path / "dets.json"), "--no_render"]
    demo.main(demo.parse_args(base + ["--output_folder", str(tmp_path / "plain")]))
    demo.main(demo.parse_args(base + ["--output_folder", str(tmp_path / "occ"), "--occlusion_map", "--occ_patch", "96", "--occ_stride", "64"]))
    assert not (tmp_path / "plain" / "imgs_" / "occlusion").exists()
    lut = occlusion.jet_lut_u8()
    mean, std = np.float32(occlusion.MEAN).reshape(3, 1, 1), np.float32(occlusion.STD).reshape(3, 1, 1)
    for n, f in frames.items():
        # folder mode's ordinary results: the same arrays, bit for bit (the .npz container itself carries a time stamp per entry)
        a = dict(np.load(tmp_path / "plain" / "imgs_" / (n[:-4] + "_poco.npz")))
        b = dict(np.load(tmp_path / "occ" / "imgs_" / (n[:-4] + "_poco.npz")))
        assert set(a) == set(b)
        for k in a:
            assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (n, k)
        d = np.asarray(dets[n], np.float32)
        for i in range(len(d)):
            stem = tmp_path / "occ" / "imgs_" / "occlusion" / f"{n[:-4]}_{i}"
            z = dict(np.load(str(stem) + ".npz"))
            assert z["records"].shape == (3, 3, 77) and z["records"].dtype == np.float32
            assert np.array_equal(z["positions"], onp.sweep_positions(224, 96, 64)) and int(z["patch"]) == 96 and int(z["stride"]) == 64
            assert z["var_pose"].shape == (24,) and z["pred_cam"].shape == (3,)
            assert np.abs(z["pred_cam"] - a["pred_cam"][i]).max() < 1e-5            # the same crop in another batch: equal to rounding
            x = crop_normalize_np(f, d[i:i + 1])[0]
            canvas = np.clip(np.round((x * std + mean) * np.float32(255)), 0, 255).astype(np.uint8).transpose(1, 2, 0)
            want = onp.heat_overlay(onp.field_of(z["records"].reshape(9, 77), "v2v"), z["positions"], 96, canvas, lut, "auto")
            got = np.asarray(Image.open(str(stem) + ".png").convert("RGB"))
            assert got.shape == (224, 224, 3) and np.array_equal(got, want), (n, i)
    assert len(list((tmp_path / "occ" / "imgs_" / "occlusion").iterdir())) == 6
