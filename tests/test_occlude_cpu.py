"""CPU: the synthetic occluders of the dataset crop.  The numpy restatement tests/occlude_np.py and the host
code poco_amd/datacrop.py against the fixture the reference's own occlude_with_pascal_objects_kp made (tests/golden/occlude.npz,
tools/gen_occlude_golden.py: draws, centres, sizes, paste_over's clipping and blend); the restated INTER_AREA resize against results
derived on paper; paste_over's geometry; the two settled failure cases; the loader's and eval.py's refusals; the C entry."""
import ctypes as C
import importlib.util
import random
from pathlib import Path

import numpy as np
import pytest

from poco_amd import _lib, datacrop
from tests import occlude_cases, occlude_np

ROOT = Path(__file__).resolve().parent.parent
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def gold():
    z = np.load(ROOT / "tests" / "golden" / "occlude.npz")
    return {k: z[k] for k in z.files}


# ---- against the reference's own function ---------------------------------------------------------------------------------------------
def test_draws_centres_sizes_and_crops_equal_the_reference(gold):
    """Per fixture case: the restatement on the global generators and occlusion_params on generator objects make the reference's
    draws (count, cut-out, size, centre, and the generators end in the same state), and the pasted crop is the reference's bit for bit."""
    assert int(gold["resize_is_restated"]) == 1                                  # the resize inside the fixture is ours, not cv2's
    cuts = [gold[f"cutout_{i}"] for i in range(int(gold["n_cutouts"]))]
    hw = [c.shape[:2] for c in cuts]
    seen_counts, one_visible, on_border = set(), False, False
    for ci, (ki, res, scale, seed) in enumerate(gold["cases"]):
        res, seed, kp = int(res), int(seed), gold[f"kp_{int(ki)}"][25:]
        calls, pastes = gold[f"calls_{ci}"], gold[f"pastes_{ci}"]
        want = [(hw.index((int(c[0]), int(c[1]))), int(c[2]), int(c[3]), int(p[0]), int(p[1])) for c, p in zip(calls, pastes)]
        assert all(tuple(p[2:]) == tuple(c[2:4]) for c, p in zip(calls, pastes))   # what was pasted has the size that was asked for
        np.random.seed(seed)
        random.seed(seed)
        d = occlude_np.occlusion_draws_np(kp, np.float64(scale), hw, res)
        assert d["objects"] == want and d["count"] == len(want) and d["skipped"] == 0 and not d["no_visible"]
        assert np.array_equal([np.random.uniform(), random.random()], gold[f"next_{ci}"])
        np_rng, py_rng = np.random.RandomState(seed), random.Random(seed)
        h = datacrop.occlusion_params(np_rng, py_rng, kp, np.float64(scale), hw, res)
        assert h["objects"] == want and h["count"] == len(want)
        assert np.array_equal([np_rng.uniform(), py_rng.random()], gold[f"next_{ci}"])
        out, touched = occlude_np.apply_objects_np(gold[f"crop_{ci}"], cuts, want)
        assert np.array_equal(bits(out), bits(gold[f"out_{ci}"])), ci
        assert np.array_equal(gold[f"crop_{ci}"], occlude_np.synthetic_crop(res, ci))
        changed = (bits(out) != bits(gold[f"crop_{ci}"])).any(axis=2)
        assert changed.any() and not (changed & ~touched).any()                   # only touched pixels change
        seen_counts.add(len(want))
        one_visible |= int((kp[:, 2] > 0.3).sum()) == 1
        on_border |= any(c in (0, res) for o in want for c in o[3:])
    assert len(seen_counts) >= 3 and one_visible and on_border                    # the fixture holds the cases it was made for


# ---- the restated resize, derived on paper ---------------------------------------------------------------------------------------------
def _rgba(rows):
    """A [h, w] array of byte values as a 4-channel image (every channel the same)."""
    a = np.asarray(rows, np.uint8)
    return np.repeat(a[:, :, None], 4, axis=2)


def test_resize_three_to_two():
    """[a, b, c] -> 2 pixels: weights (2/3, 1/3) on (a, b) and (1/3, 2/3) on (b, c), in float32, one row (y weight 1)."""
    tab = occlude_np.area_tab(3, 2)
    assert [[s for s, _ in e] for e in tab] == [[0, 1], [1, 2]]
    w = [[float(a) for _, a in e] for e in tab]
    assert w == [[float(F32(1 / 1.5)), float(F32(0.5 / 1.5))], [float(F32(0.5 / 1.5)), float(F32(1 / 1.5))]]
    a, b, c = 10, 200, 77
    got = occlude_np.resize_area(_rgba([[a, b, c]]), (2, 1))[0, :, 0]
    t, u = F32(2 / 3), F32(1 / 3)
    want = [np.rint(F32(a) * t + F32(b) * u), np.rint(F32(b) * u + F32(c) * t)]
    assert got.tolist() == want == [73, 118]                                      # 73.33.., 118.0
    assert occlude_np.resize_path((1, 3), (2, 1)) == "generic"                    # one axis 1.5, the other 1: not the fast path


def test_resize_constant_stays_constant_and_weights_sum_to_one():
    for (h, w), (dw, dh) in (((40, 23), (11, 19)), ((64, 48), (20, 26)), ((16, 16), (8, 5)), ((9, 12), (4, 3)), ((5, 7), (7, 5)), ((64, 48), (1, 1))):
        for v in (0, 1, 129, 255):
            assert (occlude_np.resize_area(np.full((h, w, 4), v, np.uint8), (dw, dh)) == v).all(), ((h, w), (dw, dh), v)
    for s, d in ((3, 2), (23, 11), (40, 19), (48, 20), (64, 26), (16, 5), (4096, 7), (7, 7), (7, 1)):
        for ent in occlude_np.area_tab(s, d):
            ws = np.asarray([a for _, a in ent], np.float64)
            assert all(0 <= i < s for i, _ in ent) and (ws > 0).all()
            assert abs(ws.sum() - 1) <= (len(ws) + 1) * 2.0 ** -24, (s, d, ws.sum())   # each weight is one float32 rounding off


def test_resize_fast_paths_copy_and_mixed_axis():
    # 2 x 2 blocks: (s + 2) >> 2 rounds half up.  Both sums have s % 4 == 2: s = 6 -> 1.5 -> 2 either way; s = 10 -> 2.5 -> 3, where
    # half-to-even would give 2.
    img = _rgba([[1, 2, 3, 4], [3, 0, 2, 1]])                                      # sums 6 and 10
    assert occlude_np.resize_path((2, 4), (2, 1)) == "fast"
    assert occlude_np.resize_area(img, (2, 1))[0, :, 1].tolist() == [2, 3]         # half-even would give [2, 2]
    # 3 x 3 blocks: round-half-even of float32(s) * float32(1.f / 9)
    blk = np.arange(27, dtype=np.uint8).reshape(3, 9) * 9
    s = np.asarray([blk[:, 3 * k:3 * k + 3].astype(np.int64).sum() for k in range(3)])
    want = np.rint(s.astype(F32) * (F32(1) / F32(9)))
    assert occlude_np.resize_path((3, 9), (3, 1)) == "fast"
    assert occlude_np.resize_area(_rgba(blk), (3, 1))[0, :, 2].tolist() == want.tolist() == [90, 117, 144]
    # 3 x 3 sums on either side of one half (a tie cannot occur: 2 s / 9 is never an odd integer)
    one = np.zeros((3, 3), np.uint8)
    one[0, 0] = 5                                                                 # 5 / 9 = 0.55.. -> 1
    assert occlude_np.resize_area(_rgba(one), (1, 1))[0, 0, 0] == 1
    one[0, 0] = 4                                                                 # 0.44.. -> 0
    assert occlude_np.resize_area(_rgba(one), (1, 1))[0, 0, 0] == 0
    # dsize == ssize copies
    r = np.random.default_rng(1)
    a = r.integers(0, 256, (5, 7, 4), dtype=np.uint8)
    got = occlude_np.resize_area(a, (7, 5))
    assert occlude_np.resize_path((5, 7), (7, 5)) == "copy" and np.array_equal(got, a) and got is not a
    # one axis integer (2), the other not (3.2): the generic path, whose x weights are then exactly 1/2
    assert occlude_np.resize_path((16, 16), (8, 5)) == "generic" and occlude_np.resize_path((16, 16), (8, 8)) == "fast"
    b = r.integers(0, 256, (16, 16, 4), dtype=np.uint8)
    got = occlude_np.resize_area(b, (8, 5))
    ytab = occlude_np.area_tab(16, 5)
    buf = (b[:, 0::2].astype(F32) * F32(0.5) + b[:, 1::2].astype(F32) * F32(0.5))
    want = np.zeros((5, 8, 4), F32)
    for dy, ent in enumerate(ytab):
        for k, (sy, beta) in enumerate(ent):
            want[dy] = beta * buf[sy] if k == 0 else want[dy] + beta * buf[sy]
    assert np.array_equal(got, np.rint(want).astype(np.uint8))
    # every named case of the shared catalogue takes the path it is there for
    for name, path in occlude_cases.PATHS.items():
        (oid, dw, dh, _, _), = occlude_cases.geometry(32)[name]
        assert occlude_np.resize_path(occlude_cases.SIZES[oid], (dw, dh)) == path, name
    for bad in ((8, 4), (3, 17), (0, 3), (3, 0)):
        with pytest.raises(ValueError):
            occlude_np.resize_area(b[:4, :4].copy() if bad[0] else b, bad)


# ---- paste_over ----------------------------------------------------------------------------------------------------------------------
def test_paste_over_geometry():
    """Where the rectangle lands: start = centre - size // 2 per axis, clipped to the crop; the source is cut by the same amount."""
    res = 32
    for (h, w) in ((4, 6), (5, 7)):                                               # even and odd sizes
        src = np.zeros((h, w, 4), np.uint8)
        src[..., 0] = np.arange(w)[None, :] + 1                                   # R = source column + 1
        src[..., 1] = np.arange(h)[:, None] + 1                                   # G = source row + 1
        src[..., 3] = 255
        for cx, cy, what in ((16, 16, "inside"), (1, 16, "left"), (31, 16, "right"), (16, 0, "top"), (16, 32, "bottom"), (32, 32, "corner"),
                             (-20, 16, "outside"), (16, 80, "outside")):
            dst = np.full((res, res, 3), 99, F32)
            touched = occlude_np.paste_over_np(src, dst, np.array([cx, cy]))
            x0, y0 = cx - w // 2, cy - h // 2
            want = np.full((res, res, 3), 99, F32)
            mask = np.zeros((res, res), bool)
            for y in range(max(y0, 0), min(y0 + h, res)):
                for x in range(max(x0, 0), min(x0 + w, res)):
                    want[y, x] = (x - x0 + 1, y - y0 + 1, 0)
                    mask[y, x] = True
            assert np.array_equal(dst, want) and np.array_equal(touched, mask), (h, w, cx, cy, what)
            assert (what == "outside") == (not mask.any()) and (what == "inside") == (int(mask.sum()) == h * w)


def test_paste_over_alpha():
    """alpha 0 leaves the pixel's bits alone apart from -0 (0 * colour + 1 * dst = +0 + dst); alpha 255 gives the colour exactly;
    alpha 192 is the two-product float32 blend."""
    r = np.random.default_rng(5)
    dst0 = r.uniform(0, 255, (8, 8, 3)).astype(F32)
    dst0[0, 0] = (-0.0, 0.0, 3.5)
    for a in (0, 192, 255):
        src = r.integers(0, 256, (8, 8, 4), dtype=np.uint8)
        src[..., 3] = a
        dst = dst0.copy()
        touched = occlude_np.paste_over_np(src, dst, np.array([4, 4]))
        assert touched.all() == (a > 0) and touched.any() == (a > 0)
        if a == 0:
            assert np.array_equal(bits(dst).reshape(-1)[1:], bits(dst0).reshape(-1)[1:]) and bits(dst)[0, 0, 0] == 0   # -0 became +0
        elif a == 255:
            assert np.array_equal(dst, src[..., :3].astype(F32))
        else:
            al = F32(192) / F32(255)
            assert np.array_equal(bits(dst), bits(al * src[..., :3].astype(F32) + (F32(1) - al) * dst0))
            assert not np.array_equal(dst, dst0)


def test_objects_apply_in_drawn_order():
    cuts = occlude_cases.cutouts()
    g = occlude_cases.geometry(32)
    crop = occlude_np.synthetic_crop(32, 0)
    ab, _ = occlude_np.apply_objects_np(crop, cuts, g["overlap_ab"])
    ba, _ = occlude_np.apply_objects_np(crop, cuts, g["overlap_ba"])
    assert not np.array_equal(ab, ba)
    none, touched = occlude_np.apply_objects_np(crop, cuts, g["outside"] + g["outside_far"])
    assert np.array_equal(bits(none), bits(crop)) and not touched.any()


# ---- the two cases in which the reference raises --------------------------------------------------------------------------------------
def test_no_visible_keypoint_leaves_the_sample_unoccluded_after_its_count_draw():
    kp = np.zeros((24, 3), F32)
    kp[:, 2] = 0.3                                                                # "> 0.3" is strict
    a, b = np.random.RandomState(4), random.Random(4)
    d = datacrop.occlusion_params(a, b, kp, 1.0, [(16, 16)], 224)
    assert d["no_visible"] and d["objects"] == [] and 1 <= d["count"] <= 7 and d["skipped"] == 0
    ref = np.random.RandomState(4)
    assert ref.randint(1, 8) == d["count"] and a.uniform() == ref.uniform()       # exactly one numpy draw was made
    assert b.random() == random.Random(4).random()                                # and none from Python's generator
    np.random.seed(4)
    assert occlude_np.occlusion_draws_np(kp, 1.0, [(16, 16)], 224) == d


def test_zero_sided_new_size_skips_the_object_after_its_draws():
    """res 32: the factor is 0.025 .. 0.125 (+ 1e-8), so a 3 x 3 cut-out always rounds to 0 and a 16 x 16 one never does."""
    kp = np.zeros((24, 3), F32)
    kp[:, 2] = 1
    hw = [(3, 3), (16, 16)]
    a, b = np.random.RandomState(9), random.Random(9)
    d = datacrop.occlusion_params(a, b, kp, 1.0, hw, 32)
    pr = random.Random(9)
    ids = [pr.choice(range(2)) for _ in range(d["count"])]
    assert d["skipped"] == ids.count(0) > 0 and [o[0] for o in d["objects"]] == [1] * ids.count(1) and not d["no_visible"]
    # the skipped objects made all their draws: the generators are where count * (choice, 2 randn, uniform) leaves them
    ref = np.random.RandomState(9)
    ref.randint(1, 8)
    for _ in range(d["count"]):
        ref.choice(range(24), 1), ref.randn(), ref.randn(), ref.uniform(0.2, 1.0)
    assert a.uniform() == ref.uniform() and b.random() == pr.random()
    np.random.seed(9)
    random.seed(9)
    assert occlude_np.occlusion_draws_np(kp, 1.0, hw, 32) == d
    with pytest.raises(ValueError, match="res"):
        datacrop.occlusion_params(a, b, kp, 1.0, hw, 257)


def test_spec_draws_augmentation_first_then_occlusion_per_sample():
    """OcclusionSpec.draw: ONE RandomState for both, per sample augm_params then the occlusion draws (BaseDataset.__getitem__); the
    keypoints are j2d_processing's with the sample's sc * scale, rot and flip."""
    from tests import datacrop_np
    r = np.random.default_rng(3)
    cuts = occlude_cases.cutouts()
    n = 5
    part = np.concatenate([r.uniform(20, 200, (n, 24, 2)), r.choice([0.0, 1.0], (n, 24, 1), p=[0.2, 0.8])], 2)
    center, scale = r.uniform(80, 140, (n, 2)).astype(F32), r.uniform(0.5, 1.2, n).astype(F32)
    cfg = dict(FLIP=1, NOISE_FACTOR=0.4, ROT_FACTOR=30, SCALE_FACTOR=0.25)
    spec = datacrop.OcclusionSpec(cuts, seed=11)
    (flip, pn, rot, sc), d = spec.draw(datacrop.AugSpec(random=True, seed=11, cfg=cfg), part, center, scale, 224)
    np.random.seed(11)
    random.seed(11)
    for i in range(n):
        f, p, ro, s = datacrop_np.augm_params_np(cfg, True)
        assert (f, ro, s) == (flip[i], rot[i], sc[i]) and np.array_equal(p, pn[i])
        kp = datacrop_np.j2d_processing_np(part[i], center[i], float(s * np.float64(scale[i])), ro, f, 224)
        assert occlude_np.occlusion_draws_np(kp, s * np.float64(scale[i]), spec.sizes, 224)["objects"] == d["objects"][i]
    assert d["count"].tolist() == [len(o) for o in d["objects"]] and d["count"].min() >= 1
    # a fixed AugSpec draws nothing: the occlusion draws start the sequence
    (flip, pn, rot, sc), d2 = spec.draw(datacrop.AugSpec(rot=30.0, flip=True), part, center, scale, 224)
    np.random.seed(11)
    random.seed(11)
    kp = datacrop_np.j2d_processing_np(part[0], center[0], float(np.float64(scale[0])), 30.0, 1, 224)
    assert occlude_np.occlusion_draws_np(kp, np.float64(scale[0]), spec.sizes, 224)["objects"] == d2["objects"][0]
    assert rot.tolist() == [30.0] * n and flip.tolist() == [1] * n
    with pytest.raises(ValueError, match="seeds differ"):
        spec.draw(datacrop.AugSpec(random=True, seed=12, cfg=cfg), part, center, scale, 224)
    rec = datacrop.occ_records(d["objects"])
    assert rec.dtype.itemsize == 144 and rec["count"].tolist() == d["count"].tolist()
    assert tuple(rec["obj"][2, 0].tolist()) == d["objects"][2][0]
    with pytest.raises(ValueError, match="at most 7"):
        datacrop.occ_records([[(0, 1, 1, 0, 0)] * 8])


# ---- the loader and eval.py ----------------------------------------------------------------------------------------------------------
def test_load_occluders(tmp_path):
    import joblib
    cuts = occlude_cases.cutouts()
    joblib.dump(cuts, tmp_path / "pascal_occluders.pkl")
    got = datacrop.load_occluders(str(tmp_path / "pascal_occluders.pkl"))
    assert len(got) == len(cuts) and all(np.array_equal(a, b) for a, b in zip(got, cuts))
    np.savez(tmp_path / "o.npz", b=cuts[1], a=cuts[0], c=cuts[2])
    got = datacrop.load_occluders(str(tmp_path / "o.npz"))
    assert [a.shape for a in got] == [cuts[0].shape, cuts[1].shape, cuts[2].shape]        # sorted key order
    np.savez(tmp_path / "rgb.npz", a=cuts[0], bad=cuts[1][..., :3])
    joblib.dump([cuts[0], cuts[1].astype(np.float32)], tmp_path / "f32.pkl")
    joblib.dump({"stats": 1}, tmp_path / "dict.pkl")
    joblib.dump([], tmp_path / "empty.pkl")
    (tmp_path / "junk.pkl").write_bytes(b"not a pickle")
    for name, word in (("rgb.npz", "'bad'"), ("f32.pkl", "entry 1"), ("dict.pkl", "list"), ("empty.pkl", "no cut-out"), ("junk.pkl", "joblib"),
                       ("missing.pkl", "not found")):
        with pytest.raises(ValueError, match=word):
            datacrop.load_occluders(str(tmp_path / name))


def _cli():
    spec = importlib.util.spec_from_file_location("poco_eval_cli", ROOT / "eval.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_eval_flag_and_refusals(tmp_path):
    cli = _cli()
    base = dict(imgname=np.array(["a.png", "b.png"]), center=np.full((2, 2), 100, np.float32), scale=np.ones(2, np.float32),
                pose=np.zeros((2, 72), np.float32), shape=np.zeros((2, 10), np.float32))
    part = np.concatenate([np.full((2, 24, 2), 100.0), np.ones((2, 24, 1))], 2)
    np.savez(tmp_path / "nopart.npz", **base)
    np.savez(tmp_path / "part.npz", part=part, **base)
    np.savez(tmp_path / "img.npz", img=np.zeros((2, 3, 224, 224), np.float32), part=part, **base)
    np.savez(tmp_path / "occ.npz", **{f"c{i}": c for i, c in enumerate(occlude_cases.cutouts())})
    np.savez(tmp_path / "bad.npz", a=np.zeros((4, 4, 3), np.uint8))
    (tmp_path / "imgs").mkdir()
    common = ["--cfg", "configs/demo_poco_cliff.yaml", "--ckpt", "none.pt", "--j_regressor", "none.npy", "--img_dir", str(tmp_path / "imgs")]

    def specs(ds, *extra):
        args = cli.parse_args(common + ["--dataset", str(tmp_path / ds)] + list(extra))
        return args, cli.augmentation_spec(args), cli.occlusion_spec(args)

    args, aug, occ = specs("part.npz")
    assert args.crop == "demo" and aug is None and occ is None                           # nothing changes without the flag
    args, aug, occ = specs("part.npz", "--aug_occlude", str(tmp_path / "occ.npz"), "--aug_seed", "5")
    assert args.crop == "dataset" and not aug.random and occ.seed == 5 and len(occ.occluders) == 5 and "5 cut-outs" in occ.describe()
    args, aug, occ = specs("part.npz", "--aug_occlude", str(tmp_path / "occ.npz"), "--augment", "--aug_seed", "5")
    assert aug.random and aug.seed == occ.seed == 5                                      # composes with --augment: one seed
    args, aug, occ = specs("part.npz", "--aug_occlude", str(tmp_path / "occ.npz"), "--aug_rot", "30", "--aug_flip")
    assert (aug.rot, aug.flip) == (30.0, True) and occ is not None
    for ds, path, word in (("nopart.npz", "occ.npz", "`part`"), ("img.npz", "occ.npz", "`img`"), ("part.npz", "bad.npz", "'a'"),
                           ("part.npz", "nothing.pkl", "not found")):
        with pytest.raises(SystemExit) as e:
            specs(ds, "--aug_occlude", str(tmp_path / path))
        assert word in str(e.value.code) and "--aug_occlude" in str(e.value.code), (ds, path, e.value.code)
    # main() refuses before the checkpoint, the regressor or the GPU are looked at
    with pytest.raises(SystemExit) as e:
        cli.main(cli.parse_args(common + ["--dataset", str(tmp_path / "nopart.npz"), "--aug_occlude", str(tmp_path / "occ.npz")]))
    assert "`part`" in str(e.value.code)
    from poco_amd import evaluate
    spec = datacrop.OcclusionSpec(occlude_cases.cutouts(), seed=1)
    with pytest.raises(ValueError, match="`part`"):
        evaluate.EvalDataset(str(tmp_path / "nopart.npz"), str(tmp_path / "imgs"), crop="dataset", occlude=spec)
    with pytest.raises(ValueError, match="`img`"):
        evaluate.EvalDataset(str(tmp_path / "img.npz"), None, crop="dataset", occlude=spec)
    with pytest.raises(ValueError, match="crop='dataset'"):
        evaluate.EvalDataset(str(tmp_path / "part.npz"), str(tmp_path / "imgs"), occlude=spec)
    ds = evaluate.EvalDataset(str(tmp_path / "part.npz"), str(tmp_path / "imgs"), crop="dataset", occlude=spec)
    assert ds.occ_count.tolist() == ds.occ_records["count"].tolist() and (ds.occ_count >= 1).all() and ds.occ_no_visible == 0
    assert np.isnan(ds.occ_cover).all()                                                  # no batch was made yet
    plain = evaluate.EvalDataset(str(tmp_path / "part.npz"), str(tmp_path / "imgs"), crop="dataset")
    assert not hasattr(plain, "occ_count") and plain.occlude is None
    assert evaluate.cover_uncert_corr([0.0, 0.5, 1.0], np.asarray([[1, 3], [2, 4], [3, 5]], np.float32).reshape(-1)) == pytest.approx(1.0)
    assert evaluate.cover_uncert_corr([0.0, 0.5, 1.0, 0.2], [4, 2, 0, 3.2]) == pytest.approx(-1.0)
    assert np.isnan(evaluate.cover_uncert_corr([0.3, 0.3], [1, 2]))


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------
def test_symbol_is_declared_and_exported():
    assert "poco_dataset_crop_occ" in _lib.header_symbols() and hasattr(_lib.lib(), "poco_dataset_crop_occ")
    assert datacrop.OCC_DTYPE.itemsize == 144 and datacrop.OCC_DTYPE["obj"].subdtype[0].itemsize == 20


def occ_call_args(good_params, table, recs):
    """Keyword arguments of a poco_dataset_crop_occ call on fake device pointers (never dereferenced: every call is refused first)."""
    FAKE = C.c_void_p(4096)
    return dict(images=FAKE, hw=FAKE, n_images=2, d_params=FAKE, h=good_params, N=len(good_params), res=32, atlas=FAKE, texels=int(
        (table["h"] * table["w"]).sum()), d_table=FAKE, h_table=table, d_occ=FAKE, h_occ=recs, out=FAKE, cover=FAKE)


def occ_call(L, kw):
    p = lambda a: C.c_void_p(0) if a is None else (a if isinstance(a, C.c_void_p) else C.c_void_p(a.ctypes.data))   # noqa: E731
    return L.poco_dataset_crop_occ(kw["images"], kw["hw"], kw["n_images"], kw["d_params"], p(kw["h"]), kw["N"], kw["res"], 1, kw["atlas"],
                                   kw["texels"], kw["d_table"], p(kw["h_table"]), len(kw["h_table"]) if kw.get("n_occ") is None else kw["n_occ"],
                                   kw["d_occ"], p(kw["h_occ"]), kw["out"], kw["cover"], C.c_void_p(0))


def bad_occ_calls(good_params, table, recs):
    """Every argument error of poco_dataset_crop_occ as (label, changed keyword arguments)."""
    NULL = C.c_void_p(0)

    def rec(**ch):
        r = recs.copy()
        for k, v in ch.items():
            if k == "count":
                r["count"][1] = v
            else:
                r["obj"][k][1, 0] = v
        return r

    def tab(**ch):
        t = table.copy()
        for k, v in ch.items():
            t[k][1] = v
        return t

    nan = good_params.copy()
    nan["src"][0, 0] = np.nan
    return [("images", dict(images=NULL)), ("hw", dict(hw=NULL)), ("d_params", dict(d_params=NULL)), ("h_params", dict(h=None)), ("out", dict(out=NULL)),
            ("atlas", dict(atlas=NULL)), ("atlas alignment", dict(atlas=C.c_void_p(4098))), ("d_table", dict(d_table=NULL)),
            ("h_table", dict(h_table=None, n_occ=len(table))), ("d_occ", dict(d_occ=NULL)), ("h_occ", dict(h_occ=None)), ("N", dict(N=0)),
            ("res 257", dict(res=257)), ("res 0", dict(res=0)), ("n_occ", dict(n_occ=0)), ("texels", dict(texels=0)), ("nan", dict(h=nan)),
            ("count 8", dict(h_occ=rec(count=8))), ("count -1", dict(h_occ=rec(count=-1))), ("id", dict(h_occ=rec(id=len(table)))),
            ("id -1", dict(h_occ=rec(id=-1))), ("dst_w 0", dict(h_occ=rec(dst_w=0))), ("dst_h 0", dict(h_occ=rec(dst_h=0))),
            ("dst_w > w", dict(h_occ=rec(id=1, dst_w=17))), ("dst_h > h", dict(h_occ=rec(id=1, dst_h=17))), ("side 0", dict(h_table=tab(h=0))),
            ("side 4097", dict(h_table=tab(w=4097))), ("outside the atlas", dict(h_table=tab(offset=10 ** 6)))]


def good_occ_inputs():
    cuts = occlude_cases.cutouts()
    params = datacrop.batch_params([(40, 30)] * 3, [0.2] * 3, [30.0] * 3, [0] * 3, [(1, 1, 1)] * 3, [1.0] * 3, 32)
    table = np.zeros(len(cuts), datacrop.OCCLUDER_DTYPE)
    off = 0
    for i, c in enumerate(cuts):
        table[i] = (off, c.shape[0], c.shape[1])
        off += c.shape[0] * c.shape[1]
    g = occlude_cases.geometry(32)
    recs = datacrop.occ_records([g["seven"], g["inside_fast_2x2"], g["none"]])
    return cuts, params, table, recs


def test_argument_errors_without_a_gpu():
    """Refused before any GPU work: the fake device pointers are never dereferenced."""
    L = datacrop._bind_occ()
    _, params, table, recs = good_occ_inputs()
    base = occ_call_args(params, table, recs)
    for label, ch in bad_occ_calls(params, table, recs):
        assert occ_call(L, dict(base, **ch)) == 1, label
        assert "poco_dataset_crop_occ" in L.poco_last_error().decode(), label
