"""The evaluator's side of the calibration on the GPU (poco_amd/calibrate.py): the 28 maps of calibrate.Fit
against tests/calib_np.py on the downloaded records, a fit applied to its own rows, the held-out scores against a numpy form, and
run_eval(calibrate=...) beside the plain run."""
import math

import numpy as np
import pytest
import torch

from poco_amd import calibrate, evaluate, ops, synth
from tests import calib_np, util
from tests.test_eval_rank_gpu import SEL, host_inputs, stepped

pytestmark = pytest.mark.gpu
U = 2.0 ** -52


def host_groups(rec, sel, rows=None):
    """[(key [n], ys [E,n])] of the 26 sorts from the downloaded records, as calibrate.groups_of hands them out on the device."""
    if rows is not None:
        rec = rec[rows]
    (k0, v0), (k1, v1) = host_inputs(rec, sel)
    unc, pose = rec[:, evaluate.R_UNC:evaluate.R_UNC + 24], rec[:, evaluate.R_POSE:evaluate.R_POSE + 24]
    return [(k0, v0), (k1, v1)] + [(unc[:, j].copy(), pose[:, j][None].copy()) for j in range(24)]


def host_maps(groups):
    """Per map (key in sorted order, y in sorted order, block, fit, knots, mag) by the restatement."""
    out = []
    for key, vals in groups:
        order = np.argsort(calib_np.canonical(key), kind="stable")
        for e in range(len(vals)):
            k, y = key[order], vals[e][order]
            out.append((k, y) + calib_np.isotonic_segment(k, y))
    return out


@pytest.fixture(scope="module")
def fitted(cuda):
    ev = stepped(cuda, [5, 3, 70], SEL, seed=33)
    rec = ev.finish(return_records=True)["records"]
    fit = calibrate.Fit(calibrate.groups_of(ev))
    yield ev, rec, fit
    ev.close()


def test_the_28_maps_are_the_restatements(fitted):
    ev, rec, fit = fitted
    maps = host_maps(host_groups(rec, SEL))
    assert len(maps) == 28 and fit.rows.tolist() == [len(m[0]) for m in maps] and not fit.dropped.any()
    assert fit.rows.tolist() == [78] * 3 + [78 * len(SEL)] + [78] * 24
    want_off = np.concatenate([[0], np.cumsum([len(m[4]) for m in maps])])
    assert np.array_equal(fit.offsets, want_off)
    dfit, dblock = fit.out["fit"].cpu().numpy(), fit.out["block"].cpu().numpy()
    for m, (k, y, block, val, knots, mag) in enumerate(maps):
        a, b = int(fit.seg[m]), int(fit.seg[m + 1])
        got = fit.knots[fit.offsets[m]:fit.offsets[m + 1]]
        assert np.array_equal(dblock[a:b] - a, block), m
        assert np.array_equal(got[:, [0, 1, 3]], knots[:, [0, 1, 3]]), m
        assert np.all(np.abs(dfit[a:b] - val) <= U * mag), m
    # a fit applied to its own training rows gives d_fit, rounded once
    key_pos = fit.key[fit.order.long()]
    for m in range(28):
        a, b = int(fit.seg[m]), int(fit.seg[m + 1])
        pred = ops.calib_apply(key_pos[a:b, None].contiguous(), torch.tensor([m], device=key_pos.device, dtype=torch.int32), fit.d_offsets,
                               fit.d_knots).cpu().numpy()[:, 0]
        assert np.array_equal(pred.view(np.uint32), dfit[a:b].astype(np.float32).view(np.uint32)), m


def test_non_finite_rows_are_dropped_and_counted(fitted):
    ev, rec, fit = fitted
    groups = calibrate.groups_of(ev)
    key, vals = groups[0]
    vals = vals.clone()
    vals[1, 4], vals[2, 9] = float("nan"), float("inf")
    key = key.clone()
    key[11] = float("inf")
    bad = calibrate.Fit([(key, vals)] + groups[1:])
    assert bad.rows.tolist()[:4] == [75, 75, 75, 78 * len(SEL)] and bad.dropped.tolist()[:4] == [3, 3, 3, 0]
    keep = np.ones(78, bool)
    keep[[4, 9, 11]] = False
    maps = host_maps(host_groups(rec[keep], SEL)[:1])
    for m in range(3):
        got = bad.knots[bad.offsets[m]:bad.offsets[m + 1]]
        assert np.array_equal(got[:, [0, 1, 3]], maps[m][4][:, [0, 1, 3]]), m


def numpy_scores(fit_groups, groups, bins):
    out = np.full((28, 3), np.nan)
    fmaps = host_maps(fit_groups)
    m = 0
    for (fkey, fvals), (key, vals) in zip(fit_groups, groups):
        for e in range(len(vals)):
            knots = fmaps[m][4]
            pred = np.asarray([calib_np.apply_map(knots, x) for x in key], np.float32)
            err = vals[e]
            order = np.argsort(pred, kind="stable")
            n = len(pred)
            ence = []
            for k in range(bins):
                c0, c1 = (k * n) // bins, ((k + 1) * n) // bins
                if c1 > c0:
                    mp = math.fsum(pred[order[c0:c1]].astype(np.float64)) / (c1 - c0)
                    me = math.fsum(err[order[c0:c1]].astype(np.float64)) / (c1 - c0)
                    ence.append(abs(mp - me) / mp)
            const = math.fsum(fvals[e].astype(np.float64)) / len(fvals[e])
            e64, p64 = err.astype(np.float64), pred.astype(np.float64)
            out[m] = (np.mean(ence), math.fsum(e64) / math.fsum(p64), 1.0 - math.fsum((e64 - p64) ** 2) / math.fsum((e64 - const) ** 2))
            m += 1
    return out


@pytest.mark.parametrize("split,bins", [("half", 5), ("parity", 20)])
def test_held_out_scores_match_numpy(fitted, split, bins):
    ev, rec, _ = fitted
    res = calibrate.calibrate(ev, split, bins, calibrate.make_meta("3dpw", True, "resnet50-cliff"))
    n = len(rec)
    a, b = (np.arange(n // 2), np.arange(n // 2, n)) if split == "half" else (np.arange(0, n, 2), np.arange(1, n, 2))
    ga, gb = host_groups(rec, SEL, a), host_groups(rec, SEL, b)
    want = 0.5 * (numpy_scores(ga, gb, bins) + numpy_scores(gb, ga, bins))
    got = res["calib_summary"]
    print("largest relative difference:", np.nanmax(np.abs(got - want) / np.maximum(np.abs(want), 1e-300)))
    assert got.shape == (28, 3) and np.array_equal(np.isnan(got), np.isnan(want)) and np.isfinite(got).all()
    assert np.all(np.abs(got - want) <= 1e-9 * np.maximum(np.abs(want), 1.0))      # sums of at most 468 float64 terms each
    assert set(res) == set(calibrate.NPZ_KEYS) and res["calib_knots"].shape == (res["calib_offsets"][-1], 4)
    none = calibrate.calibrate(ev, "none", bins)
    assert np.isnan(none["calib_summary"]).all() and np.array_equal(none["calib_knots"], res["calib_knots"])   # the table: all rows


def test_run_eval_with_and_without_calibrate(cuda, tmp_path):
    model = util.make_engine("resnet50-cliff", max_batch=16)
    n = 24
    r = np.random.default_rng(4)
    path = tmp_path / "ds.npz"
    np.savez(path, imgname=np.array([f"im{i}.png" for i in range(n)]), center=r.uniform(80, 200, (n, 2)).astype(np.float32),
             scale=r.uniform(0.5, 1.0, n).astype(np.float32), pose=(0.4 * r.standard_normal((n, 72))).astype(np.float32),
             shape=(0.5 * r.standard_normal((n, 10))).astype(np.float32), img=r.standard_normal((n, 3, 224, 224)).astype(np.float32),
             orig_shape=np.tile([[240.0, 320.0]], (n, 1)).astype(np.float32))
    ds = evaluate.EvalDataset(str(path), None, "3dpw")
    J = synth.synth_j_regressor_h36m(11)
    plain = evaluate.run_eval(model, ds, J, batch_size=16)
    spec = {"split": "half", "bins": 4, "meta": calibrate.make_meta("3dpw", True, "resnet50-cliff")}
    cal = evaluate.run_eval(model, ds, J, batch_size=16, calibrate=spec)
    assert set(cal) - set(plain) == {"calibration", "calib_summary"} and not set(plain) - set(cal)
    for k, v in plain.items():
        if isinstance(v, np.ndarray):
            assert np.array_equal(v, cal[k], equal_nan=v.dtype.kind == "f"), k
        else:
            assert v == cal[k] or (v != v and cal[k] != cal[k]), k
    evaluate.save_npz(str(tmp_path / "plain.npz"), plain, "3dpw")
    evaluate.save_npz(str(tmp_path / "cal.npz"), cal, "3dpw")
    zp, zc = dict(np.load(tmp_path / "plain.npz")), dict(np.load(tmp_path / "cal.npz"))
    assert set(zc) - set(zp) == {"calib_summary"} and zc["calib_summary"].shape == (28, 3)
    calibrate.save(str(tmp_path / "out.npz"), cal["calibration"])
    back = calibrate.load(str(tmp_path / "out.npz"))
    assert back["meta"]["head"] == "cliff" and back["meta"]["kinematic"] == "1" and back["meta"]["dataset"] == "3dpw"
    assert back["calib_rows"].tolist() == [n] * 3 + [n * 24] + [n] * 24
    assert len(calibrate.summary_lines(cal["calibration"])) == 29
