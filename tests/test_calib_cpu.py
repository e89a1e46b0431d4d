"""The calibration operators without a GPU: the yardstick tests/calib_np.py against an exact brute force and against scipy, the map f,
the C ABI's declarations and argument checks, ops' refusals, and the decision margins of every seeded float input that
tests/test_calib_gpu.py demands the exact partition of (include/poco_hip.h poco_op_isotonic / poco_op_calib_apply, DESIGN.md
section 33)."""
import math

import numpy as np
import pytest

from poco_amd import _lib
from tests import calib_np

U = 2.0 ** -52
MARGIN = 1e-9                                                             # the margin tests/test_sort_cpu.py uses


# ---- the yardstick ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", range(0, 13))
def test_yardstick_is_the_exact_fit(n):
    for seed in range(12):
        r = np.random.default_rng([n, seed])
        key = np.sort(r.integers(0, 2 + seed % 7, n)).astype(np.float32) * np.float32(0.5)
        if n and seed % 3 == 0:
            key[key == 0] = -0.0                                          # one unit with +0.0
        y = (r.integers(0, 6, n) if seed % 2 else np.round(r.standard_normal(n), 3)).astype(np.float32)
        assert calib_np.pava(key, y) == calib_np.exact_fit(key, y), (n, seed)


def test_yardstick_on_hand_made_cases():
    k = np.asarray([1, 2, 3, 4], np.float32)
    assert calib_np.pava(k, np.asarray([1, 3, 2, 4], np.float32)) == [(0, 1), (1, 2), (3, 1)]
    assert calib_np.pava(k, np.asarray([1, 1, 1, 1], np.float32)) == [(0, 4)]                      # an exact tie pools
    assert calib_np.pava(k, np.asarray([4, 3, 2, 1], np.float32)) == [(0, 4)]
    assert calib_np.pava(np.asarray([1, 1, 2, 2], np.float32), np.asarray([0, 9, 1, 2], np.float32)) == [(0, 4)]   # 4.5 >= 1.5
    assert calib_np.pava(np.asarray([-0.0, 0.0, 1], np.float32), np.asarray([5, 1, 4], np.float32)) == [(0, 2), (2, 1)]
    blk, fit, kn, mag = calib_np.isotonic_segment(k, np.asarray([1, 3, 2, 4], np.float32))
    assert blk.tolist() == [0, 1, 1, 3] and fit.tolist() == [1, 2.5, 2.5, 4] and mag.tolist() == [1, 5, 5, 4]
    assert kn.tolist() == [[1, 1, 1, 1], [2, 3, 2.5, 2], [4, 4, 4, 1]]


def test_yardstick_against_scipy():
    opt = pytest.importorskip("scipy.optimize")
    if not hasattr(opt, "isotonic_regression"):
        pytest.skip("this scipy has no isotonic_regression")
    for seed in range(6):
        r = np.random.default_rng(seed)
        n = 400
        key = np.sort(np.round(r.gamma(2.0, 0.1, n), 2)).astype(np.float32)                          # many ties
        y = ((1.0 + key) * r.gamma(2.0, 0.5, n)).astype(np.float32)
        blk, fit, kn, _ = calib_np.isotonic_segment(key, y)
        units = calib_np.units_of(key)
        means = np.asarray([math.fsum(float(t) for t in y[s:s + c]) / c for s, c in units])
        res = opt.isotonic_regression(means, weights=np.asarray([c for _, c in units], np.float64))
        want = np.repeat(res.x, [c for _, c in units])
        assert np.max(np.abs(fit - want)) <= 1e-12 * np.max(np.abs(want))
        assert len(kn) == len(res.blocks) - 1


@pytest.mark.parametrize("name", calib_np.PATTERNS)
def test_the_fit_keeps_the_sum_and_is_monotone(name):
    key, y = calib_np.pattern(name, 777, 64)
    res = calib_np.isotonic(key, y, np.arange(777), [0, 777])
    yd = y.astype(np.float64)
    assert abs(math.fsum(res["fit"]) - math.fsum(yd)) <= U * math.fsum(np.abs(yd))
    assert np.all(np.diff(res["fit"]) >= 0) and np.all(np.diff(res["knots"][:, 2]) > 0)
    assert np.all(res["knots"][:-1, 1] < res["knots"][1:, 0]) and res["knots"][:, 3].sum() == 777


# ---- the map ------------------------------------------------------------------------------------------------------------------------
KN = np.asarray([[0.5, 0.5, 1.0, 3], [1.0, 2.0, 4.0, 7], [3.0, 3.0, 4.5, 1]], np.float64)


def test_map_values_by_hand():
    f = lambda x: float(calib_np.apply_map(KN, x))                        # noqa: E731
    assert [f(-1), f(0.5), f(0.75), f(1.0), f(1.5), f(2.0), f(2.5), f(3.0), f(9), f(np.inf), f(-np.inf)] == \
        [1.0, 1.0, 2.5, 4.0, 4.0, 4.0, 4.25, 4.5, 4.5, 4.5, 1.0]
    assert np.isnan(calib_np.apply_map(KN, np.nan)) and np.isnan(calib_np.apply_map(KN[:0], 1.0))
    assert f(-0.0) == 1.0 and float(calib_np.apply_map(KN[:1], 7.0)) == 1.0


def test_map_is_monotone_and_matches_numpy_interp():
    r = np.random.default_rng(3)
    key = np.sort(r.gamma(2.0, 0.1, 500)).astype(np.float32)
    y = ((1.0 + key) * r.gamma(2.0, 0.5, 500)).astype(np.float32)
    kn = calib_np.isotonic_segment(key, y)[2]
    x = np.sort(np.concatenate([r.uniform(-0.1, 2.0, 3000).astype(np.float32), key, kn[:, 0].astype(np.float32), kn[:, 1].astype(np.float32)]))
    got = np.asarray([calib_np.apply_map(kn, v) for v in x])
    assert np.all(np.diff(got) >= 0)
    want = np.interp(x.astype(np.float64), kn[:, :2].reshape(-1), np.repeat(kn[:, 2], 2))
    assert np.all(np.abs(got - want) <= 2.0 ** -23 * np.abs(want))
    out = calib_np.calib_apply(x[:10].reshape(5, 2), [1, 0], [0, 0, len(kn)], kn)
    assert np.array_equal(out[:, 0], got[:10:2]) and np.all(np.isnan(out[:, 1]))


# ---- the decision margins of the GPU test's float inputs ------------------------------------------------------------------------------
def test_float_inputs_of_the_gpu_test_decide_with_a_margin():
    from tests.test_calib_gpu import LENGTHS, T, SEED
    for name in calib_np.PATTERNS:
        for n in LENGTHS:
            key, y = calib_np.pattern(name, n, T, SEED)
            if name in calib_np.FLOAT_PATTERNS:
                gap, split = calib_np.margins(key, y)
                assert gap > MARGIN and split > MARGIN, (name, n, gap, split)
            else:                                                         # integer-valued: sums are exact in float64, ties pool by the convention
                assert np.all(y == np.round(y)) and np.abs(y.astype(np.float64)).sum() < 2.0 ** 52, (name, n)


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("poco_op_isotonic", "poco_op_isotonic_scratch_bytes", "poco_op_calib_apply")


def test_header_declares_and_library_exports_the_new_symbols():
    from poco_amd import ops
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in _lib.header_symbols() and hasattr(L, s), s
    txt = _lib.HEADER.read_text()
    assert "#define POCO_ABI_VERSION 4" in txt and L.poco_abi_version() == 4                       # additions only
    assert f"#define POCO_ISO_TILE {ops.ISO_TILE}\n" in txt and "#define POCO_ISO_MAX_N (1 << 26)" in txt
    assert f"#define POCO_ISO_MAX_SEGS {ops.ISO_MAX_SEGS}\n" in txt


def test_scratch_query():
    from poco_amd import ops
    q = ops.isotonic_scratch_bytes
    assert q(-1, 1) == 0 and q((1 << 26) + 1, 1) == 0 and q(10, 0) == 0 and q(10, 4097) == 0
    assert 0 < q(0, 1) <= q(1, 1) < q(100000, 1) < q(1 << 26, 4096) < 1 << 32
    assert q(ops.ISO_TILE, 1) < q(ops.ISO_TILE + 1, 1) and q(12345, 2) % 256 == 0 and q(12345, 2) == q(12345, 28)


def test_isotonic_refuses_bad_arguments_before_any_gpu_work():
    from poco_amd import ops
    L = _lib.lib()
    fn = L.poco_op_isotonic
    fn.argtypes = ops.ISOTONIC_ARGTYPES
    MB = 1 << 26                                                         # fake device pointers, far enough apart not to overlap
    key, y, order, seg, scratch, block, fit, segb, knots = (MB * i for i in range(1, 10))
    M, N, S = 3000, 5000, 3
    room = ops.isotonic_scratch_bytes(N, S)

    def call(key=key, y=y, M=M, order=order, N=N, seg=seg, S=S, scratch=scratch, room=room, block=block, fit=fit, segb=segb, knots=knots, mb=0):
        return fn(key, y, M, order, N, seg, S, scratch, room, block, fit, segb, knots, mb, None)
    bad = [dict(key=None), dict(y=None), dict(order=None), dict(seg=None), dict(scratch=None), dict(block=None), dict(fit=None),
           dict(segb=None), dict(knots=None), dict(N=-1), dict(N=(1 << 26) + 1), dict(M=0), dict(M=-1), dict(M=(1 << 26) + 1), dict(S=0),
           dict(S=4097), dict(mb=-1), dict(room=0), dict(room=room - 1), dict(scratch=scratch + 4), dict(fit=fit + 4), dict(knots=knots + 4),
           dict(key=key + 2), dict(order=order + 1), dict(block=key), dict(block=y + 4 * (M - 1)), dict(fit=order + 4 * N - 8),
           dict(segb=seg + 4 * S), dict(knots=key - 32 * N + 8), dict(scratch=y - 256), dict(scratch=order), dict(block=scratch + 1024),
           dict(fit=block), dict(segb=fit + 8 * (N - 1)), dict(knots=segb), dict(knots=fit + 8)]
    for kw in bad:
        assert call(**kw) == 1, kw
        assert "poco_op_isotonic" in L.poco_last_error().decode(), kw
    # N = 0: the [N] and [M] buffers may be null, the offsets, the scratch and seg_blocks may not
    for kw in (dict(seg=None), dict(scratch=None), dict(segb=None), dict(room=0), dict(segb=seg)):
        args = dict(key=None, y=None, M=0, order=None, N=0, block=None, fit=None, knots=None, room=ops.isotonic_scratch_bytes(0, S))
        args.update(kw)
        assert call(**args) == 1, kw
        assert "poco_op_isotonic" in L.poco_last_error().decode(), kw


def test_calib_apply_refuses_bad_arguments_before_any_gpu_work():
    from poco_amd import ops
    L = _lib.lib()
    fn = L.poco_op_calib_apply
    fn.argtypes = ops.CALIB_APPLY_ARGTYPES
    MB = 1 << 26
    x, ids, offs, knots, out = (MB * i for i in range(1, 6))

    def call(x=x, R=1000, S=27, ids=ids, offs=offs, P=28, knots=knots, B=500, out=out, mb=0):
        return fn(x, R, S, ids, offs, P, knots, B, out, mb, None)
    bad = [dict(x=None), dict(ids=None), dict(offs=None), dict(knots=None), dict(out=None), dict(R=0), dict(R=(1 << 26) + 1), dict(S=0),
           dict(S=4097), dict(R=1 << 20, S=2048), dict(P=0), dict(P=4097), dict(B=-1), dict(B=(1 << 26) + 1), dict(mb=-1), dict(knots=knots + 4),
           dict(x=x + 2), dict(out=out + 1), dict(out=x), dict(out=x + 4 * 27 * 1000 - 4), dict(out=ids + 4 * 26), dict(out=offs + 4 * 28),
           dict(out=knots + 32 * 500 - 8), dict(out=x - 4 * 27 * 1000 + 4)]
    for kw in bad:
        assert call(**kw) == 1, kw
        assert "poco_op_calib_apply" in L.poco_last_error().decode(), kw


def test_ops_refuse_host_tensors_and_bad_offsets_without_a_gpu():
    import torch
    from poco_amd import ops
    with pytest.raises(_lib.PocoHipError, match="isotonic.*CUDA"):
        ops.isotonic(torch.zeros(8), torch.zeros(8), torch.zeros(8, dtype=torch.int32), [0, 8])
    with pytest.raises(_lib.PocoHipError, match="calib_apply.*CUDA"):
        ops.calib_apply(torch.zeros(8, 2), torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.int32), torch.zeros(1, 4, dtype=torch.float64))
    assert ops.check_offsets([0, 0, 5, 8, 8], 8, "t").tolist() == [0, 0, 5, 8, 8]
    assert ops.check_offsets(torch.tensor([0, 8], dtype=torch.int32), 8, "t").tolist() == [0, 8]
    for off in ([0, 5, 4, 8], [1, 8], [0, 7], [0, 9], [8], [[0, 8]], [0.0, 8.0]):
        with pytest.raises(_lib.PocoHipError, match="seg_offsets"):
            ops.check_offsets(off, 8, "isotonic: seg_offsets")


# ---- eval.py --calibrate, demo.py --calibration, the file ---------------------------------------------------------------------------------
BASE = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", "none.pt"]


def _cli(name):
    import importlib.util
    from pathlib import Path
    spec = importlib.util.spec_from_file_location(f"poco_{name}_cli_calib", Path(__file__).resolve().parent.parent / f"{name}.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_eval_flags_parse_and_are_refused_where_they_cannot_work(tmp_path):
    cli = _cli("eval")
    base = BASE + ["--j_regressor", "none.npy", "--dataset", str(tmp_path / "missing.npz")]
    a = cli.parse_args(base)
    assert a.calibrate is None and a.calib_split is None and a.calib_bins is None
    a = cli.parse_args(base + ["--calibrate", "out.npz", "--calib_split", "parity", "--calib_bins", "50"])
    assert (a.calibrate, a.calib_split, a.calib_bins) == ("out.npz", "parity", 50)
    Cf = ["--calibrate", str(tmp_path / "out.npz")]
    for flags, word in ((["--calib_bins", "20"], "need --calibrate"), (["--calib_split", "half"], "need --calibrate"),
                        (Cf + ["--calib_bins", "0"], "1..1024"), (Cf + ["--calib_bins", "1025"], "1..1024"), (Cf + ["--segm"], "--segm"),
                        (Cf + ["--likelihood"], "--likelihood"), (Cf + ["--cfg2", "configs/demo_poco_pare.yaml", "--ckpt2", "x.pt"], "--cfg2"),
                        (Cf + ["--tta", "flip", "--crop", "dataset"], "--tta"), (Cf + ["--sequences"], "--sequences"),
                        (Cf + ["--kp_refit", "1.0"], "--kp_refit"), (Cf + ["--visibility"], "--visibility"), (Cf + ["--augment"], "--augment"),
                        (Cf + ["--aug_rot", "10"], "--aug_rot"), (Cf + ["--aug_flip"], "--aug_flip"), (Cf + ["--aug_occlude", "x.pkl"], "--aug_occlude")):
        with pytest.raises(SystemExit) as e:                                     # before any GPU work, before the dataset file is looked at
            cli.main(cli.parse_args(base + flags))
        msg = str(e.value)
        assert word in msg and "calib" in msg and "\n" not in msg and "missing.npz" not in msg, (flags, msg)
    for ok in (Cf, Cf + ["--rank_metrics"], Cf + ["--calib_split", "none", "--calib_bins", "1024"], Cf + ["--aug_seed", "3"]):
        with pytest.raises(SystemExit, match="missing.npz"):                     # flags that may run get as far as the dataset file
            cli.main(cli.parse_args(base + ok))
    assert not (tmp_path / "out.npz").exists()


def _table(kinematic=True, backbone="hrnet_w48_cls-cliff"):
    from poco_amd import calibrate
    r = np.random.default_rng(1)
    tabs = []
    for m in range(28):
        key = np.sort(r.gamma(2.0, 0.1, 40 + m)).astype(np.float32)
        tabs.append(calib_np.isotonic_segment(key, ((1.0 + key) * r.gamma(2.0, 0.5, 40 + m)).astype(np.float32))[2])
    meta = calibrate.make_meta("3dpw", kinematic, backbone)
    lines = [f"{k}={v}" for k, v in meta.items()] + [f"unit:{n}={u}" for n, u in zip(calibrate.MAP_NAMES, calibrate.MAP_UNITS)]
    return {"calib_names": np.asarray(calibrate.MAP_NAMES), "calib_offsets": np.concatenate([[0], np.cumsum([len(t) for t in tabs])]).astype(np.int32),
            "calib_knots": np.concatenate(tabs), "calib_rows": np.arange(40, 68, dtype=np.int64), "calib_dropped": np.zeros(28, np.int64),
            "calib_summary": r.uniform(0, 1, (28, 3)), "calib_meta": np.asarray(lines)}


def test_npz_round_trip_and_file_checks(tmp_path):
    from poco_amd import calibrate
    res = _table()
    path = str(tmp_path / "sub" / "calib.npz")
    calibrate.save(path, res)
    back = calibrate.load(path)
    for k in calibrate.NPZ_KEYS:
        assert back[k].dtype == res[k].dtype and np.array_equal(back[k], res[k]), k
    assert back["meta"] == {"dataset": "3dpw", "kinematic": "1", "backbone": "hrnet_w48_cls-cliff", "head": "cliff",
                            **{f"unit:{n}": u for n, u in zip(calibrate.MAP_NAMES, calibrate.MAP_UNITS)}}
    assert back["meta"]["unit:crop_mpjpe"] == "m"
    calibrate.check_file(path, True, "resnet50-cliff")                    # another backbone with the same head may use the file
    with pytest.raises(ValueError, match="head"):
        calibrate.check_file(path, True, "hrnet_w32-pare")
    with pytest.raises(ValueError, match="kinematic"):
        calibrate.check_file(path, False, "resnet50-cliff")
    np.savez(tmp_path / "other.npz", x=np.zeros(3))
    with pytest.raises(ValueError, match="not a calibration file"):
        calibrate.load(str(tmp_path / "other.npz"))
    broken = dict(res, calib_offsets=res["calib_offsets"][::-1].copy())
    calibrate.save(str(tmp_path / "broken.npz"), broken)
    with pytest.raises(ValueError, match="calib_offsets"):
        calibrate.load(str(tmp_path / "broken.npz"))
    assert len(calibrate.summary_lines(res)) == 29 and calibrate.head_of("resnet50") == ""


def test_the_crop_key_on_the_host():
    from poco_amd import calibrate
    r = np.random.default_rng(6)
    var = r.uniform(0, 1, (50, 24)).astype(np.float32)
    var[0] = -0.0
    want = np.asarray([np.float32(sum((float(v) for v in row), 0.0) / 24.0) for row in var], np.float32)
    assert np.array_equal(calibrate.crop_key(var).view(np.uint32), want.view(np.uint32))
    assert calibrate.DEMO_MAP_IDS == tuple(range(4, 28)) + (0, 1, 2) and calibrate.MAP_NAMES[4] == "joint_0"


def test_demo_flag_is_refused_where_it_cannot_work(tmp_path):
    from poco_amd import calibrate
    cli = _cli("demo")
    calibrate.save(str(tmp_path / "pare.npz"), _table(backbone="hrnet_w32-pare"))
    calibrate.save(str(tmp_path / "cliff.npz"), _table())
    base = BASE + ["--mode", "folder", "--image_folder", str(tmp_path / "no_such_folder"), "--output_folder", str(tmp_path / "out"), "--no_render"]
    assert cli.parse_args(base).calibration is None
    for flags, word in ((["--calibration", str(tmp_path / "pare.npz")], "head"), (["--calibration", str(tmp_path / "missing.npz")], "--calibration"),
                        (["--calibration", str(tmp_path / "cliff.npz"), "--no_kinematic_uncert"], "kinematic"),
                        (["--calibration", str(tmp_path / "cliff.npz"), "--cfg2", "configs/demo_poco_pare.yaml", "--ckpt2", "x.pt"], "--cfg2")):
        with pytest.raises(SystemExit) as e:
            cli.main(cli.parse_args(base + flags))
        assert word in str(e.value) and "no_such_folder" not in str(e.value), (flags, e.value)
    with pytest.raises(SystemExit, match="no_such_folder"):                  # a matching file gets as far as the input folder
        cli.main(cli.parse_args(base + ["--calibration", str(tmp_path / "cliff.npz")]))
    assert not (tmp_path / "out").exists()
