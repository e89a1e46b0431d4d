"""Occlusion sensitivity maps without a GPU: the sweep positions, properties of the numpy restatement (tests/occlusion_np.py),
the C ABI's symbols and demo.py's flags."""
import numpy as np
import pytest

from poco_amd import _lib, occlusion
from tests import occlusion_np as onp


def _coverage(pos, patch, res=224):
    cnt = np.zeros((res, res), np.int32)
    for y0, x0 in pos:
        assert 0 <= y0 and y0 + patch <= res and 0 <= x0 and x0 + patch <= res, (y0, x0)
        cnt[y0:y0 + patch, x0:x0 + patch] += 1
    return cnt


def test_sweep_positions():
    """The rule: per axis k * stride for k = 0 .. ceil((res - patch) / stride), the last value clamped to res - patch.  For the
    default (224, 40, 10) that is 0, 10, ..., 180, 184: 20 per axis, 400 positions.  (19 x 19 = 361, the count 0 .. 180 alone would
    give, leaves the pixels 220 .. 223 of each axis under no patch; the rule and the coverage property it exists for decide.)"""
    p = occlusion.sweep_positions(224, 40, 10)
    assert p.dtype == np.int32 and p.shape == (400, 2) and occlusion.sweep_grid(224, 40, 10) == (20, 20)
    assert sorted(set(p[:, 0])) == list(range(0, 181, 10)) + [184] == sorted(set(p[:, 1]))
    assert np.array_equal(p[:3], [[0, 0], [0, 10], [0, 20]]) and np.array_equal(p[20], [10, 0])          # row-major (y0, x0)
    q = occlusion.sweep_positions(224, 50, 70)
    assert q.shape == (16, 2) and set(q[:, 0]) == {0, 70, 140, 174} and set(q[:, 1]) == {0, 70, 140, 174}
    assert np.array_equal(q[3], [0, 174])
    assert np.array_equal(occlusion.sweep_positions(224, 224, 10), [[0, 0]])
    assert occlusion.sweep_positions(224, 1, 223).shape == (4, 2)
    for res, patch, stride in ((224, 40, 10), (224, 50, 70), (224, 96, 64), (224, 1, 1), (224, 224, 3), (224, 223, 5), (224, 7, 100),
                               (10, 3, 4)):
        pos = occlusion.sweep_positions(res, patch, stride)
        assert np.array_equal(pos, onp.sweep_positions(res, patch, stride)), (res, patch, stride)
        cnt = _coverage(pos, patch, res)                          # (also: no patch leaves the crop)
        assert cnt[0, 0] >= 1 and cnt[-1, -1] >= 1 and cnt[0, -1] >= 1 and cnt[-1, 0] >= 1
        if stride <= patch:                                       # a step wider than the square leaves gaps between the squares
            assert cnt.min() >= 1, (res, patch, stride)
        k = occlusion.sweep_grid(res, patch, stride)
        assert k[0] * k[1] == len(pos)
    for bad in ((224, 0, 10), (224, 225, 10), (224, 40, 0), (224, -3, 10), (224, 40, -1)):
        with pytest.raises(ValueError):
            occlusion.sweep_positions(*bad)


def test_fill_and_metric_helpers():
    assert occlusion.fill_from_grey(255 * 0.485)[0] == pytest.approx(0.0, abs=1e-6)
    f = occlusion.fill_from_grey(128)
    want = [(128 / 255 - m) / s for m, s in zip(occlusion.MEAN, occlusion.STD)]
    assert np.allclose(f, want, atol=1e-6)
    for bad in (-1, 256):
        with pytest.raises(ValueError):
            occlusion.fill_from_grey(bad)
    assert occlusion.parse_metric("v2v") == "v2v" and occlusion.parse_metric("var:23") == 23 and occlusion.parse_metric("var:0") == 0
    for bad in ("var:24", "var:-1", "var:", "mesh", "var:1.5"):
        with pytest.raises(ValueError):
            occlusion.parse_metric(bad)
    lut = occlusion.jet_lut_u8()
    assert lut.shape == (256, 3) and lut.dtype == np.uint8 and tuple(lut[0]) == (0, 0, 128) and tuple(lut[255]) == (128, 0, 0)


def test_restatement_occlude_batch():
    r = np.random.default_rng(0)
    src = r.standard_normal((3, 224, 224)).astype(np.float32)
    pos = onp.sweep_positions(224, 50, 70)
    out = onp.occlude_batch(src, pos, 50, (0.5, -1.0, 2.0))
    assert out.shape == (16, 3, 224, 224) and out.dtype == np.float32
    i = 3                                                                    # (0, 174): the clamped last column
    assert (out[i, 0, :50, 174:] == 0.5).all() and (out[i, 1, :50, 174:] == -1.0).all() and (out[i, 2, :50, 174:] == 2.0).all()
    mask = np.ones((224, 224), bool)
    mask[:50, 174:] = False
    assert np.array_equal(out[i][:, mask], src[:, mask])


def test_restatement_identical_outputs_give_zero_records_and_an_unchanged_crop():
    r = np.random.default_rng(1)
    v, va, j = r.standard_normal((1, 6890, 3)).astype(np.float32), r.uniform(0.1, 1, (1, 24)).astype(np.float32), \
        r.standard_normal((1, 49, 3)).astype(np.float32)
    pos = onp.sweep_positions(224, 96, 64)
    n = len(pos)
    rec = onp.occlusion_records(np.repeat(v, n, 0), np.repeat(va, n, 0), np.repeat(j, n, 0), v[0], va[0], j[0])
    assert rec.shape == (n, 77)
    assert np.allclose(rec[:, 2], va.mean())                                 # the one column that is no difference
    rec[:, 2] = 0
    assert not rec.any()
    crop = onp.period_crop()
    for metric in ("v2v", "var", "joints", "var:5"):
        out = onp.heat_overlay(onp.field_of(rec, metric), pos, 96, crop, occlusion.jet_lut_u8(), "auto")
        assert np.array_equal(out, crop), metric


def test_restatement_records_columns():
    r = np.random.default_rng(2)
    bv, ba, bj = r.standard_normal((6890, 3)).astype(np.float32), r.uniform(0.1, 1, 24).astype(np.float32), r.standard_normal((49, 3)).astype(np.float32)
    v = np.stack([bv + np.float32(0.25), bv])
    v[1, 17] += np.float32([3, 4, 0])
    va = np.stack([ba + np.float32(0.5), ba * 2])
    j = np.stack([bj, bj + np.float32([0, 0, 2])])
    rec = onp.occlusion_records(v, va, j, bv, ba, bj)
    assert rec[0, 0] == pytest.approx(0.25 * np.sqrt(3), rel=1e-6) and rec[0, 1] == pytest.approx(0.25 * np.sqrt(3), rel=1e-6)
    assert rec[1, 0] == pytest.approx(5 / 6890, rel=1e-6) and rec[1, 1] == pytest.approx(5, rel=1e-6)
    assert rec[0, 3] == pytest.approx(0.5, rel=1e-6) and np.allclose(rec[0, 4:28], 0.5, rtol=1e-6)
    assert rec[1, 2] == pytest.approx(2 * ba.astype(np.float64).mean()) and np.allclose(rec[1, 4:28], ba)
    assert not rec[0, 28:].any() and np.allclose(rec[1, 28:], 2.0, rtol=1e-6)


def test_restatement_constant_field_is_one_colour_and_single_position_is_flat():
    lut = occlusion.jet_lut_u8()
    crop = np.full((224, 224, 3), 100, np.uint8)
    pos = onp.sweep_positions(224, 40, 10)
    # a constant field: every pixel's mean is the constant, "auto" scales it to 1 -> the hottest colour everywhere
    out = onp.heat_overlay(np.full(len(pos), 0.37, np.float32), pos, 40, crop, lut, "auto")
    want = (128 * lut[255].astype(np.int32) + 128 * 100 + 128) >> 8
    assert (out.reshape(-1, 3) == want).all()
    out = onp.heat_overlay(np.full(len(pos), 0.375, np.float32), pos, 40, crop, lut, 0.75)              # exact sums: t = 0.5, index int(127.5 + .5) = 128
    want = (128 * lut[128].astype(np.int32) + 128 * 100 + 128) >> 8
    assert (out.reshape(-1, 3) == want).all()
    # a fixed scale that clips, and negative / NaN entries at the cold end
    out = onp.heat_overlay(np.full(len(pos), 5.0, np.float32), pos, 40, crop, lut, 1.0)
    assert (out.reshape(-1, 3) == ((128 * lut[255].astype(np.int32) + 12928) >> 8)).all()
    out = onp.heat_overlay(np.full(len(pos), -5.0, np.float32), pos, 40, crop, lut, 1.0)
    assert (out.reshape(-1, 3) == ((128 * lut[0].astype(np.int32) + 12928) >> 8)).all()
    # one position (patch = the crop): one value under every pixel -> a flat colour over a flat crop, the crop's texture otherwise
    one = onp.sweep_positions(224, 224, 10)
    out = onp.heat_overlay(np.float32([0.2]), one, 224, crop, lut, "auto")
    assert len(np.unique(out.reshape(-1, 3), axis=0)) == 1
    tex = onp.period_crop()
    out = onp.heat_overlay(np.float32([0.2]), one, 224, tex, lut, 0.4)
    assert np.array_equal(out, ((128 * lut[128].astype(np.int32)[None, None] + 128 * tex.astype(np.int32) + 128) >> 8).astype(np.uint8))


def test_symbols_are_declared_and_exported():
    syms = _lib.header_symbols()
    L = _lib.lib()
    for s in ("poco_op_occlude_batch", "poco_op_occlusion_records", "poco_op_heat_overlay"):
        assert s in syms and hasattr(L, s), s
    assert "#define POCO_OCCLUSION_RECORD_FLOATS 77" in _lib.HEADER.read_text() and occlusion.REC == 77 == onp.REC


def test_argument_errors_without_gpu():
    """Validation happens before any launch: bad arguments are POCO_ERR_ARG with a message, with no device in the machine."""
    import ctypes as C
    L = _lib.lib()
    L.poco_op_occlude_batch.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.poco_op_occlusion_records.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 5
    L.poco_op_heat_overlay.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_float] + [C.c_void_p] * 4
    fill = (C.c_float * 3)(0, 0, 0)
    p = 4096                                                     # a non-null, aligned address that is never dereferenced: every call fails validation
    for a in ((None, 224, p, 1, 40, fill, p, None), (p, 222, p, 1, 40, fill, p, None), (p, 224, p, 1, 0, fill, p, None),
              (p, 224, p, 1, 225, fill, p, None), (p, 224, p, -1, 40, fill, p, None), (p, 224, None, 1, 40, fill, p, None),
              (p, 224, p, 1, 40, None, p, None), (p + 4, 224, p, 1, 40, fill, p, None), (p, 224, p, 1, 40, fill, p + 8, None)):
        assert L.poco_op_occlude_batch(*a) == 1, a
        assert b"poco_op_occlude_batch" in L.poco_last_error()
    for a in ((None, p, p, 1, 6890, p, p, p, p, None), (p, p, p, 1, 6891, p, p, p, p, None), (p, p, p, -1, 6890, p, p, p, p, None),
              (p + 4, p, p, 1, 6890, p, p, p, p, None), (p, p, p, 1, 6890, p, p, p, None, None), (p, p, p, 1, 0, p, p, p, p, None)):
        assert L.poco_op_occlusion_records(*a) == 1, a
        assert b"poco_op_occlusion_records" in L.poco_last_error()
    for a in ((None, p, 1, 40, 224, 0.0, p, p, p, None), (p, p, 0, 40, 224, 0.0, p, p, p, None), (p, p, 1, 0, 224, 0.0, p, p, p, None),
              (p, p, 1, 225, 224, 0.0, p, p, p, None), (p, p, 1, 40, 224, -1.0, p, p, p, None),
              (p, p, 1, 40, 224, float("nan"), p, p, p, None), (p, p, 1, 40, 224, float("inf"), p, p, p, None),
              (p, p, 1, 40, 224, 1.0, None, p, p, None)):
        assert L.poco_op_heat_overlay(*a) == 1, a
        assert b"poco_op_heat_overlay" in L.poco_last_error()
    # m = 0 is a no-op that needs no device
    assert L.poco_op_occlude_batch(p, 224, None, 0, 40, fill, p, None) == 0
    assert L.poco_op_occlusion_records(p, p, p, 0, 6890, p, p, p, p, None) == 0


def test_demo_flags(tmp_path, monkeypatch):
    import demo
    import poco_amd.tester as tester
    base = ["--cfg", "c.yaml", "--ckpt", "x.pt"]
    a = demo.parse_args(base)
    assert not a.occlusion_map and a.occ_patch == 40 and a.occ_stride == 10 and a.occ_fill is None and a.occ_metric == "v2v" \
        and a.occ_scale == "auto"
    a = demo.parse_args(base + ["--occlusion_map", "--occ_patch", "96", "--occ_stride", "64", "--occ_fill", "127.5", "--occ_metric",
                                "var:3", "--occ_scale", "0.05"])
    assert a.occlusion_map and a.occ_patch == 96 and a.occ_stride == 64 and a.occ_fill == 127.5 and a.occ_metric == "var:3" \
        and a.occ_scale == "0.05"
    with pytest.raises(SystemExit):
        demo.parse_args(base + ["--occ_patch", "big"])

    built = []

    class Stub:                                                   # the engine must not be built when an option is refused
        def __init__(self, args):
            built.append(args)

        def run_on_image_folder(self, *a, **k):
            return {}

    monkeypatch.setattr(tester, "POCOTester", Stub)
    (tmp_path / "imgs").mkdir()
    folder = base + ["--mode", "folder", "--image_folder", str(tmp_path / "imgs"), "--output_folder", str(tmp_path / "out")]
    with pytest.raises(SystemExit, match="--occlusion_map.*folder"):
        demo.main(demo.parse_args(base + ["--mode", "video", "--vid_file", str(tmp_path / "imgs"), "--occlusion_map"]))
    for extra, msg in ((["--occ_patch", "0"], "--occ_patch"), (["--occ_patch", "225"], "--occ_patch"), (["--occ_stride", "0"], "--occ_stride"),
                       (["--occ_fill", "256"], "--occ_fill"), (["--occ_fill", "-1"], "--occ_fill"), (["--occ_metric", "var:24"], "--occ_metric"),
                       (["--occ_metric", "heat"], "--occ_metric"), (["--occ_scale", "0"], "--occ_scale"), (["--occ_scale", "-2"], "--occ_scale"),
                       (["--occ_scale", "hot"], "--occ_scale"), (["--occ_scale", "nan"], "--occ_scale"), (["--occ_scale", "inf"], "--occ_scale")):
        with pytest.raises(SystemExit, match=msg):
            demo.main(demo.parse_args(folder + ["--occlusion_map"] + extra))
    assert not built
    demo.main(demo.parse_args(folder + ["--occ_patch", "0"]))    # without the flag its options are not looked at
    demo.main(demo.parse_args(folder + ["--occlusion_map", "--occ_patch", "224", "--occ_stride", "500", "--occ_fill", "0",
                                        "--occ_metric", "var:0", "--occ_scale", "1e-3"]))
    assert len(built) == 2
