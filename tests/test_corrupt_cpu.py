"""Image degradation without a GPU (include/poco_hip.h poco_op_corrupt): corrupt.parse_levels and every refusal,
the record layout against the C declaration, the C entry's refusals with fake pointers, the restatement tests/corrupt_np.py against
scipy (blur), by hand (pixelate, contrast), in distribution (noise) and against PIL (jpeg), and eval.py's refusals."""
import ctypes as C
import importlib.util
import io
import re
from pathlib import Path

import numpy as np
import pytest

from poco_amd import _lib, corrupt, ops
from tests import corrupt_np

ROOT = Path(__file__).resolve().parent.parent


# ---- parse_levels -----------------------------------------------------------------------------------------------------------------------
def test_parse_levels_reads_chains_and_prepends_the_clean_crop():
    lv = corrupt.parse_levels("gaussian_blur:1, gaussian_blur:2+jpeg:30,motion_blur:9:45,pixelate:3+contrast:0.5+gamma:2.2+gaussian_noise:8")
    assert lv[0] == () and len(lv) == 5
    assert lv[1] == (corrupt.Step("gaussian_blur", 1.0),)
    assert lv[2] == (corrupt.Step("gaussian_blur", 2.0), corrupt.Step("jpeg", 30.0))
    assert lv[3] == (corrupt.Step("motion_blur", 9.0, 45.0),)
    assert [s.kind for s in lv[4]] == ["pixelate", "contrast", "gamma", "gaussian_noise"]
    assert corrupt.levels_text(lv) == "clean,gaussian_blur:1,gaussian_blur:2+jpeg:30,motion_blur:9:45,pixelate:3+contrast:0.5+gamma:2.2+gaussian_noise:8"
    assert len(corrupt.parse_levels(",".join(f"jpeg:{q}" for q in range(10, 80, 10)))) == 8                       # 7 + clean = 8: allowed


@pytest.mark.parametrize("text", [
    "", " ", None, "blur:1", "gaussian_blur", "gaussian_blur:", "gaussian_blur:x", "gaussian_blur:nan", "gaussian_blur:inf", "gaussian_blur:0",
    "gaussian_blur:5.01", "gaussian_blur:-1", "gaussian_blur:1:2", "motion_blur:9", "motion_blur:8:0", "motion_blur:1:0", "motion_blur:33:0",
    "motion_blur:9:nan", "motion_blur:9.5:0", "pixelate:1", "pixelate:33", "pixelate:2.5", "contrast:-0.1", "contrast:2.1", "gamma:0.1", "gamma:5.5",
    "gaussian_noise:-1", "gaussian_noise:300", "jpeg:0", "jpeg:101", "jpeg:50.5", "jpeg:50,", "jpeg:50,,jpeg:60", "jpeg:50+", "jpeg:50,jpeg:50",
    "gamma:1+gamma:1+gamma:1+gamma:1+gamma:1", ",".join(f"jpeg:{q}" for q in range(10, 90, 10))])
def test_parse_levels_refuses(text):
    with pytest.raises(ValueError, match="--corrupt"):
        corrupt.parse_levels(text)


def test_records_are_level_major_and_name_the_dataset_row():
    lv = corrupt.parse_levels("motion_blur:5:90,gaussian_noise:8+jpeg:20")
    rec = corrupt.level_major_records(lv, [10, 11], seed=(7 << 32) | 5)
    assert rec.shape == (6, 2) and rec.dtype == ops.CORRUPT_STEP
    assert (rec["kind"][:2] == 0).all() and rec["kind"][2:4].tolist() == [[2, 0]] * 2 and rec["kind"][4:].tolist() == [[6, 7]] * 2
    assert rec["ival"][2, 0] == 5 and abs(rec["p0"][2, 0]) < 1e-7 and rec["p1"][2, 0] == 1.0
    assert rec["stream"][4:, 0].tolist() == [10, 11] and rec["seed"][4, 0].tolist() == [5, 7] and rec["ival"][5, 1] == 20
    assert rec["p0"][4, 0] == 8.0
    chains = corrupt_np.chains_from_records(rec)
    assert chains[0] == [] and [s["kind"] for s in chains[5]] == ["gaussian_noise", "jpeg"] and chains[5][0]["seed"] == (7 << 32) | 5
    with pytest.raises(ValueError):
        corrupt.records([()], [0, 1])
    with pytest.raises(ValueError):
        corrupt.records([(corrupt.Step("gamma", 1.0),) * 5], [0])


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------------
def test_header_declares_the_record_the_binding_uses():
    txt = (ROOT / "include" / "poco_hip.h").read_text()
    m = re.search(r"typedef struct \{([^}]*)\} poco_corrupt_step_t;", txt)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [re.sub(r"\s+", " ", f.strip()) for f in body.split(";") if f.strip()]
    assert fields == ["int32_t kind", "int32_t ival", "float p0, p1", "uint32_t seed[2]", "uint32_t stream"]
    assert ops.CORRUPT_STEP.names == ("kind", "ival", "p0", "p1", "seed", "stream") and ops.CORRUPT_STEP.itemsize == 28
    assert [ops.CORRUPT_STEP.fields[n][1] for n in ops.CORRUPT_STEP.names] == [0, 4, 8, 12, 16, 24]
    enum = re.search(r"enum \{ POCO_CORRUPT_NONE = 0,([^}]*)\}", txt).group(0)
    for i, name in enumerate(ops.CORRUPT_KINDS):
        assert f"POCO_CORRUPT_{name.upper()} = {i}" in enum
    assert "#define POCO_CORRUPT_MAX_STEPS 4" in txt and ops.CORRUPT_MAX_STEPS == 4 and "poco_op_corrupt" in _lib.header_symbols()


def _call(steps, N=None, L=None, lo=0, hi=None, res=8, d_in=1 << 30, d_steps=2 << 30, h=True, tmp=3 << 30, out=4 << 30):
    fn = _lib.lib().poco_op_corrupt
    fn.argtypes = [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p] * 3
    steps = np.ascontiguousarray(steps)
    N = steps.shape[0] if N is None else N
    L = steps.shape[1] if L is None else L
    return fn(d_in, d_steps, steps.ctypes.data if h else None, N, L, lo, L if hi is None else hi, res, 0, tmp, out, None)


def _rec(kind, ival=0, p0=0.0, p1=0.0, L=1, N=1):
    r = np.zeros((N, L), ops.CORRUPT_STEP)
    r[0, 0] = (ops.CORRUPT_KINDS.index(kind) if isinstance(kind, str) else kind, ival, p0, p1, (0, 0), 0)
    return r


def test_c_entry_refuses_bad_arguments_before_any_launch():
    """Fake device pointers: a call that got as far as a launch would fail differently (or fault); every one returns POCO_ERR_ARG."""
    L = _lib.lib()
    good = _rec("gamma", p0=2.0)
    bad = [dict(d_in=None), dict(d_steps=None), dict(h=False), dict(tmp=None), dict(out=None), dict(N=0), dict(N=-3), dict(res=0), dict(res=4097),
           dict(L=0), dict(L=5), dict(lo=-1), dict(lo=1, hi=0), dict(hi=2), dict(tmp=4 << 30), dict(out=1 << 30), dict(tmp=1 << 30)]
    for kw in bad:
        assert _call(good, **kw) == 1, kw
        assert "poco_op_corrupt" in L.poco_last_error().decode(), kw
    nan, inf = float("nan"), float("inf")
    for r in (_rec(8), _rec(-1), _rec("gaussian_blur", p0=0.0), _rec("gaussian_blur", p0=5.5), _rec("gaussian_blur", p0=nan),
              _rec("motion_blur", 8, 1.0, 0.0), _rec("motion_blur", 1, 1.0, 0.0), _rec("motion_blur", 33, 1.0, 0.0), _rec("motion_blur", 9, 1.0, 1.0),
              _rec("motion_blur", 9, nan, 0.0), _rec("motion_blur", 9, 0.0, inf), _rec("pixelate", 1), _rec("pixelate", 33), _rec("contrast", p0=-0.5),
              _rec("contrast", p0=2.5), _rec("contrast", p0=nan), _rec("gamma", p0=0.1), _rec("gamma", p0=6.0), _rec("gamma", p0=inf),
              _rec("gaussian_noise", p0=-1.0), _rec("gaussian_noise", p0=nan), _rec("jpeg", 0), _rec("jpeg", 101)):
        assert _call(r) == 1, r
        assert "step 0 of crop 0" in L.poco_last_error().decode(), r
    gap = np.zeros((2, 3), ops.CORRUPT_STEP)
    gap[1, 0], gap[1, 2] = _rec("gamma", p0=1.0)[0, 0], _rec("gamma", p0=1.0)[0, 0]
    assert _call(gap) == 1 and "step 2 of crop 1 follows an empty step" in L.poco_last_error().decode()


def test_ops_corrupt_refuses_host_tensors_and_bad_records_without_a_gpu():
    import torch
    with pytest.raises(_lib.PocoHipError, match="corrupt.*CUDA"):
        ops.corrupt(torch.zeros(1, 3, 8, 8), _rec("gamma", p0=1.0))
    with pytest.raises(_lib.PocoHipError, match="corrupt.*CUDA"):
        ops.corrupt(np.zeros((1, 3, 8, 8), np.float32), _rec("gamma", p0=1.0))


# ---- the restatement ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("res", [1, 2, 7, 33])
@pytest.mark.parametrize("sigma", [0.4, 1.0, 5.0])
def test_blur_restatement_equals_scipy(res, sigma):
    """radius int(3 sigma + 0.5) = 1, 3, 15: beyond res for most of these planes, so the mirror reflects more than once."""
    from scipy import ndimage
    p = np.random.default_rng(res * 10 + int(sigma * 10)).uniform(0, 255, (res, res)).astype(np.float32).astype(np.float64)
    want = ndimage.gaussian_filter(p, float(np.float32(sigma)), mode="mirror", truncate=3.0)
    assert np.abs(corrupt_np.gaussian_blur_plane(p, sigma) - want).max() <= 1e-9
    assert [corrupt_np.mirror(i, 4) for i in range(-7, 11)] == [1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2]
    assert [corrupt_np.mirror(i, 1) for i in (-3, 0, 5)] == [0, 0, 0] and [corrupt_np.mirror(i, 2) for i in range(-2, 4)] == [0, 1, 0, 1, 0, 1]


def test_pixelate_f3_on_res7_by_hand():
    p = np.arange(49, dtype=np.float64).reshape(7, 7)
    got = corrupt_np.pixelate_plane(p, 3)
    cells = {(0, 0): p[0:3, 0:3], (0, 1): p[0:3, 3:6], (0, 2): p[0:3, 6:7], (1, 0): p[3:6, 0:3], (1, 1): p[3:6, 3:6], (1, 2): p[3:6, 6:7],
             (2, 0): p[6:7, 0:3], (2, 1): p[6:7, 3:6], (2, 2): p[6:7, 6:7]}
    for y in range(7):
        for x in range(7):
            assert got[y, x] == cells[(y // 3, x // 3)].mean(), (y, x)
    assert got[0, 0] == 8.0 and got[6, 6] == 48.0 and got[0, 6] == 13.0 and got[6, 0] == 43.0          # 3x3, 1x1, 3x1 and 1x3 cells


def test_contrast_zero_is_the_mean_and_one_the_identity():
    x = np.random.default_rng(3).uniform(0, 255, (1, 3, 19, 19)).astype(np.float32)
    flat = corrupt_np.corrupt(x, [[dict(kind="contrast", p0=0.0)]])
    for c in range(3):
        m = corrupt_np.plane_mean(x[0, c].astype(np.float64))
        assert (flat[0, c] == np.float32(m)).all() and abs(m - x[0, c].astype(np.float64).mean()) < 1e-9
    same = corrupt_np.corrupt(x, [[dict(kind="contrast", p0=1.0)]])
    assert np.abs(same - x).max() <= 2.0 ** -15                           # mean + (x - mean) may round the last bit of fp32 below 256


def test_noise_moments_and_independence_of_the_batch_position():
    n = 1 << 16
    z = corrupt_np.normals(n, seed=12345, stream=3, pos=0)
    assert abs(z.mean()) <= 5.0 / np.sqrt(n)                               # se of the mean = 1 / sqrt(n)
    assert abs(z.var() - 1.0) <= 5.0 * np.sqrt(2.0 / n)                    # se of the variance of normals = sqrt(2 / n)
    assert not np.array_equal(z, corrupt_np.normals(n, 12345, 4, 0)) and not np.array_equal(z, corrupt_np.normals(n, 12345, 3, 1))
    assert not np.array_equal(z, corrupt_np.normals(n, 12346, 3, 0))
    r = np.random.default_rng(0)
    a, b, c = (r.uniform(0, 255, (3, 9, 9)).astype(np.float32) for _ in range(3))
    step = lambda s: [dict(kind="gaussian_noise", p0=8.0, seed=9, stream=s)]   # noqa: E731
    first = corrupt_np.corrupt(np.stack([a, b]), [step(5), step(6)])
    second = corrupt_np.corrupt(np.stack([c, b, a]), [step(7), step(6), step(5)])
    assert np.array_equal(first[0], second[2]) and np.array_equal(first[1], second[1]) and not np.array_equal(first[0], a)


def test_philox_known_answers():
    for counter, key, want in (((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
                               ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
                               ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))):
        assert tuple(int(w) for w in corrupt_np.philox4x32_10(counter, key)) == want


@pytest.mark.parametrize("shape", [(16, 16), (33, 17)])
@pytest.mark.parametrize("q", [10, 50, 90])
def test_jpeg_restatement_equals_pil_round_trip(shape, q):
    """DESIGN.md sections 12 and 13: libjpeg's arithmetic on both sides, so the pixels are PIL's byte for byte."""
    from PIL import Image
    r = np.random.default_rng(q + shape[0])
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    rgb = np.clip(np.stack([8 * xx, 6 * yy, 4 * (xx + yy)], -1) + r.integers(-20, 21, shape + (3,)), 0, 255).astype(np.uint8)
    f = io.BytesIO()
    Image.fromarray(rgb).save(f, "JPEG", quality=q, subsampling=2)
    want = np.array(Image.open(io.BytesIO(f.getvalue())).convert("RGB"))
    assert np.array_equal(corrupt_np.jpeg_round_trip(rgb, q), want)


# ---- eval.py ---------------------------------------------------------------------------------------------------------------------------------
def _cli():
    spec = importlib.util.spec_from_file_location("poco_eval_cli_corrupt_cpu", ROOT / "eval.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_eval_flags_parse_and_are_refused_where_they_cannot_work(tmp_path):
    cli = _cli()
    base = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", "none.pt", "--j_regressor", "none.npy", "--dataset", str(tmp_path / "missing.npz")]
    a = cli.parse_args(base)
    assert a.corrupt is None and a.corrupt_seed is None
    a = cli.parse_args(base + ["--corrupt", "jpeg:20", "--corrupt_seed", "7"])
    assert (a.corrupt, a.corrupt_seed) == ("jpeg:20", 7)
    flag = ["--crop", "dataset", "--corrupt", "gaussian_blur:2,jpeg:20+gaussian_noise:8"]
    refused = [(["--corrupt_seed", "3"], "--corrupt_seed"), (["--corrupt", "jpeg:20"], "--crop dataset"), (["--crop", "dataset", "--corrupt", "jpeg:0"], "jpeg"),
               (flag + ["--corrupt_seed", "-1"], "--corrupt_seed"), (flag + ["--tta", "flip"], "--tta"), (flag + ["--cfg2", "x.yaml", "--ckpt2", "y.pt"], "--cfg2"),
               (flag + ["--segm"], "--segm"), (flag + ["--likelihood"], "--likelihood"), (flag + ["--sequences"], "--sequences"),
               (flag + ["--visibility"], "--visibility"), (flag + ["--kp_refit", "1.0"], "--kp_refit"), (flag + ["--calibrate", str(tmp_path / "c.npz")], "--calibrate"),
               (flag + ["--rank_metrics"], "--rank_metrics")]
    for extra, word in refused:
        with pytest.raises(SystemExit) as e:
            cli.main(cli.parse_args(base + extra))
        assert word in str(e.value) and "corrupt" in str(e.value), (extra, str(e.value))
    for ok in (flag, flag + ["--bootstrap", "100"], flag + ["--save_results"], flag + ["--aug_rot", "10"], flag + ["--corrupt_seed", "9"]):
        with pytest.raises(SystemExit, match="missing.npz"):                     # flags that may run get as far as the dataset file
            cli.main(cli.parse_args(base + ok))
