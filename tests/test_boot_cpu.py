"""The cluster bootstrap without a GPU: the yardstick tests/boot_np.py against the Random123 known answers, the index map, the
statistics of poco_amd/bootstrap.py on hand-made moments against numpy and scipy on the resampled rows, one statistical sanity case,
the C ABI's declarations and argument checks, and eval.py's refusals (include/poco_hip.h poco_op_bootstrap)."""
import math

import numpy as np
import pytest

from poco_amd import _lib
from tests import boot_np

EPS = 2.0 ** -52
TOL = 64 * EPS                                                            # relative, for statistics formed from exact-ish moments


# ---- Philox and the index map ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counter,key,want", [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))])
def test_philox_known_answers(counter, key, want):
    assert boot_np.philox(counter, key) == want


def test_draws_are_the_words_of_the_counters_in_order():
    seed = (0x299f31d0 << 32) | 0xa4093822
    U = 11
    idx = boot_np.draws(seed, 7, U)
    words = [w for q in range(3) for w in boot_np.philox((q, 0, 7, 0), (0xa4093822, 0x299f31d0))][:U]
    assert idx.tolist() == [(w * U) >> 32 for w in words]
    assert not np.array_equal(idx, boot_np.draws(seed, 8, U)) and not np.array_equal(idx, boot_np.draws(seed + 1, 7, U))


@pytest.mark.parametrize("U", [1, 2, 3, 4, 5, 63, 257, 1000])
def test_index_map(U):
    for b in (1, 2, 65536):
        idx = boot_np.draws(12345, b, U)
        assert np.array_equal(idx, boot_np.draws_np(12345, b, U))
        assert np.array_equal(boot_np.draws((1 << 64) - 1 - b, b, U), boot_np.draws_np((1 << 64) - 1 - b, b, U))
        assert len(idx) == U and idx.min() >= 0 and idx.max() < U
        if U == 1:
            assert not idx.any()
    mom = np.ones((U, 1))
    out, _, counts = boot_np.resample(mom, 3, 99)
    assert counts.shape == (3, U) and np.all(counts.sum(axis=1) == U) and np.all(out == U)


def test_fsum_follows_ieee_where_math_fsum_raises():
    inf, nan = math.inf, math.nan
    assert boot_np.fsum([1.0, inf]) == inf and boot_np.fsum([-inf, 2.0]) == -inf and math.isnan(boot_np.fsum([inf, -inf]))
    assert math.isnan(boot_np.fsum([nan, 1.0])) and boot_np.fsum([]) == 0.0 and boot_np.fsum([1e100, 1.0, -1e100]) == 1.0


# ---- the statistics on hand-made moments -------------------------------------------------------------------------------------------
def _labelled_planes(seed, N, S, L):
    r = np.random.default_rng(seed)
    crop = np.abs(r.standard_normal((4 * L, N))).astype(np.float32) * 0.05 + 0.01
    joint = np.abs(r.standard_normal((2 * L, N * S))).astype(np.float32)
    for l in range(L):
        crop[4 * l] += 0.5 * crop[4 * l + 1]                               # an uncertainty that follows the error
        joint[2 * l] += 0.3 * joint[2 * l + 1]
    return crop, joint


@pytest.mark.parametrize("offsets", [None, [0, 0, 3, 4, 9, 9, 17, 20, 20]])
def test_statistics_match_numpy_and_scipy_on_the_resampled_rows(offsets):
    from scipy.stats import pearsonr
    from poco_amd import bootstrap
    N, S, L, B, seed = 20, 3, 2, 6, 5
    crop, joint = _labelled_planes(1, N, S, L)
    off = boot_np.offsets_of(N, offsets)
    c = boot_np.bootstrap(crop, bootstrap.crop_pairs(L), off, B, seed)
    j = boot_np.bootstrap(joint, bootstrap.joint_pairs(L), off * S, B, seed)
    names, stats = bootstrap.statistics(["A", "B"], c["out"], c["center"], j["out"], j["center"])
    assert len(names) == 15 and stats.shape == (15, B + 1) and names[0] == "A MPJPE" and names[10] == "B - A MPJPE"
    assert names[8] == "B Uncert Error Correlation" and names[14] == "B - A Corr(crop uncertainty, MPJPE)"
    U = len(off) - 1
    for b in range(B + 1):
        idx = np.arange(U) if b == 0 else boot_np.draws(seed, b, U)
        rows = np.concatenate([np.arange(off[u], off[u + 1]) for u in idx])
        jrows = (rows[:, None] * S + np.arange(S)[None]).reshape(-1)
        cd, jd = crop.astype(np.float64)[:, rows], joint.astype(np.float64)[:, jrows]
        want = []
        for l in range(L):
            want.append([1000.0 * np.mean(cd[4 * l + 1]), 1000.0 * np.mean(cd[4 * l + 2]), 1000.0 * np.mean(cd[4 * l + 3]),
                         pearsonr(jd[2 * l + 1], jd[2 * l])[0], pearsonr(cd[4 * l], cd[4 * l + 1])[0]])
        full = want[0] + want[1] + [x - y for x, y in zip(want[1], want[0])]
        for k, w in enumerate(full):
            scale = abs(w) if k < 10 else max(abs(full[k - 5]), abs(full[k - 10]))     # a difference: of the two values it is formed from
            assert abs(stats[k, b] - w) <= TOL * scale, (names[k], b, stats[k, b], w)
    assert np.allclose(boot_np.evaluator_summary(crop, joint, offsets, S, B, seed, 0.9),
                       np.asarray([bootstrap.summarize(s, 0.9) for s in stats]), rtol=1e-12, atol=0, equal_nan=True)


def test_single_unnamed_label_and_summary_rules():
    from poco_amd import bootstrap
    crop, joint = _labelled_planes(2, 9, 2, 1)
    c = boot_np.bootstrap(crop, bootstrap.crop_pairs(1), None, 4, 0)
    j = boot_np.bootstrap(joint, bootstrap.joint_pairs(1), np.arange(10) * 2, 4, 0)
    names, stats = bootstrap.statistics([""], c["out"], c["center"], j["out"], j["center"])
    assert names == list(bootstrap.STAT_NAMES) and stats.shape == (5, 5)
    nan = math.nan
    s = bootstrap.summarize(np.asarray([1.0, 2.0, nan, 4.0, math.inf, 3.0]), 0.5)           # 3 of 5 valid
    assert s[0] == 1.0 and s[4] == 3 and s[1] == np.std([2.0, 4.0, 3.0], ddof=1) and (s[2], s[3]) == (2.5, 3.5)
    s = bootstrap.summarize(np.asarray([1.0, 2.0, nan, nan, math.inf, 3.0]), 0.5)           # 2 of 5: fewer than half
    assert s[4] == 2 and s[1] == np.std([2.0, 3.0], ddof=1) and math.isnan(s[2]) and math.isnan(s[3])
    s = bootstrap.summarize(np.asarray([nan, nan, nan]), 0.95)
    assert math.isnan(s[0]) and math.isnan(s[1]) and math.isnan(s[2]) and s[4] == 0
    same = bootstrap.summarize(np.asarray([0.0, 0.0, 0.0, 0.0]), 0.95)
    assert same == (0.0, 0.0, 0.0, 0.0, 3.0)
    # a constant plane has no variance: r is NaN in every row, not an error
    flat = np.ones((4, 9), np.float32)
    c = boot_np.bootstrap(flat, bootstrap.crop_pairs(1), None, 3, 0)
    _, st = bootstrap.statistics([""], c["out"], c["center"], j["out"][:4], j["center"])
    assert np.all(np.isnan(st[4])) and np.all(st[0] == 1000.0)


def test_standard_error_of_the_mean_of_normal_rows():
    """4 096 standard-normal rows, row units, B = 2 000: the bootstrap standard error of the mean against s / sqrt(n).  Its relative
    spread is about sqrt(1 / (2 B) + 1 / (2 n)) = 2 %, so 10 % is five of those."""
    n, B, seed = 4096, 2000, 5
    x = np.random.default_rng(seed).standard_normal(n).astype(np.float32).astype(np.float64)
    means = np.empty(B + 1)
    means[0] = x.mean()
    for b in range(1, B + 1):
        idx = boot_np.draws_np(seed, b, n)
        means[b] = x[idx].mean()
    from poco_amd import bootstrap
    point, se, lo, hi, valid = bootstrap.summarize(means, 0.95)
    ratio = se / (x.std(ddof=1) / math.sqrt(n))
    print("bootstrap se / (s / sqrt(n)):", ratio)
    assert valid == B and abs(ratio - 1.0) <= 0.10
    assert lo <= point <= hi and point == x.mean()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
NEW_SYMBOLS = ("poco_op_bootstrap", "poco_op_bootstrap_scratch_bytes")


def test_header_declares_and_library_exports_the_new_symbols():
    from poco_amd import ops
    L = _lib.lib()
    for s in NEW_SYMBOLS:
        assert s in _lib.header_symbols() and hasattr(L, s), s
    txt = _lib.HEADER.read_text()
    assert "#define POCO_ABI_VERSION 4" in txt and L.poco_abi_version() == 4                       # additions only
    assert "#define POCO_BOOT_MAX_N (1 << 24)" in txt and f"#define POCO_BOOT_MAX_PLANES {ops.BOOT_MAX_PLANES}\n" in txt
    assert f"#define POCO_BOOT_MAX_PAIRS {ops.BOOT_MAX_PAIRS}\n" in txt and f"#define POCO_BOOT_MAX_B {ops.BOOT_MAX_B}\n" in txt
    assert "2^-32" in txt and "8e-6" in txt and "2^-8" in txt                                      # the bias note


def test_scratch_query():
    from poco_amd import ops
    q = ops.bootstrap_scratch_bytes
    for bad in ((0, 1, 0, 1), ((1 << 24) + 1, 1, 0, 1), (10, 0, 0, 10), (10, 17, 0, 10), (10, 1, -1, 10), (10, 1, 17, 10), (10, 1, 0, 0),
                (10, 1, 0, 11)):
        assert q(*bad) == 0, bad
    assert 0 < q(1, 1, 0, 1) <= q(100000, 4, 3, 100000) <= q(1 << 24, 16, 16, 1 << 24) < 1 << 32
    assert q(4096, 1, 0, 1) < q(4096 * 40, 1, 0, 1) and q(12345, 3, 1, 7) % 256 == 0


def test_bootstrap_refuses_bad_arguments_before_any_gpu_work():
    from poco_amd import ops
    L = _lib.lib()
    fn = L.poco_op_bootstrap
    fn.argtypes = ops.BOOTSTRAP_ARGTYPES
    GB = 1 << 30                                                         # fake device pointers, far enough apart not to overlap
    planes, offs, scratch, center, mom, out, counts = (GB * i for i in range(1, 8))
    n, E, P, U, B = 5000, 3, 2, 40, 100
    M = 1 + E + P
    host_pairs = np.asarray([[0, 1], [2, 2]], np.int32)
    bad_pairs = [np.asarray([[0, 3], [2, 2]], np.int32), np.asarray([[0, 1], [-1, 2]], np.int32)]
    room = ops.bootstrap_scratch_bytes(n, E, P, U)

    def call(planes=planes, n=n, E=E, pairs=host_pairs, P=P, offs=offs, U=U, B=B, seed=3, scratch=scratch, room=room, center=center, mom=mom,
             out=out, counts=counts, mb=0):
        return fn(planes, n, E, None if pairs is None else pairs.ctypes.data, P, offs, U, B, seed, scratch, room, center, mom, out, counts, mb,
                  None)
    bad = [dict(planes=None), dict(pairs=None), dict(scratch=None), dict(center=None), dict(mom=None), dict(out=None),
           dict(offs=None),                                               # no offsets: U must be n
           dict(n=0), dict(n=(1 << 24) + 1), dict(E=0), dict(E=17), dict(P=-1), dict(P=17), dict(U=0), dict(U=n + 1), dict(B=-1),
           dict(B=65537), dict(mb=-1), dict(pairs=bad_pairs[0]), dict(pairs=bad_pairs[1]), dict(room=0), dict(room=room - 1),
           dict(scratch=scratch + 4), dict(center=center + 4), dict(mom=mom + 4), dict(out=out + 4), dict(planes=planes + 2),
           dict(offs=offs + 1), dict(counts=counts + 2),
           dict(center=planes), dict(mom=planes + 4 * E * n - 8), dict(out=offs + 4 * U), dict(counts=offs), dict(scratch=planes + 8),
           dict(center=scratch), dict(mom=center), dict(out=mom + 8 * U * M - 8), dict(counts=out + 8 * B * M), dict(out=mom - 8 * (B + 1) * M + 8),
           dict(counts=mom - 4 * B * U + 4), dict(mom=scratch + 8)]
    for kw in bad:
        assert call(**kw) == 1, kw
        assert "poco_op_bootstrap" in L.poco_last_error().decode(), kw


def test_ops_refuse_host_tensors_and_bad_arguments_without_a_gpu():
    import torch
    from poco_amd import ops
    with pytest.raises(_lib.PocoHipError, match="bootstrap.*CUDA"):
        ops.bootstrap(torch.zeros(2, 8), [(0, 1)], None, 4, 0)
    with pytest.raises(_lib.PocoHipError, match="bootstrap.*CUDA"):
        ops.bootstrap(torch.zeros(8), [], None, 4, 0)
    for off in ([0, 5, 4, 8], [1, 8], [0, 7], [0, 9], [8]):
        with pytest.raises(_lib.PocoHipError, match="bootstrap: unit_offsets"):
            ops.check_offsets(off, 8, "bootstrap: unit_offsets")


# ---- eval.py --bootstrap ------------------------------------------------------------------------------------------------------------
BASE = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", "none.pt"]


def _cli(name):
    import importlib.util
    from pathlib import Path
    spec = importlib.util.spec_from_file_location(f"poco_{name}_cli_boot", Path(__file__).resolve().parent.parent / f"{name}.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_spec_and_flag_errors():
    from poco_amd import bootstrap
    s = bootstrap.BootSpec(2000)
    assert (s.B, s.unit, s.level, s.seed) == (2000, "crop", 0.95, 0)
    for kw in (dict(B=0), dict(B=65537), dict(B=10, unit="row"), dict(B=10, level=1.0), dict(B=10, level=0.0), dict(B=10, seed=-1),
               dict(B=10, seed=1 << 53)):
        with pytest.raises(ValueError, match="boot"):
            bootstrap.BootSpec(**kw)


def test_eval_flags_parse_and_are_refused_where_they_cannot_work(tmp_path):
    cli = _cli("eval")
    base = BASE + ["--j_regressor", "none.npy", "--dataset", str(tmp_path / "missing.npz")]
    a = cli.parse_args(base)
    assert a.bootstrap is None and a.boot_unit is None and a.boot_level is None and a.boot_seed is None
    a = cli.parse_args(base + ["--bootstrap", "2000", "--boot_unit", "track", "--boot_level", "0.9", "--boot_seed", "7"])
    assert (a.bootstrap, a.boot_unit, a.boot_level, a.boot_seed) == (2000, "track", 0.9, 7)
    Bf = ["--bootstrap", "100"]
    for flags, word in ((["--boot_unit", "crop"], "needs --bootstrap"), (["--boot_level", "0.9"], "needs --bootstrap"),
                        (["--boot_seed", "1"], "needs --bootstrap"), (["--bootstrap", "0"], "1..65536"), (["--bootstrap", "65537"], "1..65536"),
                        (Bf + ["--boot_level", "1.0"], "--boot_level"), (Bf + ["--boot_level", "0"], "--boot_level"),
                        (Bf + ["--boot_seed", "-1"], "--boot_seed"), (Bf + ["--segm"], "--segm"), (Bf + ["--likelihood"], "--likelihood"),
                        (Bf + ["--sequences"], "--sequences"), (Bf + ["--visibility"], "--visibility")):
        with pytest.raises(SystemExit) as e:                                     # before any GPU work, before the dataset file is looked at
            cli.main(cli.parse_args(base + flags))
        msg = str(e.value)
        assert word in msg and "boot" in msg and "\n" not in msg and "missing.npz" not in msg, (flags, msg)
    for ok in (Bf, Bf + ["--rank_metrics"], Bf + ["--boot_unit", "track", "--boot_level", "0.5", "--boot_seed", "9"], Bf + ["--aug_seed", "3"],
               Bf + ["--kp_refit", "1.0"], Bf + ["--calibrate", str(tmp_path / "c.npz")]):
        with pytest.raises(SystemExit, match="missing.npz"):                     # flags that may run get as far as the dataset file
            cli.main(cli.parse_args(base + ok))


def test_boot_unit_track_refuses_names_that_do_not_group(tmp_path):
    cli = _cli("eval")
    n = 4
    common = dict(center=np.zeros((n, 2), np.float32), scale=np.ones(n, np.float32), pose=np.zeros((n, 72), np.float32),
                  shape=np.zeros((n, 10), np.float32))
    np.savez(tmp_path / "bad.npz", imgname=np.asarray(["a/x.png", "a/y.png", "a/z.png", "a/w.png"]), **common)
    np.savez(tmp_path / "good.npz", imgname=np.asarray(["a/im_1.png", "a/im_2.png", "b/im_1.png", "b/im_2.png"]), **common)
    args = lambda ds, unit: cli.parse_args(BASE + ["--j_regressor", str(tmp_path / "noJ.npy"), "--dataset", str(tmp_path / ds),   # noqa: E731
                                                   "--bootstrap", "10", "--boot_unit", unit])
    with pytest.raises(SystemExit) as e:
        cli.main(args("bad.npz", "track"))
    assert "--boot_unit track" in str(e.value) and "frame number" in str(e.value)
    for ds, unit in (("bad.npz", "crop"), ("good.npz", "track")):                 # these get as far as the next check
        with pytest.raises(SystemExit) as e:
            cli.main(args(ds, unit))
        assert "joint regressor not found" in str(e.value)
