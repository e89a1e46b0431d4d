"""CPU: the contract of test-time augmentation pinned on its numpy restatement tests/tta_np.py - the yardstick
of tests/test_tta_gpu.py: the inverse transforms against datacrop.pose_processing (itself pinned to the reference by
tests/golden/datacrop.npz), the fixed-sweep Jacobi projection against the SVD projection, the properties of the fusion, and the host
side: parse_views, every flag refusal of eval.py and demo.py, the C ABI's declaration and argument checks (fake pointers, refused
before any GPU work)."""
import importlib.util
import math
from pathlib import Path

import numpy as np
import pytest

from poco_amd import _lib, datacrop, tta
from tests import tta_np

ROOT = Path(__file__).resolve().parent.parent


def rodrigues(aa):
    """Axis-angle [3] -> rotation matrix, float64."""
    a = np.asarray(aa, np.float64).reshape(3)
    th = math.sqrt(float(a @ a))
    if th < 1e-300:
        return np.eye(3)
    k = a / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + math.sin(th) * Kx + (1 - math.cos(th)) * (Kx @ Kx)


def random_rotation(r, max_angle=math.pi):
    axis = r.standard_normal(3)
    return rodrigues(axis / np.linalg.norm(axis) * r.uniform(0, max_angle))


# ---- inverse transforms ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", [0, 1])
@pytest.mark.parametrize("rot", [0, 15, -15, 90, 180])
def test_untransform_inverts_pose_processing(rot, f):
    """pose_processing hands out float32 axis-angle: one rounding of 2^-24 relative on components of at most pi, 1.9e-7 per component,
    3.3e-7 on the vector, and a rotation matrix moves by at most that much per entry: 1e-6 bounds it."""
    r = np.random.default_rng(100 + rot + f)
    c, s = tta_np.view_cs(rot)
    worst = 0.0
    for _ in range(6):
        p = 0.6 * r.standard_normal(72)
        q = datacrop.pose_processing(p, rot, f)
        assert q.dtype == np.float32
        for j in range(24):
            js = tta_np.FLIP_PERM[j] if f else j
            back = tta_np.untransform(rodrigues(q[3 * js:3 * js + 3]), j, f, c, s)
            worst = max(worst, np.abs(back - rodrigues(p[3 * j:3 * j + 3])).max())
    assert worst <= 1e-6, worst
    if rot or f:                                                  # the transform did something: without the inverse the root is elsewhere
        assert np.abs(rodrigues(q[:3]) - rodrigues(p[:3])).max() > 1e-3


def test_the_flip_on_matrices_is_flip_pose_exactly():
    r = np.random.default_rng(3)
    for _ in range(5):
        p = r.standard_normal(72)
        fp = datacrop.flip_pose(p)
        assert fp.dtype == np.float64
        for j in range(24):
            js = tta_np.FLIP_PERM[j]
            assert np.abs(tta_np.unflip(rodrigues(p[3 * js:3 * js + 3])) - rodrigues(fp[3 * j:3 * j + 3])).max() <= 1e-12
    R = random_rotation(r)
    assert np.array_equal(tta_np.unflip(tta_np.unflip(R)), R)     # an involution, exact


def test_view_cs_is_exact_at_the_quarter_turns():
    from poco_amd import ops
    for fn in (tta_np.view_cs, ops.tta_view_cs):
        assert fn(0) == (1.0, 0.0) and fn(90) == (0.0, 1.0) and fn(-90) == (0.0, -1.0) and fn(180) == (-1.0, 0.0) and fn(-180) == (-1.0, 0.0)
        c, s = fn(15)
        assert abs(c - math.cos(math.pi / 12)) <= 1e-16 and abs(s - math.sin(math.pi / 12)) <= 1e-16
    assert all(tta_np.view_cs(x) == ops.tta_view_cs(x) for x in (0, 15, -15, 33.3, 90, -90, 180, -180, 179.5))


# ---- the solve ------------------------------------------------------------------------------------------------------------------
def solve_cases():
    """(M, W) of K rotations within 0.6 rad of a common one under positive weights.  For a unit x, x^T (sum w_k Q_k / W) x >= cos 0.6 =
    0.825 (Q_k = the perturbations), so the smallest singular value of M / W is at least 0.825: no case is near-singular."""
    r = np.random.default_rng(26)
    cases = []
    for K in (2, 3, 5, 8):
        for spread in (0.0, 1e-3, 0.2, 0.6):
            for wmax in (1.0, 1e3, 1e9):
                R0 = random_rotation(r)
                Rs = [R0 @ random_rotation(r, spread) for _ in range(K)]
                w = r.uniform(wmax / 100, wmax, K)
                cases.append((sum(wk * Rk for wk, Rk in zip(w, Rs)), float(w.sum())))
    return cases


def test_jacobi_projection_equals_the_svd_projection():
    worst = 0.0
    for M, W in solve_cases():
        assert np.linalg.svd(M / W, compute_uv=False).min() > 0.3
        R = tta_np.project(M)
        worst = max(worst, np.abs(R - tta_np.project_svd(M)).max())
        assert abs(np.linalg.det(R) - 1) <= 1e-12 and np.abs(R.T @ R - np.eye(3)).max() <= 1e-12
    assert worst <= 1e-12, worst


def test_projection_of_a_singular_sum_is_still_a_rotation():
    R1 = random_rotation(np.random.default_rng(1))
    M = R1 + R1 @ np.diag([1.0, -1.0, -1.0])                      # a half-turn apart: rank 1
    assert np.linalg.svd(M, compute_uv=False)[1] < 1e-12
    R = tta_np.project(M)
    assert np.isfinite(R).all() and np.abs(R.T @ R - np.eye(3)).max() <= 1e-12 and np.linalg.det(R) > 0
    assert np.array_equal(tta_np.project(np.zeros((3, 3))), np.eye(3))


# ---- properties of the fusion -----------------------------------------------------------------------------------------------------
def _identical(K, B=2, seed=4):
    r = np.random.default_rng(seed)
    pose = np.stack([random_rotation(r) for _ in range(B * 24)]).reshape(1, B, 24, 3, 3)
    var = r.uniform(0.01, 0.5, (1, B, 24)).astype(np.float32).astype(np.float64)
    betas = r.standard_normal((1, B, 10))
    return np.tile(pose, (K, 1, 1, 1, 1)).reshape(K * B, 24, 3, 3), np.tile(var, (K, 1, 1)).reshape(K * B, 24), np.tile(betas, (K, 1, 1)).reshape(K * B, 10)


@pytest.mark.parametrize("weight", [0, 1])
@pytest.mark.parametrize("K", [2, 3, 8])
def test_identical_views_fuse_to_themselves(K, weight):
    pose, var, betas = _identical(K)                              # float64 rotations: orthonormal to 1e-16
    o = tta_np.fuse(pose, var, betas, [(0, 0.0)] * K, weight)
    B = len(pose) // K
    assert np.abs(o["pose"] - pose[:B]).max() <= 1e-12
    assert np.nanmax(o["spread"]) <= 1e-24 and not np.isnan(o["spread"]).any()
    assert np.array_equal(o["var"].astype(np.float32), var[:B].astype(np.float32)) and np.abs(o["var"] / var[:B] - 1).max() <= 1e-15
    assert np.abs(o["betas"] - betas[:B]).max() <= 1e-14


def _views_case(seed=7, K=4, B=3):
    r = np.random.default_rng(seed)
    views = [(0, 0.0), (1, 0.0), (0, 15.0), (1, -90.0)][:K]
    pose = np.stack([random_rotation(r) for _ in range(K * B * 24)]).reshape(K * B, 24, 3, 3).astype(np.float32)
    var = r.uniform(0.01, 0.5, (K * B, 24)).astype(np.float32)
    betas = r.standard_normal((K * B, 10)).astype(np.float32)
    return pose, var, betas, views


def test_var_under_uncertainty_weights_is_the_harmonic_mean():
    pose, var, betas, views = _views_case()
    K, B = len(views), len(pose) // len(views)
    o = tta_np.fuse(pose, var, betas, views, 1)
    v = var.reshape(K, B, 24).astype(np.float64)
    for b in range(B):
        for j in range(24):
            vs = np.array([v[k, b, tta_np.FLIP_PERM[j] if views[k][0] else j] for k in range(K)])
            hm = K / np.sum(1.0 / (vs + 1e-9)) - 1e-9             # sum w v = K - 1e-9 W
            assert abs(o["var"][b, j] / hm - 1) <= 1e-12
            assert vs.min() <= o["var"][b, j] <= vs.mean()
    u = tta_np.fuse(pose, var, betas, views, 0)
    assert np.abs(u["var"][0, 3] - np.mean([v[k, 0, 3] for k in range(K)])) <= 1e-15      # joint 3 is its own mirror


@pytest.mark.parametrize("weight", [0, 1])
def test_a_view_with_nan_var_or_nan_pose_drops_out(weight):
    pose, var, betas, views = _views_case()
    K, B = len(views), len(pose) // len(views)
    keep = [0, 1, 3]
    rows = lambda a, ks: np.concatenate([a[k * B:(k + 1) * B] for k in ks])   # noqa: E731
    want = tta_np.fuse(rows(pose, keep), rows(var, keep), rows(betas, keep), [views[k] for k in keep], weight)
    for what in ("var", "pose", "neg", "inf"):
        p, v = pose.copy(), var.copy()
        if what == "var":
            v[2 * B:3 * B] = np.nan
        elif what == "neg":
            v[2 * B:3 * B] = -0.25
        elif what == "inf":
            v[2 * B:3 * B] = np.inf
        else:
            p[2 * B:3 * B, :, 1, 2] = np.nan
        o = tta_np.fuse(p, v, betas, views, weight)
        assert o["dropped"][2].all() and not o["dropped"][[0, 1, 3]].any()
        for k in ("pose", "var", "spread", "betas"):
            assert np.array_equal(o[k], want[k]), (what, k)


def test_all_views_dropped_copies_the_base_row_and_spread_is_nan():
    pose, var, betas, views = _views_case()
    K, B = len(views), len(pose) // len(views)
    v = var.copy()
    v.reshape(K, B, 24)[:, 1, 5] = np.nan                         # joint 5 of crop 1 in every view - and its mirror 4 in the flipped ones
    v.reshape(K, B, 24)[:, 1, 4] = np.nan
    v.reshape(K, B, 24)[:, 2, 0] = np.nan                         # the root of crop 2: its shape has no weight either
    o = tta_np.fuse(pose, v, betas, views, 1)
    assert np.isnan(o["spread"][1, 5]) and np.isnan(o["spread"][1, 4]) and np.isnan(o["spread"][2, 0]) and np.isnan(o["spread"]).sum() == 3
    assert np.array_equal(o["pose"][1, 5], pose[1, 5].astype(np.float64)) and np.isnan(o["var"][1, 5])
    assert np.array_equal(o["betas"][2], betas[2].astype(np.float64)) and not np.array_equal(o["betas"][1], betas[1].astype(np.float64))
    assert o["W"][1, 5] == 0 and o["W"][1, 6] > 0


# ---- parse_views ----------------------------------------------------------------------------------------------------------------
def test_parse_views():
    V = tta.View
    assert tta.parse_views("flip,rot:-15,rot:15,flip+scale:1.1") == [V(), V(flip=True), V(rot=-15.0), V(rot=15.0), V(flip=True, scale=1.1)]
    assert tta.parse_views(" rot:180 + flip ") == [V(), V(flip=True, rot=180.0)]
    assert tta.views_text(tta.parse_views("flip,rot:-15+scale:0.9")) == "identity,flip,rot:-15+scale:0.9"
    assert len(tta.parse_views("rot:1,rot:2,rot:3,rot:4,rot:5,rot:6,rot:7")) == 8
    for bad, word in (("flip,flip", "twice"), ("rot:0", "twice"), ("scale:1", "twice"), ("rot:15,scale:1+rot:15", "twice"),
                      ("rot:1,rot:2,rot:3,rot:4,rot:5,rot:6,rot:7,rot:8", "at most 8"), ("scale:0", "scale must be > 0"),
                      ("scale:-1.5", "scale must be > 0"), ("rot:181", "at most 180"), ("rot:-180.5", "at most 180"), ("rot:nan", "finite"),
                      ("scale:inf", "finite"), ("rot:", "finite"), ("rot", "cannot read"), ("flip:1", "cannot read"), ("mirror", "cannot read"),
                      ("flip+flip", "cannot read"), ("rot:1+rot:2", "cannot read"), ("flip,,rot:5", "cannot read"), ("", "at least one"),
                      (None, "at least one")):
        with pytest.raises(ValueError, match=word):
            tta.parse_views(bad)


# ---- eval.py and demo.py ----------------------------------------------------------------------------------------------------------
BASE = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", "none.pt"]


def _one_sentence(msg, word):
    assert word in msg and msg.count(". ") == 0 and "\n" not in msg, msg


def test_eval_flags_parse_and_are_refused_where_they_cannot_work(tmp_path):
    spec = importlib.util.spec_from_file_location("poco_eval_cli_tta", ROOT / "eval.py")
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = BASE + ["--j_regressor", "none.npy", "--dataset", str(tmp_path / "missing.npz")]
    a = cli.parse_args(base)
    assert a.tta is None and a.tta_weight is None
    a = cli.parse_args(base + ["--tta", "flip,rot:15", "--tta_weight", "uniform"])
    assert (a.tta, a.tta_weight) == ("flip,rot:15", "uniform")
    with pytest.raises(SystemExit):
        cli.parse_args(base + ["--tta", "flip", "--tta_weight", "median"])
    T = ["--tta", "flip", "--crop", "dataset"]
    for flags, word in ((["--tta", "flip"], "--crop dataset"), (["--tta", "flip", "--crop", "demo"], "--crop dataset"),
                        (T + ["--aug_rot", "10"], "--aug_rot"), (T + ["--aug_scale", "1.1"], "--aug_scale"), (T + ["--aug_flip"], "--aug_flip"),
                        (T + ["--aug_noise", "1,1,1"], "--aug_noise"), (T + ["--augment"], "--augment"),
                        (T + ["--aug_occlude", "x.npz"], "--aug_occlude"), (T + ["--cfg2", "configs/demo_poco_pare.yaml", "--ckpt2", "x.pt"], "--cfg2"),
                        (T + ["--segm"], "--segm"), (T + ["--likelihood"], "--likelihood"), (["--tta_weight", "uniform"], "needs --tta"),
                        (["--tta", "flip,flip", "--crop", "dataset"], "twice"), (["--tta", "rot:200", "--crop", "dataset"], "180")):
        with pytest.raises(SystemExit) as e:                                     # before any GPU work, before the dataset file is looked at
            cli.main(cli.parse_args(base + flags))
        _one_sentence(str(e.value), word)
        assert "missing.npz" not in str(e.value), (flags, e.value)
    with pytest.raises(SystemExit, match="missing.npz"):                         # flags that may run get as far as the dataset file
        cli.main(cli.parse_args(base + T + ["--tta_weight", "uniform"]))


def test_demo_flags_parse_and_are_refused_where_they_cannot_work(tmp_path):
    import demo
    a = demo.parse_args(BASE)
    assert a.tta is None and a.tta_weight is None
    a = demo.parse_args(BASE + ["--tta", "flip", "--tta_weight", "uncert"])
    assert (a.tta, a.tta_weight) == ("flip", "uncert")
    T = ["--tta", "flip"]
    for flags, word in ((T + ["--mode", "video"], "--mode video"), (T + ["--mode", "directory"], "--mode directory"),
                        (T + ["--cfg2", "configs/demo_poco_pare.yaml", "--ckpt2", "x.pt"], "--cfg2"), (T + ["--occlusion_map"], "--occlusion_map"),
                        (T + ["--save_dataset", str(tmp_path / "d.npz")], "--save_dataset"), (T + ["--save_segm"], "--save_segm"),
                        (T + ["--mode", "video", "--gpus", "2"], "--mode video"), (["--tta_weight", "uniform"], "needs --tta"),
                        (["--tta", "scale:0"], "scale must be > 0")):
        with pytest.raises(SystemExit) as e:                                     # before any GPU work: no engine, no input folder needed
            demo.main(demo.parse_args(BASE + flags + ["--vid_file", str(tmp_path / "missing"), "--image_folder", str(tmp_path / "missing")]))
        _one_sentence(str(e.value), word)
    with pytest.raises(SystemExit, match="not found"):                           # flags that may run get as far as the input folder
        demo.main(demo.parse_args(BASE + T + ["--image_folder", str(tmp_path / "missing")]))


def test_flag_error_sentences():
    from types import SimpleNamespace as NS
    assert tta.flag_error(NS(tta=None, tta_weight=None), "eval") is None and tta.flag_error(NS(), "demo") is None
    assert tta.flag_error(NS(tta="flip", crop="dataset"), "eval") is None and tta.flag_error(NS(tta="flip", mode="folder", gpus=1), "demo") is None
    _one_sentence(tta.flag_error(NS(tta="flip", mode="folder", gpus=2), "demo"), "--gpus")
    _one_sentence(tta.flag_error(NS(tta="flip", mode="webcam", gpus=1), "demo"), "--mode webcam")
    _one_sentence(tta.flag_error(NS(tta="flip", crop="dataset", ckpt2="x.pt"), "eval"), "--cfg2")


def test_the_model_wrapper_refuses_what_it_does_not_offer():
    import torch

    class Fake:
        _finalized, max_batch = True, 8
        device = torch.device("cuda:0")
    views = tta.parse_views("flip,rot:15")
    m = tta.TTAModel(Fake(), views, "uniform")
    assert m.max_batch == 2 and m.K == 3 and m.table == [(0, 0.0), (1, 0.0), (0, 15.0)] and m.weight == "uniform"
    with pytest.raises(AttributeError, match="graph_forward"):
        m.graph_forward
    with pytest.raises(_lib.PocoHipError, match="want_segm"):
        m({}, want_segm=True)
    with pytest.raises(ValueError, match="weight"):
        tta.TTAModel(Fake(), views, "median")
    with pytest.raises(ValueError, match="identity first"):
        tta.TTAModel(Fake(), views[1:], "uncert")
    small = Fake()
    small.max_batch = 2
    with pytest.raises(_lib.PocoHipError, match="max_batch"):
        tta.TTAModel(small, views, "uncert")


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_c_abi_declares_the_entry_and_refuses_bad_arguments():
    from poco_amd import ops
    L = _lib.lib()
    assert "poco_op_tta_fuse" in _lib.header_symbols() and hasattr(L, "poco_op_tta_fuse")
    txt = _lib.HEADER.read_text()
    assert "#define POCO_ABI_VERSION 4" in txt and "#define POCO_TTA_MAX_VIEWS 8" in txt                  # additions only
    assert L.poco_abi_version() == 4
    fn = L.poco_op_tta_fuse
    fn.argtypes = ops.TTA_ARGTYPES
    MB = 1 << 26                                                     # fake device pointers, far enough apart not to overlap
    pose, var, betas, pose_out, var_out, spread, betas_out = (MB * i for i in range(1, 8))
    good = [(0, 1.0, 0.0), (1, 1.0, 0.0), (0, math.cos(0.3), math.sin(0.3))]

    def call(pose=pose, var=var, betas=betas, B=4, views=good, weight=1, pose_out=pose_out, var_out=var_out, spread=spread, betas_out=betas_out):
        return fn(pose, var, betas, B, ops.tta_views(views), weight, pose_out, var_out, spread, betas_out, 0, None)
    bad = [dict(pose=None), dict(var=None), dict(betas=None), dict(pose_out=None), dict(var_out=None), dict(spread=None), dict(betas_out=None),
           dict(views=good[:1]), dict(views=[]), dict(views=good + [(0, 0.0, 1.0)] * 6), dict(B=0), dict(B=-1), dict(B=(1 << 24) + 1),
           dict(weight=2), dict(weight=-1), dict(views=[good[0], (2, 1.0, 0.0)]), dict(views=[good[0], (-1, 1.0, 0.0)]),
           dict(views=[good[0], (0, float("nan"), 0.0)]), dict(views=[good[0], (0, 0.0, float("inf"))]), dict(views=[good[0], (0, 1.0, 1e-5)]),
           dict(views=[good[0], (0, 0.5, 0.5)]), dict(views=[(1, 1.0, 0.0), good[1]]), dict(views=[(0, 0.0, 1.0), good[1]]),
           dict(views=[(0, -1.0, 0.0), good[1]]), dict(pose_out=pose), dict(var_out=var), dict(betas_out=betas), dict(spread=var),
           dict(pose_out=pose + 4 * 216 * 5), dict(var_out=spread), dict(spread=spread + 0, var_out=spread + 4 * 24 * 3)]
    for kw in bad:
        assert call(**kw) == 1, kw
        assert "poco_op_tta_fuse" in L.poco_last_error().decode(), kw


def test_ops_tta_fuse_refuses_bad_arguments_without_a_gpu():
    """The wrapper's own checks come before any GPU work; host tensors are refused as such."""
    import torch
    from poco_amd import ops
    with pytest.raises(_lib.PocoHipError, match="tta_fuse.*CUDA"):
        ops.tta_fuse(torch.zeros(4, 24, 3, 3), torch.zeros(4, 24), torch.zeros(4, 10), [(0, 0.0), (1, 0.0)])
