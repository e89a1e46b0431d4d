"""CPU: the visibility contract without a GPU - the numpy restatement (tests/visibility_np.py) on cases counted on paper, the
finish-time statistics of poco_amd/visibility.py against their restatement (NaN handling included), eval.py's flag refusals and
missing-key exits, the new C entries declared and exported, and every argument error refused before any GPU work (the device pointers
are fake and never dereferenced)."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

from poco_amd import _lib, datacrop, ops, visibility
from tests import visibility_np
from tests.test_occlude_cpu import bad_occ_calls, good_occ_inputs, occ_call_args

ROOT = Path(__file__).resolve().parent.parent
FAKE, NULL = C.c_void_p(4096), C.c_void_p(0)
NEW = ["poco_op_part_visibility", "poco_op_part_visibility_scratch_bytes", "poco_dataset_crop_occ_mask"]


def _counts(mesh, margin, mask=None):
    v, f, p = mesh.arrays()
    assert mesh.exact()
    return visibility_np.part_visibility(v[None], np.zeros((1, 3), np.float32), f, p, mesh.focal, mesh.res, margin, mask)[0]


# ---- the restatement on paper ----------------------------------------------------------------------------------------------------------
def test_right_triangle_on_an_8x8_frame():
    """Legs of 6 pixels from (0.25, 0.25): a centre (c + .5, r + .5) is inside iff c + r <= 5 -> 21 pixels, none on an edge."""
    m = visibility_np.Mesh(8)
    m.tri((0.25, 0.25), (6.25, 0.25), (0.25, 6.25), 5)
    for margin in (0, 3, 8):
        c = _counts(m, margin)
        assert c[5].tolist() == [21, 21, 21, 21] and not np.delete(c, 5, 0).any(), margin
    # the other winding covers the same pixels
    m2 = visibility_np.Mesh(8)
    m2.tri((0.25, 0.25), (0.25, 6.25), (6.25, 0.25), 5)
    assert np.array_equal(_counts(m2, 3), _counts(m, 3))
    # moved 4 pixels to the left: columns -4 .. 1; in the frame stay c' + r <= 5 with c' = c + 4 >= 4 -> (4,0), (4,1), (5,0)
    s = visibility_np.Mesh(8)
    s.tri((-3.75, 0.25), (2.25, 0.25), (-3.75, 6.25), 7)
    assert _counts(s, 4)[7].tolist() == [21, 3, 3, 3]
    assert _counts(s, 0)[7].tolist() == [3, 3, 3, 3]                           # the window is the frame: the body outside is not counted
    assert _counts(s, 2)[7].tolist() == [3 + 4 + 3, 3, 3, 3]                   # columns -2, -1 hold c' = 2, 3: r <= 3 and r <= 2
    # a mask over the column 0 hides (4,0) and (4,1) of the three front pixels
    mask = np.zeros((1, 8, 8), np.uint8)
    mask[0, :, 0] = 1
    assert _counts(s, 4, mask)[7].tolist() == [21, 3, 3, 1]


def test_occlusion_shared_edges_back_faces_and_degenerate_faces():
    m = visibility_np.Mesh(8)
    # part 1: a square [1, 5]^2 of two triangles whose diagonal runs through the centres (1.5, 1.5) .. (4.5, 4.5): 16 centres, each once
    a, b, c, d = m.vert(1, 1), m.vert(5, 1), m.vert(5, 5), m.vert(1, 5)
    m.tri(a, b, c, 1)
    m.tri(a, c, d, 1)
    # part 1 again, behind itself with the other winding: total is not doubled
    m.tri((1, 1, 128.0), (1, 5, 128.0), (5, 5, 128.0), 1)
    # part 2 behind part 1, covering [0, 8) x [1, 3): 16 centres, 8 of them behind the square
    e, f, g, h = m.vert(0, 1, 96.0), m.vert(8, 1, 96.0), m.vert(8, 3, 96.0), m.vert(0, 3, 96.0)
    m.tri(e, f, g, 2)
    m.tri(e, g, h, 2)
    # faces that cover nothing: behind the near plane, NaN, zero area, a repeated index
    m.tri((0, 0), (8, 0), (4, 8, 0.05), 3)
    m.tri((0, 0), (8, 0), (float("nan"), 8), 4)
    m.tri((1, 1), (3, 3), (5, 5), 6)
    m.faces.append([a, a, b])
    m.parts.append(8)
    c_ = _counts(m, 2)
    assert c_[1].tolist() == [16, 16, 16, 16]
    assert c_[2].tolist() == [16, 16, 8, 8]
    assert not c_[[3, 4, 6, 8]].any() and c_.sum() == 16 * 4 + 16 * 2 + 8 * 2
    v, fc, p = m.arrays()
    bad = np.concatenate([fc, [[0, 1, 99]]]).astype(np.int32)                  # an index outside [0, V) covers nothing either
    got = visibility_np.part_visibility(v[None], np.zeros((1, 3), np.float32), bad, np.append(p, 9), m.focal, 8, 2)[0]
    assert np.array_equal(got, c_)
    # equal depth: face 0 (part 10) and face 1 (part 11) coincide; the lower face index is in front everywhere
    q = visibility_np.Mesh(8)
    q.tri((0.25, 0.25), (6.25, 0.25), (0.25, 6.25), 10)
    q.tri((0.25, 0.25), (6.25, 0.25), (0.25, 6.25), 11)
    cq = _counts(q, 0)
    assert cq[10].tolist() == [21, 21, 21, 21] and cq[11].tolist() == [21, 21, 0, 0]


# ---- statistics ------------------------------------------------------------------------------------------------------------------------
def _made_up(n=40, seed=2):
    r = np.random.default_rng(seed)
    total = r.integers(1, 400, (n, 24))
    area = (total * r.uniform(0, 1, (n, 24))).astype(np.int64)
    front = (area * r.uniform(0, 1, (n, 24))).astype(np.int64)
    seen = (front * r.uniform(0, 1, (n, 24))).astype(np.int64)
    counts = np.stack([total, area, front, seen], -1).astype(np.int32)
    counts[3, 5] = 0                                                            # a part outside the window: every ratio NaN
    counts[4, 6] = (50, 0, 0, 0)                                               # wholly in the margin: vis 0, vis_frame 0, the others NaN
    counts[5, 7] = (50, 20, 0, 0)                                              # wholly hidden by the body: vis_obj NaN
    counts[:, 9] = 0                                                            # a joint never in the window
    counts[6, 8] = (10, 10, 10, 10)                                            # fully visible: the last bin is closed
    vis = visibility_np.ratios(counts)["vis"]
    u = np.nan_to_num(1 - vis, nan=0.5) * 0.7 + r.uniform(0, 0.3, (n, 24))
    e = np.nan_to_num(1 - vis, nan=0.5) * 0.3 + r.uniform(0, 1.0, (n, 24))
    return counts, u.astype(np.float32), e.astype(np.float32)


def test_statistics_equal_their_restatement_and_leave_out_what_is_undefined():
    counts, u, e = _made_up()
    for bins in (5, 2, 20):
        got, want = visibility.statistics(counts, u.reshape(-1), e.reshape(-1), bins), visibility_np.statistics(counts, u, e, bins)
        for k in visibility.COMPONENTS:
            assert np.array_equal(got[k], visibility_np.ratios(counts)[k], equal_nan=True), k
            assert got["corr"][k] == pytest.approx(want["corr"][k], abs=1e-12), k
        assert (got["valid"], got["invalid"]) == (want["valid"], want["invalid"]) == (40 * 24 - 41, 41)
        assert np.allclose(got["mean"], want["mean"], rtol=0, atol=1e-12, equal_nan=True) and np.isnan(got["mean"][9])
        assert np.allclose(got["corr_joint"], want["corr_joint"], rtol=0, atol=1e-12, equal_nan=True) and np.isnan(got["corr_joint"][9]).all()
        assert got["mean_all"] == pytest.approx(want["mean_all"], abs=1e-12)
        assert got["corr_err"] == pytest.approx(want["corr_err"], abs=1e-12)
        assert np.allclose(got["bins"], want["bins"], rtol=0, atol=1e-12, equal_nan=True) and got["bins"].shape == (bins, 3)
        assert got["bins"][:, 0].sum() == got["valid"]
    st = visibility.statistics(counts, u, e, 5)
    assert np.isnan(st["vis"][3, 5]) and st["vis"][4, 6] == 0 and st["vis_frame"][4, 6] == 0 and np.isnan(st["vis_self"][4, 6])
    assert st["vis_self"][5, 7] == 0 and np.isnan(st["vis_obj"][5, 7]) and st["vis"][6, 8] == 1
    assert st["corr"]["vis"][0] > 0.5 and st["corr"]["vis"][1] > 0.5           # the made-up uncertainty follows 1 - vis
    # vis is the product of its three components where all are defined
    ok = np.isfinite(st["vis_obj"])
    assert np.allclose(st["vis"][ok], (st["vis_frame"] * st["vis_self"] * st["vis_obj"])[ok], rtol=1e-12, atol=0)
    res = visibility.result_arrays(counts, st, 112)
    assert res["vis_counts"].dtype == np.int32 and res["vis_summary"].shape == (len(visibility.SUMMARY_NAMES),)
    assert res["vis_summary"][0] == st["mean_all"] and res["vis_summary"][-4:].tolist() == [40 * 24 - 41, 41, 112, 5]
    lines = visibility.report_lines(res)
    assert lines[0].startswith("Visibility (window margin 112 px): mean ") and "(41 without a pixel in the window)" in lines[0]
    assert sum(line.startswith("Corr(1 - vis") for line in lines) == 7 and len(lines) == 10 + 5
    assert sum(l.startswith("  [") for l in lines) == 5 and lines[-1].startswith("  [0.80, 1.00]: ")
    # everything undefined: no statistic, no exception
    none = visibility.statistics(np.zeros((2, 24, 4), np.int32), np.ones((2, 24)), np.ones((2, 24)))
    assert none["valid"] == 0 and np.isnan(none["mean_all"]) and np.isnan(none["corr"]["vis"]).all() and not none["bins"][:, 0].any()
    # ties share their ranks; a constant side has no correlation
    assert visibility.average_ranks([3, 1, 3, 2]).tolist() == [3.5, 1, 3.5, 2]
    assert visibility.spearman([1, 2, 3, 4], [1, 8, 27, 64]) == pytest.approx(1.0) and np.isnan(visibility.pearson([1, 1, 1], [1, 2, 3]))
    with pytest.raises(ValueError, match="2..20"):
        visibility.statistics(counts, u, e, 21)


# ---- flags -----------------------------------------------------------------------------------------------------------------------------
def _cli():
    spec = importlib.util.spec_from_file_location("poco_eval_cli_visibility", ROOT / "eval.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_flag_refusals_and_missing_keys(tmp_path):
    ev = _cli()
    base = ["--cfg", "configs/demo_poco_cliff.yaml", "--ckpt", "k", "--j_regressor", "j", "--dataset", str(tmp_path / "ds.npz"),
            "--smpl", str(tmp_path / "smpl.npz")]
    a = ev.parse_args(base)
    assert a.visibility is False and a.vis_margin is None and a.vis_bins is None and visibility.flag_error(a) is None
    V = base + ["--visibility"]
    for extra, words in ((["--cfg2", "c", "--ckpt2", "k"], "reads one model's outputs: it cannot be combined with --cfg2 / --ckpt2"),
                         (["--tta", "flip", "--crop", "dataset"], "reads one forward's outputs: it cannot be combined with --tta"),
                         (["--sequences"], "--sequences cannot be combined with --visibility"),
                         (["--rank_metrics"], "ranks the records of the plain evaluation: it cannot be combined with --visibility"),
                         (["--likelihood"], "cannot be combined with --likelihood"),
                         (["--vis_bins", "1"], "--vis_bins must be in 2..20"), (["--vis_bins", "21"], "--vis_bins must be in 2..20"),
                         (["--vis_margin", "-1"], "--vis_margin must be in 0..res")):
        with pytest.raises(SystemExit) as e:
            ev.main(ev.parse_args(V + extra))
        assert words in str(e.value.code), (extra, e.value.code)
    for extra in (["--vis_bins", "5"], ["--vis_margin", "10"]):
        with pytest.raises(SystemExit, match="needs --visibility"):
            ev.main(ev.parse_args(base + extra))
    # what composes is not refused by the flag check
    for extra in (["--segm"], ["--aug_flip"], ["--augment"], ["--aug_occlude", "o.npz"], ["--crop", "dataset"], ["--vis_bins", "20", "--vis_margin", "0"]):
        assert visibility.flag_error(ev.parse_args(V + extra)) is None, extra
    # missing keys are named, as --segm names them
    np.savez(tmp_path / "ds.npz", imgname=np.array(["a"]), center=np.zeros((1, 2)), scale=np.ones(1), pose=np.zeros((1, 72)))
    with pytest.raises(SystemExit) as e:
        ev.check_visibility(ev.parse_args(V))
    assert "--visibility needs ['shape', 'part'] in the dataset" in str(e.value.code)
    with pytest.raises(ValueError, match=r"\['pose', 'shape', 'part'\]"):
        visibility.check_dataset_keys(["imgname"])
    np.savez(tmp_path / "ds.npz", imgname=np.array(["a"]), center=np.zeros((1, 2)), scale=np.ones(1), pose=np.zeros((1, 72)),
             shape=np.zeros((1, 10)), part=np.zeros((1, 24, 3)))
    with pytest.raises(SystemExit, match="body-model file not found"):
        ev.check_visibility(ev.parse_args(V))
    np.savez(tmp_path / "smpl.npz", lbs_weights=np.zeros((4, 24), np.float32))
    with pytest.raises(SystemExit, match="faces"):
        ev.check_visibility(ev.parse_args(V))
    with pytest.raises(SystemExit, match="part mapping not found"):
        ev.check_visibility(ev.parse_args(V + ["--part_mapping", str(tmp_path / "nope.npy")]))
    np.savez(tmp_path / "smpl.npz", lbs_weights=np.zeros((4, 24), np.float32), faces=np.zeros((1, 3), np.int32))
    ev.check_visibility(ev.parse_args(V))
    ev.check_visibility(ev.parse_args(base))                                   # without the flag nothing is looked at


# ---- the C entries ---------------------------------------------------------------------------------------------------------------------
def test_new_entries_are_declared_exported_and_check_their_arguments():
    L = _lib.lib()
    syms = _lib.header_symbols()
    for s in NEW:
        assert s in syms and hasattr(L, s), s
    assert "#define POCO_ABI_VERSION 4" in _lib.HEADER.read_text()             # additions only: the ABI version is not bumped
    msg = lambda: L.poco_last_error().decode()   # noqa: E731
    f = C.c_float(5000.0)
    good_parts = np.array([0, 23, 5, 7], np.uint8)

    def vis(v=FAKE, B=1, V=10, t=FAKE, fc=FAKE, F=4, fp=FAKE, hfp=good_parts, focal=f, res=224, margin=112, mask=NULL, scratch=FAKE, out=FAKE):
        h = NULL if hfp is None else C.c_void_p(hfp.ctypes.data)
        return L.poco_op_part_visibility(v, B, V, t, fc, F, fp, h, focal, res, margin, mask, scratch, out, NULL)
    for kw in (dict(v=NULL), dict(t=NULL), dict(fc=NULL), dict(fp=NULL), dict(scratch=NULL), dict(out=NULL), dict(B=0), dict(B=65536), dict(V=0),
               dict(F=0), dict(res=0), dict(res=4097), dict(margin=-1), dict(margin=225), dict(res=32, margin=33), dict(focal=C.c_float(0.0)),
               dict(focal=C.c_float(float("nan"))), dict(focal=C.c_float(float("inf"))), dict(scratch=C.c_void_p(4100)),
               dict(out=C.c_void_p(4098)), dict(hfp=np.array([0, 24, 5, 7], np.uint8)), dict(hfp=np.array([0, 1, 2, 255], np.uint8))):
        assert vis(**kw) == 1 and "poco_op_part_visibility" in msg(), kw
    assert "face 1 has part 24" in (vis(hfp=np.array([0, 24, 5, 7], np.uint8)), msg())[1]
    sb = ops.part_visibility_scratch_bytes
    assert sb(1, 224, 112) == 224 * 224 * 8 + 448 * 448 * 4 and sb(3, 17, 0) == 3 * (17 * 17 * 8 + 17 * 17 * 4)
    assert sb(2, 33, 33) == 2 * (33 * 33 * 8 + 99 * 99 * 4) and sb(65535, 4096, 4096) == 65535 * (4096 * 4096 * 8 + 12288 * 12288 * 4)
    assert sb(0, 224, 0) == sb(1, 0, 0) == sb(1, 4097, 0) == sb(1, 224, -1) == sb(1, 224, 225) == sb(65536, 224, 0) == 0

    # poco_dataset_crop_occ_mask: everything poco_dataset_crop_occ refuses, and a null mask
    Lm = datacrop._bind_occ()
    _, params, table, recs = good_occ_inputs()
    base = occ_call_args(params, table, recs)

    def mask_call(kw):
        p = lambda a: NULL if a is None else (a if isinstance(a, C.c_void_p) else C.c_void_p(a.ctypes.data))   # noqa: E731
        return Lm.poco_dataset_crop_occ_mask(kw["images"], kw["hw"], kw["n_images"], kw["d_params"], p(kw["h"]), kw["N"], kw["res"], 1, kw["atlas"],
                                             kw["texels"], kw["d_table"], p(kw["h_table"]),
                                             len(kw["h_table"]) if kw.get("n_occ") is None else kw["n_occ"], kw["d_occ"], p(kw["h_occ"]),
                                             kw["out"], kw["cover"], kw.get("mask", FAKE), NULL)
    for label, ch in bad_occ_calls(params, table, recs) + [("mask", dict(mask=NULL))]:
        assert mask_call(dict(base, **ch)) == 1, label
        assert "poco_dataset_crop_occ_mask" in msg(), label
    with pytest.raises(ValueError, match="want_mask needs occlusion"):
        datacrop.dataset_crop([None], [0], params[:1], 32, want_mask=True)
