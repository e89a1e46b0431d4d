"""CPU: the track stitcher without a GPU.  The restatement tests/stitch_np.py on an example worked out by hand, its line fit against
numpy.polyfit and its assignment against an exhaustive search; the decision margins of every seeded scene and the recorded rounding
floor; the C ABI's declaration and argument checks of poco_op_track_stitch (fake pointers, refused before any GPU work);
ops.track_stitch's refusals; poco_amd/stitch.py's packing, box interpolation and row splicing with the restatement in the operator's
place; demo.py's flags; min_frames of sort.build_tracks and tester.load_tracking."""
import ctypes as C
import json
import pickle

import numpy as np
import pytest

from poco_amd import _lib, sort, stitch
from tests import stitch_np, stitch_scenes


def _run(sc, **over):
    return stitch_np.track_stitch(sc["clip_offsets"], sc["frag_offsets"], sc["frames"], sc["boxes"], sc["betas"], sc["var"],
                                  **{**sc["params"], **over})


# ---- the restatement ------------------------------------------------------------------------------------------------------------------
def _hand_example():
    """Three fragments, every weight exactly 1 (var = u_ref = 0.25), boxes 20 x 40:
      A  frames 0, 1, 2   cx = 10, 12, 14   cy = 50   beta_0 = 0.5
      B  frames 5, 6, 7   cx = 20, 22, 24   cy = 50   beta_0 = 0.5      (A walking on at 2 pixels a frame)
      C  frames 5, 6      cx = 100, 100     cy = 50   beta_0 = -0.5     (somebody else)
    A's tail fit of cx: t = -2, -1, 0, tbar = -1, qbar = 12, Stt = 2, Stq = (-1)(-2) + 0 + (1)(2) = 4: velocity 2, state 12 + 2 = 14.
    B's head fit: t = 0, 1, 2, tbar = 1, qbar = 22, velocity 2, state 22 - 2 = 20.  D = 5 - 2 = 3, h = 1.5: pa.cx = 14 + 3 = 17,
    pb.cx = 20 - 3 = 17, so c_m = 0; the mean shapes are equal, so c_s = 0: gain(A -> B) = 1.
    A -> C: pb.cx = 100, dx = -83, c_m = sqrt(83^2 / 1600) / (0.5 sqrt 3) = 2.396 > 1; c_s = sqrt(1 / 10) / sqrt(0.05^2) = 6.32 > 1.
    B -> anything and C -> anything: D < 1.  So A -> B is the only link: chains {A, B} = 0 and {C} = 1."""
    frames = np.array([0, 1, 2, 5, 6, 7, 5, 6], np.int32)
    cx = [10, 12, 14, 20, 22, 24, 100, 100]
    boxes = np.array([[x, 50.0, 20.0, 40.0] for x in cx], np.float64)
    betas = np.zeros((8, 10), np.float32)
    betas[:6, 0], betas[6:, 0] = 0.5, -0.5
    return dict(clip_offsets=None, frag_offsets=[0, 3, 6, 8], frames=frames, boxes=boxes, betas=betas, var=np.full((8, 24), 0.25, np.float32))


def test_restatement_on_the_hand_example():
    out = stitch_np.track_stitch(**_hand_example(), u_ref=0.25)
    assert out["succ"].tolist() == [1, -1, -1] and out["pred"].tolist() == [-1, 0, -1] and out["chain"].tolist() == [0, 0, 1]
    assert out["gain"].tolist() == [1.0, 0.0, 0.0] and out["status"].tolist() == [0] and out["total"].tolist() == [1.0]
    A, B, Cc = out["desc"]
    l40 = np.log(40.0)
    assert A.tolist() == [0.5] + [0.0] * 9 + [0.0, 3.0, 3.0, 3.0, 14.0, 50.0, l40, 2.0, 0.0, 0.0, 10.0, 50.0, l40, 2.0, 0.0, 0.0, 0.0, 2.0]
    assert B[14:].tolist() == [24.0, 50.0, l40, 2.0, 0.0, 0.0, 20.0, 50.0, l40, 2.0, 0.0, 0.0, 5.0, 7.0]
    assert Cc[0] == -0.5 and Cc[13] == 2.0 and Cc[14:].tolist() == [100.0, 50.0, l40, 0.0, 0.0, 0.0, 100.0, 50.0, l40, 0.0, 0.0, 0.0, 5.0, 6.0]
    g, cm, cs, D = stitch_np.pair_gain(A, Cc, 30, 0.5, 1.0, 0.05, 1.0, np.float64)
    assert g == 0.0 and D == 3 and cm == pytest.approx(83.0 / 40.0 / (0.5 * np.sqrt(3.0)), rel=1e-12) and cs == pytest.approx(np.sqrt(0.1) / 0.05, rel=1e-12)
    # max_gap = 1: D = 3 > 2, nothing is linked; one fragment alone; a clip without fragments
    assert stitch_np.track_stitch(**_hand_example(), u_ref=0.25, max_gap=1)["succ"].tolist() == [-1, -1, -1]
    ex = _hand_example()
    one = stitch_np.track_stitch(None, [0, 3], ex["frames"][:3], ex["boxes"][:3], ex["betas"][:3], ex["var"][:3])
    assert one["succ"].tolist() == [-1] and one["chain"].tolist() == [0]
    assert stitch_np.track_stitch([0, 0], [0], ex["frames"][:0], ex["boxes"][:0], ex["betas"][:0], ex["var"][:0])["status"].tolist() == [0]


def test_tree_sum_and_weights():
    v = [np.float64(x) for x in np.random.default_rng(0).normal(0, 1, 1000)]
    assert stitch_np.tree_sum(v, np.float64) == pytest.approx(float(np.sum(v)), abs=1e-12)
    assert stitch_np.tree_sum(v[:1], np.float64) == v[0] and stitch_np.tree_sum([], np.float64) == 0.0
    # one row with var = 1e6 weighs (0.3 / 1e6)^2 = 9e-14 of a row with var = 0.3: the mean shape does not follow its betas
    sc = stitch_scenes.scenes()["outlier_var"]
    out = _run(sc)
    clean = np.delete(sc["betas"][:20].astype(np.float64), 7, 0)
    assert sc["var"][7, 0] == 1e6 and (sc["betas"][7] == 5.0).all()
    assert np.abs(out["desc"][0, :10] - clean.mean(0)).max() < 0.02 and np.abs(out["desc"][0, :10] - sc["betas"][:20].mean(0)).max() > 0.2
    assert out["succ"].tolist() == [1, -1]


def test_line_fit_against_polyfit():
    r = np.random.default_rng(1)
    for m in (2, 3, 8, 32):
        t = np.sort(r.choice(np.arange(-60, 1), m, replace=False))
        q = [np.float64(v) for v in 300.0 + 2.5 * t + r.normal(0, 1.0, m)]
        state, vel = stitch_np.line_fit(t.tolist(), q, np.float64)
        slope, icpt = np.polyfit(t.astype(np.float64), np.asarray(q), 1)
        assert vel == pytest.approx(slope, rel=1e-9, abs=1e-11) and state == pytest.approx(icpt, rel=1e-10)
    assert stitch_np.line_fit([0], [np.float64(7.5)], np.float64) == (7.5, 0.0)                    # one row: no velocity
    assert stitch_np.line_fit([3, 3], [np.float64(1.0), np.float64(3.0)], np.float64) == (2.0, 0.0)  # equal t: no velocity, the mean


def test_assignment_against_brute_force():
    r = np.random.default_rng(2)
    for n in (1, 2, 3, 4, 5):
        for _ in range(20):
            G = r.random((n, n)) * (r.random((n, n)) < 0.6)                                          # zeros: pairs that are no links
            np.fill_diagonal(G, 0.0)
            total, col = stitch_np.assign(G)
            best, bcol = stitch_np.brute_assign(G)
            assert total == pytest.approx(best, abs=1e-12)
            linked = [c for c in col if c >= 0]
            assert len(set(linked)) == len(linked) and all(G[i][c] > 0 for i, c in enumerate(col) if c >= 0)
    assert stitch_np.chains_of([2, -1, 1, -1], [-1, 2, 0, -1]) == [0, 0, 0, 1]


def test_scenes_cover_the_shapes_and_link_as_designed():
    sc = stitch_scenes.scenes()
    out = {n: _run(s) for n, s in sc.items()}
    links = lambda n: out[n]["succ"].tolist()                                   # noqa: E731
    assert links("single") == [-1] and links("empty_clip") == [1, -1, -1] and sc["empty_clip"]["clip_offsets"].tolist() == [0, 2, 2, 3]
    assert links("gap_1") == [1, -1] and links("gap_edge") == [1, -1] and links("gap_over") == [-1, -1]
    assert out["gap_1"]["margin_gap"].tolist() == [30] and out["gap_edge"]["margin_gap"].tolist() == [0] and out["gap_over"]["margin_gap"].tolist() == [1]
    assert links("short") == [1, -1, 0] and out["short"]["chain"].tolist() == [0, 0, 0] and (out["short"]["desc"][0, 17:20] == 0).all()
    assert links("fit_1") == [1, -1] and links("fit_32") == [1, -1] and (out["fit_1"]["desc"][:, 17:20] == 0).all()
    for T in (63, 64, 65, 1000):
        assert links(f"rows_{T}") == [1, -1] and out[f"rows_{T}"]["desc"][:, 13].tolist() == [T, T]
    assert links("crossing") == [3, 2, -1, -1]
    assert links("shape_on") == [3, 2, -1, -1] and links("shape_off") == [2, 3, -1, -1]                # the links differ with the shape term
    assert links("chain3") == [-1, 2, 0] and out["chain3"]["chain"].tolist() == [0, 0, 0] and out["chain3"]["pred"].tolist() == [2, -1, 1]
    assert links("overlap") == [-1, -1] and out["overlap"]["chain"].tolist() == [0, 1]
    G = out["greedy"]["G"][0]
    assert G[0, 2] == G.max() and G[1, 3] == 0 and links("greedy") == [3, 2, -1, -1]                   # not the greedy choice
    assert out["greedy"]["total"][0] > G[0, 2] + 0.2
    crowd = out["crowd256"]
    assert len(crowd["succ"]) == 256 and crowd["succ"][:128].tolist() == list(range(255, 127, -1)) and (crowd["succ"][128:] == -1).all()
    assert crowd["chain"][:128].tolist() == list(range(128))


def test_every_scene_has_decision_margins():
    """Where the margins exceed 1e-9, two fp64 implementations of the contract take the same discrete decisions; D is an integer."""
    for name, sc in stitch_scenes.scenes().items():
        out = _run(sc)
        ma, mg = float(out["margin_assign"].min()), float(out["margin_gate"].min())
        print(f"stitch {name}: margin_assign {ma:.3e}, margin_gate {mg:.3e}, margin_gap {int(out['margin_gap'].min())}")
        assert ma > 1e-9 and mg > 1e-9, name
        assert out["margin_gap"].dtype == np.int64
    tie = _run(stitch_scenes.tie_scene())
    assert tie["margin_assign"].min() == 0.0 and tie["total"][0] > 0.9


def test_recorded_rounding_floor_is_the_measured_one():
    """FLOOR of tests/stitch_scenes.py (the GPU test allows 16 x it) is what float64 against numpy.longdouble gives here, with the
    same discrete outputs; where long double is no wider than double the difference is 0 and only that is checked."""
    worst = 0.0
    for name, sc in stitch_scenes.scenes().items():
        a, b = _run(sc), _run(sc, dtype=np.longdouble)
        assert all(np.array_equal(a[k], b[k]) for k in ("succ", "pred", "chain", "status")), name
        for k in ("desc", "gain"):
            if a[k].size:
                worst = max(worst, float(np.abs((a[k] - b[k]) / (1 + np.abs(b[k]))).max()))
    print(f"stitch_np float64 against longdouble: largest |difference| / (1 + |value|) of desc and gain {worst:.3e}")
    assert worst <= stitch_scenes.FLOOR * 1.001
    if np.finfo(np.longdouble).eps < 1e-18:
        assert worst >= stitch_scenes.FLOOR * 0.99


# ---- the C ABI -------------------------------------------------------------------------------------------------------------------
def test_c_abi_declares_exports_and_checks_its_arguments():
    L = _lib.lib()
    assert "poco_op_track_stitch" in _lib.header_symbols() and hasattr(L, "poco_op_track_stitch")
    txt = _lib.HEADER.read_text()
    assert "#define POCO_STITCH_MAX_FRAGS 256" in txt and "#define POCO_STITCH_DESC 28" in txt and "POCO_STITCH_SCRATCH_DOUBLES(P)" in txt
    fake, null = C.c_void_p(4096), C.c_void_p(0)

    def call(co=fake, fo=fake, frames=fake, boxes=fake, betas=fake, var=fake, Cn=2, P=5, N=90, max_gap=30, fit_len=8, u_ref=0.3,
             motion_tol=0.5, shape_tol=1.0, shape_floor=0.05, shape_w=1.0, scratch=fake, succ=fake, pred=fake, chain=fake, gain=fake,
             desc=fake, status=fake):
        return L.poco_op_track_stitch(co, fo, frames, boxes, betas, var, C.c_int64(Cn), C.c_int64(P), C.c_int64(N), max_gap, fit_len,
                                      C.c_double(u_ref), C.c_double(motion_tol), C.c_double(shape_tol), C.c_double(shape_floor),
                                      C.c_double(shape_w), scratch, succ, pred, chain, gain, desc, status, null)
    nan, inf = float("nan"), float("inf")
    for kw in (dict(Cn=0), dict(Cn=-1), dict(P=-1), dict(N=-1), dict(Cn=(1 << 24) + 1), dict(P=(1 << 22) + 1), dict(N=(1 << 24) + 1),
               dict(N=1 << 40), dict(co=null), dict(fo=null), dict(status=null), dict(frames=null), dict(boxes=null), dict(betas=null),
               dict(var=null), dict(scratch=null), dict(succ=null), dict(pred=null), dict(chain=null), dict(gain=null), dict(desc=null),
               dict(co=null, P=0, N=0), dict(max_gap=-1), dict(fit_len=0), dict(fit_len=33), dict(u_ref=0.0), dict(u_ref=nan),
               dict(motion_tol=0.0), dict(motion_tol=-1.0), dict(motion_tol=inf), dict(shape_tol=0.0), dict(shape_tol=nan),
               dict(shape_floor=0.0), dict(shape_floor=inf), dict(shape_w=-0.5), dict(shape_w=nan), dict(shape_w=inf)):
        assert call(**kw) == 1, kw
        assert "poco_op_track_stitch" in L.poco_last_error().decode(), kw


def test_ops_track_stitch_refuses_bad_arguments_without_a_gpu():
    import torch
    from poco_amd import ops
    N = 8
    ok = dict(clip_offsets=[0, 1, 3], frag_offsets=[0, 3, 6, 8], frames=torch.tensor([0, 1, 2, 5, 6, 7, 5, 6], dtype=torch.int32),
              boxes=torch.tensor([[10.0, 10.0, 4.0, 8.0]] * N, dtype=torch.float64), betas=torch.zeros((N, 10)), var=torch.full((N, 24), 0.1))
    put = lambda k, i, j, v: ok[k].clone().index_put((torch.tensor(i), torch.tensor(j)), torch.tensor(v, dtype=ok[k].dtype))   # noqa: E731
    many = 257
    crowd = dict(clip_offsets=[0, many], frag_offsets=list(range(many + 1)), frames=torch.zeros(many, dtype=torch.int32),
                 boxes=ok["boxes"][:1].repeat(many, 1), betas=torch.zeros((many, 10)), var=torch.full((many, 24), 0.1))
    for kw, word in ((dict(boxes=ok["boxes"].float()), "float64"), (dict(boxes=ok["boxes"][:, :3]), "[N,4]"), (dict(betas=ok["betas"][:, :9]), "[N,10]"),
                     (dict(var=ok["var"].double()), "float32"), (dict(frames=ok["frames"].long()), "int32"), (dict(betas=ok["betas"][:7]), "N = 8 rows"),
                     (dict(frag_offsets=[0, 6, 3, 8]), "not monotone at fragment 1"), (dict(frag_offsets=[0, 3, 3, 8]), "fragment 1 is empty"),
                     (dict(frag_offsets=[1, 3, 6, 8]), "start at 0"), (dict(frag_offsets=[0, 3, 6, 7]), "end at N"),
                     (dict(frag_offsets=[0.0, 3.0, 6.0, 8.0]), "integer"), (dict(clip_offsets=[0, 2, 1, 3]), "not monotone at clip 1"),
                     (dict(clip_offsets=[0, 1, 2]), "end at P"), (dict(clip_offsets=[0]), "C >= 1"), (crowd, "clip 0 holds 257"),
                     (dict(frames=torch.tensor([0, 1, 2, 5, 5, 7, 5, 6], dtype=torch.int32)), "fragment 1 do not increase strictly at row 4"),
                     (dict(frames=torch.tensor([0, 1, 2, 5, 6, 7, 6, 5], dtype=torch.int32)), "fragment 2"),
                     (dict(boxes=put("boxes", 4, 2, 0.0)), "fragment 1"), (dict(boxes=put("boxes", 7, 3, -1.0)), "fragment 2"),
                     (dict(boxes=put("boxes", 0, 0, float("nan"))), "fragment 0"), (dict(betas=put("betas", 3, 9, float("inf"))), "fragment 1: betas"),
                     (dict(var=put("var", 6, 0, float("nan"))), "fragment 2: var"), (dict(var=put("var", 2, 23, -0.1)), "fragment 0: var must be finite and >= 0"),
                     (dict(max_gap=-1), "max_gap"), (dict(max_gap=1.5), "max_gap"), (dict(fit_len=0), "fit_len"), (dict(fit_len=33), "fit_len"),
                     (dict(u_ref=0.0), "u_ref"), (dict(motion_tol=float("nan")), "motion_tol"), (dict(shape_tol=-1.0), "shape_tol"),
                     (dict(shape_floor=0.0), "shape_floor"), (dict(shape_w=-1.0), "shape_w"), (dict(shape_w=float("inf")), "shape_w"), ({}, "CUDA")):
        with pytest.raises(_lib.PocoHipError) as e:
            ops.track_stitch(**{**ok, **kw})
        assert "track_stitch" in str(e.value) and word in str(e.value), (kw, e.value)


# ---- poco_amd/stitch.py with the restatement in the operator's place -----------------------------------------------------------------
@pytest.fixture
def restated(monkeypatch):
    import torch
    from poco_amd import ops
    calls = []

    def fake(clip_offsets, frag_offsets, frames, boxes, betas, var, **kw):
        calls.append(kw)
        out = stitch_np.track_stitch(clip_offsets, np.asarray(frag_offsets), frames.numpy(), boxes.numpy(), betas.numpy(), var.numpy(), **kw)
        return {k: torch.from_numpy(np.asarray(out[k], np.float64 if k in ("gain", "desc") else np.int32))
                for k in ("succ", "pred", "chain", "gain", "desc", "status")}
    monkeypatch.setattr(ops, "track_stitch", fake)
    return calls


def _video():
    """The hand example as run_on_video leaves it: person '7' = A, '12' = B, '3' = C (so the sorted order is C, A, B), float32 boxes."""
    ex = _hand_example()
    tr, st = {}, {}
    for pid, lo, hi in (("12", 3, 6), ("7", 0, 3), ("3", 6, 8)):
        tr[pid] = {"bbox": ex["boxes"][lo:hi].astype(np.float32), "frames": ex["frames"][lo:hi].astype(np.int64)}
        st[pid] = {"pred_shape": ex["betas"][lo:hi], "var_pose": ex["var"][lo:hi],
                   "pred_cam": np.arange(lo, hi, dtype=np.float32)[:, None] * np.ones((1, 3), np.float32)}
    return tr, st


def test_packing_sorts_by_person_id():
    tr, st = _video()
    buf = stitch.pack_fragments(tr, st)
    assert buf["pids"] == ["3", "7", "12"] and buf["frag_offsets"].tolist() == [0, 2, 5, 8] and buf["frag_offsets"].dtype == np.int32
    assert buf["frames"].tolist() == [5, 6, 0, 1, 2, 5, 6, 7] and buf["frames"].dtype == np.int32
    assert buf["boxes"].dtype == np.float64 and buf["boxes"][:, 0].tolist() == [100, 100, 10, 12, 14, 20, 22, 24]
    assert buf["betas"].dtype == np.float32 and buf["betas"][:, 0].tolist() == [-0.5] * 2 + [0.5] * 6 and buf["var"].shape == (8, 24)
    assert stitch.pack_fragments({"b": tr["7"], "10": tr["3"], "9": tr["12"]}, {"b": st["7"], "10": st["3"], "9": st["12"]})["pids"] == ["9", "10", "b"]
    with pytest.raises(ValueError, match="'7'"):
        stitch.pack_fragments(tr, {**st, "7": {k: v[:2] for k, v in st["7"].items()}})


def test_interpolated_boxes():
    a, b = np.array([14.0, 50.0, 20.0, 40.0]), np.array([20.0, 56.0, 23.0, 43.0])
    mid = stitch.interpolate_boxes(a, b, 2, 5, np.float32)
    assert mid.dtype == np.float32 and mid.tolist() == [[16.0, 52.0, 21.0, 41.0], [18.0, 54.0, 22.0, 42.0]]
    assert stitch.interpolate_boxes(a, b, 2, 3, np.float64).shape == (0, 4)                         # D = 1: no hole
    third = stitch.interpolate_boxes(np.array([0.1, 0.0, 1.0, 1.0]), np.array([0.4, 0.0, 1.0, 1.0]), 0, 3, np.float64)
    assert third[0, 0] == 0.1 + (0.4 - 0.1) * (1.0 / 3.0) and third[1, 0] == 0.1 + (0.4 - 0.1) * (2.0 / 3.0)   # fp64, in this order


def test_stitch_tracks_merges_and_splices(restated):
    tr, st = _video()
    merged, mst, chains = stitch.stitch_tracks(tr, st, 8, device="cpu", u_ref=0.25)
    assert len(restated) == 1 and restated[0]["u_ref"] == 0.25 and restated[0]["max_gap"] == 30       # one call, the defaults filled in
    assert list(merged) == ["3", "7"] and [c["pid"] for c in chains] == ["3", "7"]                      # a chain takes its first fragment's id
    assert chains[1]["fragments"] == ["7", "12"] and chains[1]["gains"] == [1.0] and chains[0]["fragments"] == ["3"]
    assert merged["7"]["frames"].tolist() == list(range(8)) and merged["7"]["bbox"].dtype == np.float32
    assert merged["7"]["bbox"][:, 0].tolist() == [10, 12, 14, 16, 18, 20, 22, 24]
    assert chains[1]["stitch"].tolist() == [0, 0, 0, 1, 1, 0, 0, 0] and chains[1]["stitch"].dtype == np.uint8
    assert chains[1]["stitch_frag"].tolist() == [0, 0, 0, -1, -1, 1, 1, 1] and chains[1]["stitch_frag"].dtype == np.int32
    assert mst["7"]["pred_cam"][:, 0].tolist() == [0, 1, 2, 3, 4, 5]                                    # the own rows, in order
    gap = stitch.gap_tracks(merged, chains)
    assert list(gap) == ["7"] and gap["7"]["frames"].tolist() == [3, 4] and gap["7"]["bbox"][:, 0].tolist() == [16.0, 18.0]
    gst = {"7": {"pred_shape": np.ones((2, 10), np.float32), "var_pose": np.ones((2, 24), np.float32), "pred_cam": np.full((2, 3), -9.0, np.float32)}}
    full = stitch.merge_gap_rows(mst, gst, chains)
    assert full["7"]["pred_cam"][:, 0].tolist() == [0, 1, 2, -9, -9, 3, 4, 5] and full["7"]["pred_shape"].shape == (8, 10)
    assert full["3"] is mst["3"]
    with pytest.raises(ValueError, match="'7'"):
        stitch.merge_gap_rows(mst, {"7": {k: v[:1] for k, v in gst["7"].items()}}, chains)
    # the 25-frame rule on the chains
    k_tr, k_st, kept, dropped = stitch.drop_short(merged, full, chains, min_frames=8)
    assert list(k_tr) == ["7"] and list(k_st) == ["7"] and dropped == 1 and kept[0]["pid"] == "7"
    assert stitch.drop_short(merged, full, chains)[3] == 2 and stitch.MIN_NUM_FRAMES == 25
    assert stitch.summary_line(3, chains, 1) == "track_stitch: 3 fragments, 1 links, 2 chains, 2 gap rows, 1 chains dropped"
    # no fill: the ids are joined, the hole stays
    merged, mst, chains = stitch.stitch_tracks(tr, st, device="cpu", u_ref=0.25, fill=False)
    assert merged["7"]["frames"].tolist() == [0, 1, 2, 5, 6, 7] and chains[1]["stitch"].tolist() == [0] * 6 and not stitch.gap_tracks(merged, chains)
    assert chains[1]["stitch_frag"].tolist() == [0, 0, 0, 1, 1, 1]
    # nothing to join
    merged, _, chains = stitch.stitch_tracks(tr, st, device="cpu", u_ref=0.25, max_gap=1)
    assert list(merged) == ["3", "7", "12"] and all(len(c["fragments"]) == 1 for c in chains)
    with pytest.raises(ValueError, match="outside"):
        stitch.stitch_tracks(tr, st, 7, device="cpu")
    with pytest.raises(TypeError, match="iou"):
        stitch.stitch_tracks(tr, st, device="cpu", iou=0.3)


def test_written_chains_read_back(restated, tmp_path):
    from poco_amd.tester import load_tracking
    tr, st = _video()
    merged, _, _ = stitch.stitch_tracks(tr, st, device="cpu", u_ref=0.25)
    sort.write_tracking(str(tmp_path / "tracking_results_stitched.json"), merged)
    back = load_tracking(str(tmp_path / "tracking_results_stitched.json"))
    assert list(back) == list(merged)
    for pid in merged:
        assert np.array_equal(back[pid]["frames"], merged[pid]["frames"]) and np.array_equal(back[pid]["bbox"], merged[pid]["bbox"])


# ---- min_frames ------------------------------------------------------------------------------------------------------------------------
def test_min_frames_of_build_tracks_and_load_tracking(monkeypatch, tmp_path):
    import inspect

    import torch
    from poco_amd import ops
    from poco_amd.tester import load_tracking
    from tests import sort_np

    def fake(dets, frame_offsets, clip_offsets=None, **kw):
        out = sort_np.sort_tracks(dets.numpy(), np.asarray(frame_offsets), clip_offsets, **kw)
        return {k: torch.from_numpy(out[k]) for k in ("tracker", "id", "box", "count", "status")}
    monkeypatch.setattr(ops, "sort_tracks", fake)
    assert inspect.signature(sort.build_tracks).parameters["min_frames"].default == 25
    assert inspect.signature(load_tracking).parameters["min_frames"].default == 25
    names = [f"{i:06d}.png" for i in range(30)]
    dets = {n: [[100.0 + i, 100.0, 40.0, 80.0]] + ([[300.0, 100.0 + i, 40.0, 80.0]] if i < 10 else []) for i, n in enumerate(names)}
    assert list(sort.build_tracks(dets, names, device="cpu")) == ["0"]                                # the default: ten frames are dropped
    assert list(sort.build_tracks(dets, names, device="cpu", min_frames=5)) == ["0", "1"]
    assert list(sort.build_tracks(dets, names, device="cpu", min_frames=11)) == ["0"]
    raw = {"a": {"bbox": np.ones((30, 4), np.float32), "frames": np.arange(30)}, "b": {"bbox": np.ones((10, 4), np.float32), "frames": np.arange(10)}}
    with open(tmp_path / "tracking_results_bbox.pkl", "wb") as f:
        pickle.dump(raw, f)
    path = str(tmp_path / "tracking_results_bbox.pkl")
    assert list(load_tracking(path)) == ["a"] and list(load_tracking(path, min_frames=5)) == ["a", "b"]
    assert list(load_tracking(path, min_frames=11)) == ["a"]


# ---- demo.py's flags ----------------------------------------------------------------------------------------------------------------
BASE = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", "none.pt", "--mode", "video", "--vid_file", "none"]


def test_demo_flags_parse_and_conflicts_end_before_the_engine(tmp_path):
    import demo
    a = demo.parse_args(BASE)
    assert a.track_stitch is False and (a.stitch_max_gap, a.stitch_fit_len, a.stitch_motion_tol, a.stitch_shape_tol, a.stitch_shape,
                                        a.stitch_min_frag, a.stitch_no_fill) == (30, 8, 0.5, 1.0, 1.0, 5, False)
    assert a.stitch_max_gap == a.infill_max_gap and stitch.flag_error(a) is None
    a = demo.parse_args(BASE + ["--track_stitch", "--stitch_max_gap", "12", "--stitch_fit_len", "4", "--stitch_motion_tol", "0.25",
                                "--stitch_shape_tol", "2", "--stitch_shape", "0", "--stitch_min_frag", "3", "--stitch_no_fill"])
    assert stitch.flag_error(a) is None
    assert stitch.params_of(a) == {"max_gap": 12, "fit_len": 4, "motion_tol": 0.25, "shape_tol": 2.0, "shape_w": 0.0}
    on = ["--track_stitch"]
    folder = ["--cfg", "c.yaml", "--ckpt", "none.pt", "--mode", "folder", "--image_folder", "none"]
    for argv, word in ((BASE + ["--stitch_max_gap", "12"], "needs --track_stitch"), (BASE + ["--stitch_no_fill"], "needs --track_stitch"),
                       (BASE + ["--stitch_shape", "0"], "needs --track_stitch"), (folder + on, "--mode video"),
                       (BASE + on + ["--kp_refit", "1.0"], "--kp_refit"), (BASE + on + ["--tracking_method", "pose"], "keypoints"),
                       (BASE + on + ["--gpus", "2"], "--gpus"), (BASE + on + ["--save_dataset", "d.npz"], "--save_dataset"),
                       (BASE + on + ["--stitch_max_gap", "-1"], "--stitch_max_gap"), (BASE + on + ["--stitch_fit_len", "33"], "--stitch_fit_len"),
                       (BASE + on + ["--stitch_motion_tol", "0"], "--stitch_motion_tol"), (BASE + on + ["--stitch_shape_tol", "nan"], "--stitch_shape_tol"),
                       (BASE + on + ["--stitch_shape", "-1"], "--stitch_shape"), (BASE + on + ["--stitch_min_frag", "0"], "--stitch_min_frag")):
        msg = stitch.flag_error(demo.parse_args(argv))
        assert msg is not None and word in msg, (argv, msg)
    with pytest.raises(SystemExit, match="needs --track_stitch"):
        demo.main(demo.parse_args(BASE + ["--stitch_fit_len", "4"]))
    with pytest.raises(SystemExit, match="--gpus"):
        demo.main(demo.parse_args(BASE + on + ["--gpus", "2"]))
    # a keypoint track ends before the engine is built
    fr = tmp_path / "frames"
    fr.mkdir()
    kp = {"0": {"bbox": [[10.0, 10.0, 4.0, 8.0]] * 3, "frames": [0, 1, 2], "joints2d": np.ones((3, 25, 3)).tolist()}}
    (tmp_path / "kp.json").write_text(json.dumps(kp))
    with pytest.raises(SystemExit, match="joints2d"):
        demo.main(demo.parse_args(BASE[:-1] + [str(fr), "--track_stitch", "--tracking", str(tmp_path / "kp.json"),
                                              "--output_folder", str(tmp_path / "out")]))
    assert not (tmp_path / "out").exists()
    assert stitch.tracking_error({"0": {"bbox": np.ones((3, 4)), "frames": [0, 1, 2]}}) is None and stitch.tracking_error(None) is None
