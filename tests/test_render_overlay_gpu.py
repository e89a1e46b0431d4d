"""GPU: the wireframe pass and the keypoint discs of csrc/render.hip against their numpy contract (tests/render_overlay_np.py),
culling, depth, determinism, the untouched filled path, argument checks, and demo.py --wireframe / --draw_keypoints /
--render_crop end to end.

The comparison rule is the filled path's (tests/test_render_gpu.py): where both cover a pixel the bytes differ by at most one level
and at least 99.9 % are equal (the device's powf is not libm's); pixels neither covers keep the frame's bytes; coverage is
identical except at pixels the restatement itself flags as within 1e-3 of a decision, whose share of the line fragments must stay
under 1 % (measured when the test was written: at most 0.70 % over the twelve cases below)."""
import ctypes as C
import functools
import json

import numpy as np
import pytest
import torch

from poco_amd import _lib, render
from poco_amd._lib import PocoHipError
from tests import render_np, render_overlay_np as ov
from tests.test_render_gpu import _assets, _scene

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(kind, H, W, side):
    """(frame, verts [P,V,3], faces, cams, colours, materials, rotation, restatement image, restatement info) - computed once."""
    rot = render.side_rotation() if side else None
    r = np.random.default_rng(H + W)
    frame = r.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "mesh":
        frame, verts, faces, cams, cols = _scene(2, H, W, seed=3)
    else:
        v, faces = ov.tilted_quad() if kind == "quad" else ov.tetrahedron()
        verts = v[None]
        cams = np.array([[1.2 * H / W, 1.2, 0.07, -0.04]], np.float32)
        cols = np.array([render.vertex_color(np.full(24, 0.37, np.float32), "hrnet_w48_cls-cliff")], np.float32)
    mats = np.zeros(len(verts), np.float32)
    info = {}
    ref = ov.wire_np(frame, verts, faces, cams, cols, mats, rot, info=info)
    return frame, verts, faces, cams, cols, mats, rot, ref, info


def _compare(got, cov_g, frame, ref, info):
    cov_r = info["ids"] >= 0
    fragile = info["fragile"]
    assert cov_r.sum() > 20, "scene draws too little to test anything"
    assert info["fragile_fragments"] < 0.01 * info["fragments"], (info["fragile_fragments"], info["fragments"])
    assert not (cov_g ^ cov_r)[~fragile].any()
    both = cov_g & cov_r & ~fragile
    d = np.abs(got.astype(int) - ref.astype(int)).max(-1)
    assert d[both].max() <= 1
    assert (d[both] == 0).mean() >= 0.999
    assert np.array_equal(got[~cov_g & ~cov_r], frame[~cov_g & ~cov_r])


@pytest.mark.parametrize("H,W", [(48, 64), (81, 97)])
@pytest.mark.parametrize("side", [False, True])
@pytest.mark.parametrize("kind", ["quad", "tetra", "mesh"])
def test_wireframe_matches_numpy_contract(cuda, kind, H, W, side):
    frame, verts, faces, cams, cols, mats, rot, ref, info = _case(kind, H, W, side)
    R = render.Renderer(faces, verts.shape[1], cuda)
    cnt = torch.zeros(H, W, dtype=torch.int32, device=cuda)
    got = R.render(torch.from_numpy(frame.copy()).to(cuda), verts, cams, cols, mats, rot, frag_count=cnt, wireframe=True).cpu().numpy()
    _compare(got, cnt.cpu().numpy() > 0, frame, ref, info)


def _ids_of(R, H, W, verts, cam, dev, wireframe=True, colour=(1, 1, 1), material=1):
    ids = torch.zeros(H, W, dtype=torch.int32, device=dev)
    frame = torch.zeros(H, W, 3, dtype=torch.uint8, device=dev)
    out = R.render(frame, verts[None], [cam], [colour], [material], wireframe=wireframe, ids=ids).cpu().numpy()
    return out, ids.cpu().numpy()


def test_integer_scenes_are_exact(cuda):
    H = W = 32
    for verts, faces, cam, _ in (ov.int_tetrahedron(H, W), ov.int_quads(H, W)):
        info = {}
        ref = ov.wire_np(np.zeros((H, W, 3), np.uint8), verts[None], faces, [cam], [[1, 1, 1]], [1], info=info)
        out, ids = _ids_of(render.Renderer(faces, verts.shape[0], cuda), H, W, verts, cam, cuda)
        assert np.array_equal(ids, info["ids"])                   # coverage and the winning (triangle, edge) ids
        assert np.abs(out.astype(int) - ref.astype(int)).max() <= 1 and (ids >= 0).sum() > 40


def test_culling_and_depth(cuda):
    H = W = 32
    verts, faces, cam, (cc, cr) = ov.int_quads(H, W)
    # what each quad alone would put at the crossing: the flat near quad shades brighter than the tilted far one (157 against
    # 141 for this grey, which does not saturate)
    blank, grey = np.zeros((H, W, 3), np.uint8), (0.3, 0.3, 0.3)
    alone = [ov.wire_np(blank, verts[None], faces[k:k + 2], [cam], [grey], [0])[cr, cc].astype(int) for k in (0, 2)]
    assert alone[0].min() > 0 and alone[1].min() > 0 and (alone[0] - alone[1]).min() > 10
    for order in ([0, 1, 2, 3], [2, 3, 0, 1]):                    # the near quad's triangles first, then last
        f = np.ascontiguousarray(faces[order])
        out, ids = _ids_of(render.Renderer(f, 8, cuda), H, W, verts, cam, cuda, colour=grey, material=0)
        assert ids[cr, cc] >= 0 and f[ids[cr, cc] >> 2].max() <= 3, "the far quad's edge won the crossing"
        assert np.abs(out[cr, cc].astype(int) - alone[0]).max() <= 1, "the crossing does not carry the nearer edge's colour"
    vb, fb, cam, _ = ov.int_quads(H, W, back=True)
    out, ids = _ids_of(render.Renderer(fb, 8, cuda), H, W, vb, cam, cuda)
    assert (ids < 0).all() and not out.any()                      # a back-facing quad draws nothing
    # the hook on the filled path: the winning triangle (two pixels inside the near quad's corner, over the far quad), -1 outside
    out, ids = _ids_of(render.Renderer(faces, 8, cuda), H, W, verts, cam, cuda, wireframe=False)
    assert ids[cr + 2, cc - 2] in (0, 1) and ids[cr + 2, cc + 3] in (2, 3) and ids[0, 0] == -1


def test_flags_zero_is_the_filled_call_and_wireframe_is_deterministic(cuda):
    H, W = 81, 97
    frame, verts, faces, cams, cols, mats, rot, _, _ = _case("mesh", H, W, False)
    R = render.Renderer(faces, verts.shape[1], cuda)
    dv = torch.from_numpy(verts).to(cuda)
    prm = R.params(cams, cols, mats)
    stream = C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)
    a, b = torch.from_numpy(frame.copy()).to(cuda), torch.from_numpy(frame.copy()).to(cuda)
    L = _lib.lib()
    _lib.check(L.poco_renderer_render(R._h, a.data_ptr(), H, W, dv.data_ptr(), 2, prm.data_ptr(), None, None, stream))
    _lib.check(L.poco_renderer_render_ex(R._h, b.data_ptr(), H, W, dv.data_ptr(), 2, prm.data_ptr(), None, None, 0, stream))
    assert torch.equal(a, b) and not np.array_equal(a.cpu().numpy(), frame)
    w = [R.render(torch.from_numpy(frame.copy()).to(cuda), dv, cams, cols, mats, wireframe=True).cpu().numpy() for _ in range(2)]
    assert np.array_equal(w[0], w[1]) and not np.array_equal(w[0], a.cpu().numpy())


def _disc_points():
    """49 * 2 points on 64 x 48: random ones with a margin beyond the frame, then border, corner, negative-fraction,
    overlapping and not-a-number ones."""
    r = np.random.default_rng(11)
    pts = r.uniform([-8, -8], [72, 56], (98, 2)).astype(np.float32)
    pts[:14] = [[0, 0], [63, 47], [63.9, 0.2], [-0.9, 20.5], [30, -0.99], [-1.5, -1.5], [64, 24], [31.5, 48], [-4, 24], [20, 52],
                [40, 20], [42, 21], [41, 19], [np.nan, 5]]
    rgb = r.integers(0, 256, (98, 3), dtype=np.uint8)
    return pts, rgb


def test_discs_match_numpy_contract(cuda):
    H, W = 48, 64
    frame = np.random.default_rng(2).integers(0, 256, (H, W, 3), dtype=np.uint8)
    pts, rgb = _disc_points()
    ref = ov.draw_discs_np(frame, pts, rgb, 4)
    got = [render.draw_discs(torch.from_numpy(frame.copy()).to(cuda), pts, rgb).cpu().numpy() for _ in range(2)]
    assert np.array_equal(got[0], ref) and np.array_equal(got[0], got[1])
    assert (ref != frame).any(-1).sum() > 1000
    for r in (0, 1, 8):                                           # the ends of the table
        assert np.array_equal(render.draw_discs(torch.from_numpy(frame.copy()).to(cuda), pts, rgb, r).cpu().numpy(),
                              ov.draw_discs_np(frame, pts, rgb, r))
    assert np.array_equal(render.draw_discs(torch.from_numpy(frame.copy()).to(cuda), np.zeros((0, 2)), np.zeros((0, 3))).cpu().numpy(),
                          frame)


def test_bad_arguments_are_errors(cuda):
    v, f = render_np.icosphere(1)
    R = render.Renderer(f, v.shape[0], cuda)
    frame = torch.zeros(16, 16, 3, dtype=torch.uint8, device=cuda)
    dv = torch.from_numpy(v[None] * 0.5).to(cuda)
    prm = R.params([[1, 1, 0, 0]], [[1, 1, 1]], [1])
    L = _lib.lib()
    ex = lambda *a: L.poco_renderer_render_ex(*a, None)                                                  # noqa: E731
    good = (R._h, frame.data_ptr(), 16, 16, dv.data_ptr(), 1, prm.data_ptr(), None, None)
    assert ex(*good, 1) == 0
    for k in (0, 1, 4, 6):                                        # handle, frame, vertices, parameters
        bad = list(good)
        bad[k] = None
        assert ex(*bad, 1) == 1, k
    for flags in (4, 8, 1 << 31, 2):                              # unknown bits; the id hook without its buffer
        assert ex(*good, flags) == 1, flags
    with pytest.raises(PocoHipError, match="r <= 8"):
        render.draw_discs(frame, [[3, 3]], [[1, 1, 1]], 9)
    with pytest.raises(PocoHipError):
        render.draw_discs(frame, [[3, 3]], [[1, 1, 1]], -1)
    dd = L.poco_renderer_draw_discs
    assert dd(frame.data_ptr(), 16, 16, dv.data_ptr(), dv.data_ptr(), -1, 4, None) == 1
    assert dd(None, 16, 16, dv.data_ptr(), dv.data_ptr(), 1, 4, None) == 1
    assert dd(frame.data_ptr(), 16, 16, None, dv.data_ptr(), 1, 4, None) == 1
    assert dd(frame.data_ptr(), 16, 16, dv.data_ptr(), None, 1, 4, None) == 1
    # a face count over the wireframe limit: the filled call is still accepted, the wireframe call is refused before any work
    many = np.tile(np.array([[0, 1, 2]], np.int32), (render.MAX_WIRE_FACES + 1, 1))
    big = render.Renderer(many, 3, cuda)
    tri = np.array([[[-0.5, -0.5, 0], [0.5, -0.5, 0], [0, 0.5, 0]]], np.float32)
    frame.zero_()
    with pytest.raises(PocoHipError, match="2\\^20"):
        big.render(frame, tri, [[1, 1, 0, 0]], [[1, 1, 1]], [1], wireframe=True)
    assert not frame.cpu().numpy().any()
    # the handles still work
    R.render(frame, dv, [[1, 1, 0, 0]], [[1, 1, 1]], [1], wireframe=True)
    assert frame.cpu().numpy().any()


# ---- demo.py end to end ------------------------------------------------------------------------------------------------
BACKBONE = "resnet50-cliff"


def _folder_kp(j2d):
    """tester.py:324-328 restated: SMPL joints [25:] white, then OpenPose joints [:25] black."""
    j = np.asarray(j2d, np.float32)[:, :2]
    return np.concatenate([j[25:], j[:25]]), np.concatenate([np.full((24, 3), 255, np.uint8), np.zeros((25, 3), np.uint8)])


def _expect(img, faces, verts, cams, var, kps, wire, dev, numpy=True, backbone=BACKBONE):
    """(the restatement's picture, the pixels it flags as fragile, the device renderer's picture): person by person, the mesh and
    then that person's discs.  numpy=False leaves the restatement's picture out (the frame is returned in its place)."""
    ref, gpu = img.copy(), torch.from_numpy(img.copy()).to(dev)
    fragile = np.zeros(img.shape[:2], bool)
    R = render.Renderer(faces, verts.shape[1], dev)
    for i in range(len(verts)):
        col = render.vertex_color(var[i], backbone)
        if not numpy:
            pass
        elif wire:
            info = {}
            ref = ov.wire_np(ref, verts[i][None], faces, [cams[i]], [col], [0], info=info)
            fragile |= info["fragile"]
        else:
            ref = render_np.render_np(ref, verts[i][None], faces, [cams[i]], [col], [0])
        R.render(gpu, verts[i][None], [cams[i]], [col], [0], wireframe=wire)
        if kps is not None:
            ref = ov.draw_discs_np(ref, kps[i][0], kps[i][1], 4) if numpy else ref
            render.draw_discs(gpu, kps[i][0], kps[i][1])
    return ref, fragile, gpu.cpu().numpy()


def _check_picture(png, ref, fragile, gpu):
    assert np.array_equal(png, gpu)                               # the demo's bytes are the library's, exactly
    d = np.abs(png.astype(int) - ref.astype(int)).max(-1)
    assert d[~fragile].max() <= 1 and (d[~fragile] == 0).mean() >= 0.999


def _stamps(points, shape):
    """bool [H,W]: the pixels the r = 4 stamps of `points` cover (the restatement's, from the truncated positions)."""
    return ov.draw_discs_np(np.zeros(shape + (3,), np.uint8), points, [[1, 1, 1]], 4).any(-1)


def _check_folder_discs(png, j2d):
    """The discs of the LAST person drawn (nothing is painted after them): the OpenPose joints [:25] black on top, the SMPL joints
    [25:] white wherever no black stamp covers them - on the canvas, and overlapping, so that the order is really tested."""
    j = np.asarray(j2d, np.float32)[:, :2]
    black, white = _stamps(j[:25], png.shape[:2]), _stamps(j[25:], png.shape[:2])
    assert black.sum() > 61 and (white & ~black).sum() > 20 and (white & black).sum() > 20, (black.sum(), white.sum())
    assert (png[black] == 0).all(), "a black OpenPose stamp is missing or covered"
    assert (png[white & ~black] == 255).all(), "a white SMPL stamp is missing"


@pytest.fixture(scope="module")
def folder_case(tmp_path_factory):
    from PIL import Image
    tmp = tmp_path_factory.mktemp("overlay")
    ckpt, smpl, faces = _assets(tmp)
    imgs = tmp / "imgs"
    imgs.mkdir()
    r = np.random.default_rng(0)
    frames = {f"im{i}.png": r.integers(0, 256, (120, 160, 3), dtype=np.uint8) for i in range(2)}
    for n, fr in frames.items():
        Image.fromarray(fr).save(imgs / n)
    dets = {"im0.png": [[80, 60, 75, 75], [40, 50, 45, 60]], "im1.png": [[100, 50, 60, 80]]}
    (tmp / "dets.json").write_text(json.dumps(dets))
    common = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(ckpt), "--mode", "folder", "--image_folder", str(imgs),
              "--batch_size", "4", "--smpl", str(smpl), "--detections", str(tmp / "dets.json")]
    return tmp, common, frames, dets, faces


def _run(tmp, common, name, flags):
    import demo
    demo.main(demo.parse_args(common + ["--output_folder", str(tmp / name)] + flags))
    return tmp / name / "imgs_"


def test_demo_folder_wireframe_keypoints(folder_case, cuda):
    from PIL import Image
    tmp, common, frames, dets, faces = folder_case
    out = _run(tmp, common, "wk", ["--render", "--wireframe", "--draw_keypoints"])
    for n, fr in frames.items():
        res = dict(np.load(out / (n[:-4] + "_poco.npz")))
        png = np.asarray(Image.open(out / "poco_results" / (n[:-4] + ".png")))
        assert png.shape == (120, 160, 3)
        kps = [_folder_kp(j) for j in res["smpl_joints2d"]]
        _check_picture(png, *_expect(fr, faces, res["verts"], res["orig_cam"], res["var"], kps, True, cuda))
        _check_folder_discs(png, res["smpl_joints2d"][-1])
        # the wireframe itself: pixels that are neither the input's nor a disc's
        discs = _stamps(np.concatenate([j[:, :2] for j in res["smpl_joints2d"]]), png.shape[:2])
        assert ((png != fr).any(-1) & ~discs).sum() > 100, "no mesh line was drawn"


def test_demo_folder_render_crop(folder_case, cuda):
    from PIL import Image
    from oracle import crop_np
    tmp, common, frames, dets, faces = folder_case
    out = _run(tmp, common, "crop", ["--render", "--wireframe", "--draw_keypoints", "--render_crop"])
    for n, fr in frames.items():
        res = dict(np.load(out / (n[:-4] + "_poco.npz")))
        png = np.asarray(Image.open(out / "poco_results" / (n[:-4] + ".png")))
        assert png.shape == (224, 224, 3)
        box = np.asarray(dets[n][0], np.float32)
        canvas = crop_np.crop_u8_np(fr, box[None], 1.0, 224)[0]
        s, tx, ty = res["pred_cam"][0]
        j = np.asarray(res["smpl_joints2d"][0], np.float64)[:, :2]             # original-image pixels -> crop pixels
        jc = np.stack([112.0 + (j[:, 0] - float(box[0])) * (224 / float(box[2])),
                       112.0 + (j[:, 1] - float(box[1])) * (224 / float(box[3]))], 1).astype(np.float32)
        ref, fragile, gpu = _expect(canvas, faces, res["verts"][:1], np.array([[s, s, tx, ty]], np.float32), res["var"][:1],
                                    [_folder_kp(jc)], True, cuda)
        _check_picture(png, ref, fragile, gpu)
        # the discs sit at the CROP coordinates of the joints (all 49 on the canvas here), not at their image coordinates
        assert ((jc >= 4) & (jc < 220)).all(), "a joint of the synthetic run left the canvas: the position check would see less"
        _check_folder_discs(png, jc)
        at_image_coords = _stamps(j.astype(np.float32)[:25], (224, 224)) & ~_stamps(jc, (224, 224))
        assert at_image_coords.sum() > 61 and not (png[at_image_coords] == 0).all()
        untouched = (png == ref).all(-1) & (ref == canvas).all(-1)
        assert untouched.mean() > 0.5 and np.array_equal(png[untouched], canvas[untouched])   # the canvas is the crop's bytes


def test_demo_folder_without_new_flags_is_the_parent_path(folder_case, cuda):
    """--render alone: the picture is poco_renderer_render's (Renderer.render without wireframe calls exactly that), all people
    in one call, as before."""
    from PIL import Image
    tmp, common, frames, dets, faces = folder_case
    out = _run(tmp, common, "plain", ["--render"])
    for n, fr in frames.items():
        res = dict(np.load(out / (n[:-4] + "_poco.npz")))
        png = np.asarray(Image.open(out / "poco_results" / (n[:-4] + ".png")))
        R = render.Renderer(faces, res["verts"].shape[1], cuda)
        prm = R.params(res["orig_cam"], [render.vertex_color(v, BACKBONE) for v in res["var"]], np.zeros(len(res["var"])))
        dv = torch.from_numpy(res["verts"]).to(cuda)
        frame = torch.from_numpy(fr.copy()).to(cuda)
        _lib.check(_lib.lib().poco_renderer_render(R._h, frame.data_ptr(), 120, 160, dv.data_ptr(), len(res["var"]), prm.data_ptr(),
                                                   None, None, C.c_void_p(torch.cuda.current_stream(cuda).cuda_stream)))
        assert np.array_equal(png, frame.cpu().numpy()) and (png != fr).any()


def test_demo_video_keypoints(tmp_path, cuda):
    """POCO-PARE: its joints are crop-normalised, so video mode's conversion puts them inside the boxes, on the frame.  (Video
    mode converts unconditionally, as the reference does at tester.py:458-462, which sends CLIFF's image-space joints far off any
    frame; that run would show no disc.)"""
    from PIL import Image
    import demo
    backbone = "hrnet_w32-pare"
    ckpt, smpl, faces = _assets(tmp_path, backbone)
    fr_dir = tmp_path / "frames"
    fr_dir.mkdir()
    r = np.random.default_rng(1)
    frames = [r.integers(0, 256, (120, 160, 3), dtype=np.uint8) for _ in range(5)]
    for i, fr in enumerate(frames):
        Image.fromarray(fr).save(fr_dir / f"{i:06d}.png")
    tracks = {"0": {"bbox": [[80, 60, 80, 80]] * 5, "frames": [0, 1, 2, 3, 4]}, "1": {"bbox": [[50, 70, 60, 70]] * 2, "frames": [1, 2]}}
    (tmp_path / "tracks.json").write_text(json.dumps(tracks))
    demo.main(demo.parse_args(["--cfg", "configs/demo_poco_pare.yaml", "--ckpt", str(ckpt), "--mode", "video", "--vid_file",
                               str(fr_dir), "--batch_size", "5", "--smpl", str(smpl), "--tracking", str(tmp_path / "tracks.json"),
                               "--output_folder", str(tmp_path / "out"), "--render", "--draw_keypoints"]))
    b = dict(np.load(tmp_path / "out" / "frames_" / "poco_results.npz"))
    green = np.array([0, 255, 0])
    for i, fr in enumerate(frames):
        png = np.asarray(Image.open(tmp_path / "out" / "frames_" / "tmp_images_output" / f"{i:06d}.png"))
        assert png.shape == (120, 160, 3)
        people = [p for p in ("0", "1") if i in tracks[p]["frames"]]
        k = {p: tracks[p]["frames"].index(i) for p in people}
        res = {key: np.stack([b[f"{p}/{key}"][k[p]] for p in people]) for key in ("verts", "orig_cam", "var", "smpl_joints2d")}
        order = render.video_order(res["orig_cam"])
        joints = [np.asarray(res["smpl_joints2d"][o], np.float32)[:, :2] for o in order]
        kps = [(j, np.tile(np.array([[0, 255, 0]], np.uint8), (49, 1))) for j in joints]
        _, _, gpu = _expect(fr, faces, res["verts"][order], res["orig_cam"][order], res["var"][order], kps, False, cuda, numpy=False,
                            backbone=backbone)
        assert np.array_equal(png, gpu)
        # green discs at the truncated smpl_joints2d: every stamp pixel of the person painted last, and no green pixel that is
        # not a stamp pixel of somebody in this frame
        last, anyone = _stamps(joints[-1], png.shape[:2]), _stamps(np.concatenate(joints), png.shape[:2])
        assert last.sum() > 61, "the joints of the synthetic run are not on the frame"
        assert (png[last] == green).all()
        assert not ((png == green).all(-1) & ~anyone & ~(fr == green).all(-1)).any()
