"""GPU: the demo renderer (csrc/render.hip) against its numpy contract (tests/render_np.py), its fill rule, painter's order,
composite and argument checks, and demo.py --render end to end."""
import json

import numpy as np
import pytest
import torch

from poco_amd import render, synth
from poco_amd._lib import PocoHipError
from tests import render_np, util
from tests.test_render_cpu import grid_mesh

pytestmark = pytest.mark.gpu


def _scene(n, H, W, seed):
    """n overlapping deformed icospheres with their own weak-perspective cameras, colours and materials."""
    r = np.random.default_rng(seed)
    verts, faces = [], None
    cams, cols = [], []
    for i in range(n):
        v, faces = render_np.deformed_sphere(seed * 10 + i, subdiv=3, radius=0.5)
        verts.append(v)
        s = r.uniform(0.9, 1.4)
        cams.append([s * H / W, s, r.uniform(-0.4, 0.4), r.uniform(-0.3, 0.3)])
        cols.append(render.vertex_color(r.uniform(0, 1, 24).astype(np.float32), "hrnet_w48_cls-cliff"))
    frame = r.integers(0, 256, (H, W, 3), dtype=np.uint8)
    return frame, np.stack(verts), faces, np.array(cams, np.float32), np.array(cols, np.float32)


def _near_edge(vis, faces, verts, cams, H, W, rotation, tol=1e-3):
    """pixels whose centre lies within tol px of an edge of the triangle visible there (coverage may differ by rounding)."""
    near = np.zeros(H * W, bool)
    flat = vis.reshape(-1)
    hit = np.nonzero(flat != render_np.EMPTY)[0]
    P = verts.shape[0]
    pers = P - 1 - (flat[hit] >> np.uint64(54)).astype(np.int64)
    tri = (flat[hit] & np.uint64((1 << 22) - 1)).astype(np.int64)
    for p in range(P):
        col, row, _ = render_np.project(verts[p], cams[p], H, W, rotation)
        sel = pers == p
        pix, f = hit[sel], tri[sel]
        px, py = (pix % W) + 0.5, (pix // W) + 0.5
        idx = faces[f]
        for e in range(3):
            a, b = idx[:, e], idx[:, (e + 1) % 3]
            ax, ay, bx, by = col[a], row[a], col[b], row[b]
            L = np.hypot(bx - ax, by - ay) + 1e-12
            d = np.abs((bx - ax) * (py - ay) - (by - ay) * (px - ax)) / L
            near[pix[d < tol]] = True
    return near.reshape(H, W)


@pytest.mark.parametrize("H,W,n", [(240, 320, 2), (480, 640, 4)])
@pytest.mark.parametrize("side", [False, True])
@pytest.mark.parametrize("material", [render.MATERIAL_UNCERT, render.MATERIAL_PLAIN])
def test_render_matches_numpy_contract(cuda, H, W, n, side, material):
    frame, verts, faces, cams, cols = _scene(n, H, W, seed=H + n + side)
    rot = render.side_rotation() if side else None
    mats = np.full(n, material, np.float32)
    ref, vis_r = render_np.render_np(frame, verts, faces, cams, cols, mats, rot, return_vis=True)
    R = render.Renderer(faces, verts.shape[1], cuda)
    dev = torch.from_numpy(frame.copy()).to(cuda)
    cnt = torch.zeros(H, W, dtype=torch.int32, device=cuda)
    got = R.render(dev, torch.from_numpy(verts).to(cuda), cams, cols, mats, rot, frag_count=cnt).cpu().numpy()
    cov_g = cnt.cpu().numpy() > 0
    cov_r = vis_r != render_np.EMPTY
    near = _near_edge(vis_r, faces, verts, cams, H, W, rot)
    assert cov_r.sum() > 0.1 * H * W, "scene covers too little to test anything"
    assert not (cov_g ^ cov_r)[~near].any()
    both = cov_g & cov_r & ~near
    d = np.abs(got.astype(int) - ref.astype(int)).max(-1)
    assert d[both].max() <= 1
    assert (d[both] == 0).mean() >= 0.999
    assert np.array_equal(got[~cov_g & ~cov_r], frame[~cov_g & ~cov_r])


def test_render_grid_is_watertight(cuda):
    H, W = 32, 32
    verts, faces, cam, expect = grid_mesh(H, W)
    R = render.Renderer(faces, verts.shape[0], cuda)
    cnt = torch.zeros(H, W, dtype=torch.int32, device=cuda)
    frame = torch.zeros(H, W, 3, dtype=torch.uint8, device=cuda)
    R.render(frame, verts[None], [cam], [[1, 1, 1]], [render.MATERIAL_PLAIN], frag_count=cnt)
    c = cnt.cpu().numpy()
    assert np.array_equal(c, expect.astype(np.int32))         # exactly the analytic set, each pixel once


def test_painter_order_and_depth(cuda):
    H, W = 64, 64
    v, f = render_np.icosphere(2)
    R = render.Renderer(f, v.shape[0], cuda)
    red, blue = [1, 0, 0], [0, 0, 1]
    # two people on the same pixels; the later one sits farther away (q_z = -v_z more negative) and still covers the first
    near, far = v * 0.3 + np.float32([0, 0, -0.2]), v * 0.3 + np.float32([0, 0, 0.4])
    cam = [1.0, 1.0, 0.0, 0.0]
    frame = torch.zeros(H, W, 3, dtype=torch.uint8, device=cuda)
    out = R.render(frame, np.stack([near, far]), [cam, cam], [red, blue], [1, 1]).cpu().numpy()
    c = out[H // 2, W // 2]
    assert c[2] > c[0], c                                     # blue (the later person) on top
    frame.zero_()
    c = R.render(frame, np.stack([far, near]), [cam, cam], [blue, red], [1, 1]).cpu().numpy()[H // 2, W // 2]
    assert c[0] > c[2], c
    # inside one person the nearer surface wins, whatever the triangle order: a tilted far triangle (index 0) and a flat near
    # one (index 1) of one mesh shade differently; the GPU pixel must be the contract's, and the contract's must be the near one
    tris = np.array([[-0.8, -0.8, 0.26], [0.8, -0.8, 0.74], [0.0, 0.8, 0.5],          # v_z = 0.5 + 0.3 x: q_z ~ -0.5
                     [-0.5, -0.5, -0.3], [0.5, -0.5, -0.3], [0.0, 0.5, -0.3]], np.float32)   # q_z = 0.3
    for faces2 in (np.array([[0, 2, 1], [3, 5, 4]], np.int32), np.array([[3, 5, 4], [0, 2, 1]], np.int32)):
        R2 = render.Renderer(faces2, 6, cuda)
        frame = torch.zeros(H, W, 3, dtype=torch.uint8, device=cuda)
        got = R2.render(frame, tris[None], [cam], [render.GREY], [1]).cpu().numpy()[H // 2, W // 2]
        ref, vis = render_np.render_np(np.zeros((H, W, 3), np.uint8), tris[None], faces2, [cam], [render.GREY], [1],
                                       return_vis=True)
        near_f = int(np.nonzero(faces2[:, 0] == 3)[0][0])
        assert int(vis[H // 2, W // 2] & np.uint64((1 << 22) - 1)) == near_f
        only_far = render_np.render_np(np.zeros((H, W, 3), np.uint8), tris[None], faces2[[1 - near_f]], [cam], [render.GREY],
                                       [1])[H // 2, W // 2]
        assert not np.array_equal(only_far, ref[H // 2, W // 2])
        assert np.array_equal(got, ref[H // 2, W // 2])


def test_uncovered_bytes_and_determinism(cuda):
    H, W = 240, 320
    frame, verts, faces, cams, cols = _scene(3, H, W, seed=7)
    R = render.Renderer(faces, verts.shape[1], cuda)
    outs = []
    for _ in range(2):
        dev = torch.from_numpy(frame.copy()).to(cuda)
        cnt = torch.zeros(H, W, dtype=torch.int32, device=cuda)
        outs.append(R.render(dev, verts, cams, cols, np.zeros(3), frag_count=cnt).cpu().numpy())
        un = cnt.cpu().numpy() == 0
        assert un.any() and np.array_equal(outs[-1][un], frame[un])
    assert np.array_equal(outs[0], outs[1])


def test_bad_arguments_are_errors(cuda):
    v, f = render_np.icosphere(1)
    bad = f.copy()
    bad[3, 1] = v.shape[0]
    with pytest.raises(PocoHipError, match="outside"):
        render.Renderer(bad, v.shape[0], cuda)
    R = render.Renderer(f, v.shape[0], cuda)
    frame = torch.zeros(16, 16, 3, dtype=torch.uint8, device=cuda)
    P = render.MAX_PEOPLE + 1
    with pytest.raises(PocoHipError, match="P <= 1024"):
        R.render(frame, np.zeros((P, v.shape[0], 3), np.float32), np.ones((P, 4)), np.ones((P, 3)), np.zeros(P))
    # the handle still works afterwards
    R.render(frame, v[None] * 0.5, [[1, 1, 0, 0]], [[1, 1, 1]], [1])
    assert frame.cpu().numpy().any()


# ---- demo.py --render end to end -------------------------------------------------------------------------------------
def _assets(tmp_path, variant="resnet50-cliff"):
    w = util.synth_weights(variant)
    ckpt = tmp_path / "poco_synth.pt"
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, ckpt)
    smpl = synth.synth_smpl(7)
    # a triangle list over the synthetic body's vertices: strips through consecutive vertex indices
    smpl["faces"] = np.stack([np.arange(0, 3000), np.arange(1, 3001), np.arange(2, 3002)], 1).astype(np.int32)
    np.savez(tmp_path / "smpl.npz", **smpl)
    return ckpt, tmp_path / "smpl.npz", smpl["faces"]


def _expected(img, faces, res, sideview, side_bg, order=None, backbone="resnet50-cliff", dev=None):
    verts, cam, var = res["verts"], res["orig_cam"], res["var"]
    if order is not None:
        verts, cam, var = verts[order], cam[order], var[order]
    R = render.Renderer(faces, verts.shape[1], dev)
    frame = torch.from_numpy(img.copy()).to(dev)
    cols = np.array([render.vertex_color(v, backbone) for v in var], np.float32)
    out = R.render(frame.clone(), verts, cam, cols, np.zeros(len(cam))).cpu().numpy()
    if sideview:
        side = torch.full_like(frame, side_bg)
        s = R.render(side, verts, cam, cols, np.zeros(len(cam)), render.side_rotation()).cpu().numpy()
        out = np.concatenate([out, s], 1)
    return out


def test_demo_folder_render(tmp_path, cuda):
    from PIL import Image
    import demo
    ckpt, smpl, faces = _assets(tmp_path)
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    r = np.random.default_rng(0)
    frames = {f"im{i}.png": r.integers(0, 256, (240, 320, 3), dtype=np.uint8) for i in range(2)}
    for n, fr in frames.items():
        Image.fromarray(fr).save(imgs / n)
    dets = {"im0.png": [[160, 120, 150, 150], [80, 100, 90, 120]], "im1.png": [[200, 100, 120, 160]]}
    (tmp_path / "dets.json").write_text(json.dumps(dets))
    common = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(ckpt), "--mode", "folder", "--image_folder", str(imgs),
              "--batch_size", "4", "--smpl", str(smpl), "--detections", str(tmp_path / "dets.json")]
    demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "plain")]))
    demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "rend"), "--render", "--sideview"]))
    for n, fr in frames.items():
        a = dict(np.load(tmp_path / "plain" / "imgs_" / (n[:-4] + "_poco.npz")))
        b = dict(np.load(tmp_path / "rend" / "imgs_" / (n[:-4] + "_poco.npz")))
        assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
        png = np.asarray(Image.open(tmp_path / "rend" / "imgs_" / "poco_results" / (n[:-4] + ".png")))
        assert png.shape == (240, 640, 3)
        exp = _expected(fr, faces, b, True, 255, dev=cuda)
        assert np.array_equal(png, exp)
        assert (png[:, :320] != fr).any(), "nothing was drawn"
    assert not (tmp_path / "plain" / "imgs_" / "poco_results").exists()


def test_demo_video_render(tmp_path, cuda):
    from PIL import Image
    import demo
    ckpt, smpl, faces = _assets(tmp_path)
    fr_dir = tmp_path / "frames"
    fr_dir.mkdir()
    r = np.random.default_rng(1)
    frames = [r.integers(0, 256, (120, 160, 3), dtype=np.uint8) for _ in range(3)]
    for i, fr in enumerate(frames):
        Image.fromarray(fr).save(fr_dir / f"{i:06d}.png")
    tracks = {"0": {"bbox": [[80, 60, 80, 80]] * 3, "frames": [0, 1, 2]}, "1": {"bbox": [[50, 70, 60, 70]] * 2, "frames": [1, 2]}}
    (tmp_path / "tracks.json").write_text(json.dumps(tracks))
    common = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(ckpt), "--mode", "video", "--vid_file", str(fr_dir),
              "--batch_size", "5", "--smpl", str(smpl), "--tracking", str(tmp_path / "tracks.json")]
    demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "plain")]))
    demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "rend"), "--render"]))
    a = dict(np.load(tmp_path / "plain" / "frames_" / "poco_results.npz"))
    b = dict(np.load(tmp_path / "rend" / "frames_" / "poco_results.npz"))
    assert a.keys() == b.keys() and all(np.array_equal(a[k], b[k]) for k in a)
    log = (tmp_path / "rend" / "frames_" / "uncertainty.log").read_text().splitlines()
    assert len(log) == 5 and all(ln.startswith("img_f:") and " person:0" in ln and " var:" in ln for ln in log)
    for i, fr in enumerate(frames):
        png = np.asarray(Image.open(tmp_path / "rend" / "frames_" / "tmp_images_output" / f"{i:06d}.png"))
        assert png.shape == (120, 160, 3)
        people = [p for p in ("0", "1") if i in tracks[p]["frames"]]
        k = {p: tracks[p]["frames"].index(i) for p in people}
        res = {key: np.stack([b[f"{p}/{key}"][k[p]] for p in people]) for key in ("verts", "orig_cam", "var")}
        order = render.video_order(res["orig_cam"])
        assert np.array_equal(png, _expected(fr, faces, res, False, 0, order=order, dev=cuda))
