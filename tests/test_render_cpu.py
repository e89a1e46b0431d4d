"""CPU: the host side of the demo renderer - jet LUT, get_vertex_colors restatement, the numpy contract's projection against
the reference's literal matrices, the C ABI's declarations and argument checks, and the demo CLI's new flags."""
import numpy as np
import pytest

from poco_amd import render
from tests import render_np


def test_jet_lut_matches_matplotlib():
    cm = pytest.importorskip("matplotlib.cm")
    import matplotlib
    jet = matplotlib.colormaps["jet"] if hasattr(matplotlib, "colormaps") else cm.get_cmap("jet")
    lut = render.jet_lut()
    assert lut.shape == (256, 3)
    ref = jet(np.arange(256))[:, :3]
    assert np.array_equal(lut, ref)
    # the index rule: trunc(x * 256) clamped, for float32 values as Normalize hands them over
    xs = np.float32([-0.5, 0.0, 1e-3, 0.25, 0.5, 0.5 - 2 ** -10, 0.7, 0.99, 1.0, 1.5, 7.0])
    for x in xs:
        assert np.array_equal(render.jet(x), np.asarray(jet(x))[:3]), x


def _ref_vertex_color(var, backbone):
    """renderer.py:193-224 for one person (every vertex gets the same label), with matplotlib, quantised as trimesh stores it."""
    cm = pytest.importorskip("matplotlib.cm")
    from matplotlib import colors
    import matplotlib
    jet = matplotlib.colormaps["jet"] if hasattr(matplotlib, "colormaps") else cm.get_cmap("jet")
    lab = np.asarray(var, np.float32).copy()
    vmax, thr = 1, 0.40
    if "cliff" in backbone:
        if lab[0] > 2 * thr:
            vmax = lab[0]
        lab[:] = lab[0]
    else:
        if lab[0] > thr:
            vmax = lab[0]
        lab[:] = lab[:].mean()
    c = np.asarray(jet(colors.Normalize(vmin=0, vmax=vmax)(lab[0])))[:3]
    return np.round(c * 255) / 255


@pytest.mark.parametrize("backbone", ["hrnet_w48_cls-cliff", "hrnet_w32-pare"])
def test_vertex_color_thresholds(backbone):
    r = np.random.default_rng(3)
    for v0 in (0.05, 0.39, 0.41, 0.79, 0.81, 1.7):
        var = r.uniform(0.0, 0.9, 24).astype(np.float32)
        var[0] = v0
        got = render.vertex_color(var, backbone)
        assert np.array_equal(got, _ref_vertex_color(var, backbone)), (backbone, v0)
    # both sides of each threshold by hand
    lo, hi = np.full(24, 0.2, np.float32), np.full(24, 0.2, np.float32)
    if "cliff" in backbone:
        lo[0], hi[0] = 0.79, 0.81
        assert np.array_equal(render.vertex_color(lo, backbone), np.round(render.jet_lut()[int(np.float32(0.79) * 256)] * 255) / 255)
        assert np.array_equal(render.vertex_color(hi, backbone), np.round(render.jet_lut()[255] * 255) / 255)   # var[0]/var[0] = 1
    else:
        lo[0], hi[0] = 0.39, 0.41
        m_lo, m_hi = lo.mean(dtype=np.float32), hi.mean(dtype=np.float32)
        assert np.array_equal(render.vertex_color(lo, backbone), np.round(render.jet_lut()[int(m_lo * 256)] * 255) / 255)
        assert np.array_equal(render.vertex_color(hi, backbone),
                              np.round(render.jet_lut()[int(np.float32(m_hi / np.float32(0.41)) * 256)] * 255) / 255)


def test_projection_matches_reference_matrices():
    """render_np.project against P @ [R Rx | 0] of vibe_renderer.py:49-56,88-110 and GL's viewport (rows from the top)."""
    r = np.random.default_rng(0)
    v = r.normal(size=(50, 3)).astype(np.float32) * 0.4
    H, W = 240, 320
    for rot in (None, render.side_rotation()):
        for cam in ([0.5, 0.6, 0.1, -0.2], [1.3, 1.1, -0.4, 0.3]):
            sx, sy, tx, ty = cam
            P = np.eye(4)
            P[0, 0], P[1, 1], P[0, 3], P[1, 3], P[2, 2] = sx, sy, tx * sx, -ty * sy, -1
            Rx = np.diag([1.0, -1.0, -1.0, 1.0])                                     # rotation_matrix(radians(180), [1,0,0])
            R = np.eye(4)
            if rot is not None:
                R[:3, :3] = rot
            clip = (P @ R @ Rx @ np.c_[v, np.ones(len(v))].T).T
            ndc = clip[:, :3] / clip[:, 3:]
            col = (ndc[:, 0] + 1) * W / 2
            row = H - (ndc[:, 1] + 1) * H / 2
            c, rw, qz = render_np.project(v, cam, H, W, rot)
            assert np.abs(c - col).max() < 1e-4 and np.abs(rw - row).max() < 1e-4
            assert np.abs(-qz - ndc[:, 2]).max() < 1e-5                              # NDC z = -q_z


def test_side_rotation_is_trimesh_ry270():
    R = render.side_rotation()
    assert np.abs(R - np.array([[0, 0, -1], [0, 1, 0], [1, 0, 0]])).max() < 1e-6
    assert abs(np.linalg.det(R) - 1) < 1e-6


def test_video_order_is_stable_ascending_sy():
    cams = np.array([[1, 0.5, 0, 0], [1, 0.2, 0, 0], [1, 0.5, 0, 0], [1, 0.1, 0, 0]], np.float32)
    assert list(render.video_order(cams)) == [3, 1, 0, 2]


def test_render_np_grid_is_watertight():
    """The numpy contract itself: a grid whose shared edges pass through pixel centres covers each analytic pixel once."""
    H = W = 32
    verts, faces, cam, expect = grid_mesh(H, W)
    _, vis = render_np.render_np(np.zeros((H, W, 3), np.uint8), verts[None], faces, [cam], [[1, 1, 1]], [1], return_vis=True)
    assert np.array_equal(vis != render_np.EMPTY, expect)


def grid_mesh(H, W, x0=4, x1=20, y0=6, y1=26, step=2):
    """A planar grid of triangles in the z = 0 plane whose vertices lie on pixel centres (so every interior edge, diagonals
    included, runs through centres).  Camera sx = 2/W, sy = 2/H: col = W/2 + q_x (+ tx), row = H/2 - q_y ... all exact.
    Returns (verts [V,3], faces [F,3], cam, analytic coverage [H,W] bool)."""
    xs = np.arange(x0, x1 + 1, step) + 0.5
    ys = np.arange(y0, y1 + 1, step) + 0.5
    nx, ny = len(xs), len(ys)
    gx, gy = np.meshgrid(xs, ys)
    # q = Rx(180) v = (v_x, -v_y, -v_z); col = W/2 (1 + sx q_x) = W/2 + q_x with sx = 2/W; row = H/2 - q_y = H/2 + v_y
    v = np.stack([gx - W / 2, gy - H / 2, np.zeros_like(gx)], -1).reshape(-1, 3).astype(np.float32)
    faces = []
    for j in range(ny - 1):
        for i in range(nx - 1):
            a, b, c, d = j * nx + i, j * nx + i + 1, (j + 1) * nx + i, (j + 1) * nx + i + 1
            faces += [(a, b, d), (a, d, c)] if (i + j) % 2 else [(a, b, c), (b, d, c)]
    cam = [2.0 / W, 2.0 / H, 0.0, 0.0]
    expect = np.zeros((H, W), bool)
    expect[y0:y1, x0:x1] = True          # centres c + 0.5 in [x0 + 0.5, x1 + 0.5): the left / top boundaries are owned
    return v, np.array(faces, np.int32), cam, expect


def test_header_declares_renderer():
    from poco_amd import _lib
    syms = _lib.header_symbols()
    for s in ("poco_renderer_create", "poco_renderer_render", "poco_renderer_destroy"):
        assert s in syms
    txt = _lib.HEADER.read_text()
    assert "#define POCO_ABI_VERSION 4" in txt and "typedef struct poco_renderer* poco_renderer_t;" in txt


def test_renderer_create_rejects_bad_faces():
    """Validation happens on the host before any GPU call: needs the library, not a device."""
    import ctypes as C
    from poco_amd import _lib
    try:
        L = _lib.lib()
    except _lib.PocoHipError:
        pytest.skip("library not built")
    L.poco_renderer_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    bad = np.array([[0, 1, 2], [1, 2, 7]], np.int32)
    assert L.poco_renderer_create(bad.ctypes.data, 2, 7, C.byref(h)) == 1 and not h.value
    assert b"outside" in L.poco_last_error()
    neg = np.array([[0, -1, 2]], np.int32)
    assert L.poco_renderer_create(neg.ctypes.data, 1, 7, C.byref(h)) == 1
    assert L.poco_renderer_create(bad.ctypes.data, 1 << 22, 7, C.byref(h)) == 1       # F beyond the key's 22 bits
    assert L.poco_renderer_create(None, 1, 7, C.byref(h)) == 1


def test_demo_parse_args_render_flags():
    import demo
    base = ["--cfg", "c.yaml", "--ckpt", "x.pt"]
    a = demo.parse_args(base)
    assert not a.render and not a.sideview and not a.no_uncert_color and not a.no_render
    a = demo.parse_args(base + ["--render", "--sideview", "--no_uncert_color"])
    assert a.render and a.sideview and a.no_uncert_color
    assert demo.render_enabled(a) and not demo.render_enabled(demo.parse_args(base + ["--render", "--no_render"]))


def test_demo_render_without_faces_exits(tmp_path):
    import demo
    np.savez(tmp_path / "smpl.npz", v_template=np.zeros((6890, 3), np.float32))
    (tmp_path / "imgs").mkdir()
    args = demo.parse_args(["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(tmp_path / "none.pt"),
                            "--mode", "folder", "--image_folder", str(tmp_path / "imgs"), "--smpl", str(tmp_path / "smpl.npz"),
                            "--output_folder", str(tmp_path / "out"), "--render"])
    with pytest.raises(SystemExit) as e:
        demo.main(args)
    assert "faces" in str(e.value)
    assert not (tmp_path / "out").exists()
