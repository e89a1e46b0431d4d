"""CPU: the wireframe line rule, culling and the keypoint stamp as tests/render_overlay_np.py restates them, on scenes whose
arithmetic is exact, plus the interface the feature adds (demo flags, header symbols)."""
import numpy as np
import pytest

from poco_amd import _lib
from tests import render_overlay_np as ov

H = W = 32


def test_line_rule_on_integer_segments():
    # horizontal: centres 2.5 .. 9.5 lie in [2, 10); the minor coordinate stays 5
    assert ov.line_pixels((2, 5), (10, 5), H, W) == {(c, 5) for c in range(2, 10)}
    # vertical: |dx| = 0 < |dy|, rows are the major axis
    assert ov.line_pixels((7, 3), (7, 12), H, W) == {(7, r) for r in range(3, 12)}
    # 45 degrees: the tie goes to columns; row = floor(4 + (c + 0.5 - 4)) = c
    assert ov.line_pixels((4, 4), (12, 12), H, W) == {(c, c) for c in range(4, 12)}
    # 1:3: row = floor(2 + (c + 0.5 - 3) / 3)
    assert ov.line_pixels((3, 2), (15, 6), H, W) == {(c, 2 + (c - 3) // 3) for c in range(3, 15)}
    # the same pixels whichever end is A (the walk direction changes t, not the set, on these exact scenes)
    assert ov.line_pixels((10, 5), (2, 5), H, W) == ov.line_pixels((2, 5), (10, 5), H, W)
    # degenerate: no extent along the major axis
    assert ov.line_pixels((5, 5), (5, 5), H, W) == set()
    # clipped to the frame
    assert ov.line_pixels((-4, 1), (40, 1), H, W) == {(c, 1) for c in range(W)}
    assert ov.line_pixels((3, -6), (3, 3), H, W) == {(3, r) for r in range(0, 3)}
    # |q_z| > 1 is dropped fragment by fragment
    fr = ov.segment_fragments((0, 4, 0.0), (16, 4, 2.0), H, W)
    assert {int(p % W) for p in fr["pix"]} == set(range(0, 8))               # z = 2 t <= 1 up to the centre 7.5 (t = 0.469)


def test_shared_edge_walks_are_identical():
    """Both triangles of a shared edge walk it from the lower vertex index: the same A, B and therefore the same fragments."""
    r = np.random.default_rng(5)
    col, row, qz = (r.uniform(2, 30, 4).astype(np.float32), r.uniform(2, 30, 4).astype(np.float32),
                    r.uniform(-0.9, 0.9, 4).astype(np.float32))
    t1, t2 = np.array([0, 1, 2]), np.array([2, 1, 3])                        # share edge 1-2, opposite windings along it
    e1 = [e for e in range(3) if ov.edge_ends(t1, e) == (1, 2)][0]
    e2 = [e for e in range(3) if ov.edge_ends(t2, e) == (1, 2)][0]
    frs = []
    for t, e in ((t1, e1), (t2, e2)):
        A, B = ov.edge_ends(t, e)
        frs.append(ov.segment_fragments((col[A], row[A], qz[A]), (col[B], row[B], qz[B]), H, W))
    assert len(frs[0]["pix"]) > 5
    for k in ("pix", "z", "t"):
        assert np.array_equal(frs[0][k].view(np.uint32) if frs[0][k].dtype == np.float32 else frs[0][k],
                              frs[1][k].view(np.uint32) if frs[1][k].dtype == np.float32 else frs[1][k])


def test_tetrahedron_draws_front_edges_only():
    verts, faces, cam, scr = ov.int_tetrahedron(H, W)
    front = ov.front_facing(verts, faces)
    assert sorted(tuple(sorted(f)) for f in faces[front]) == [(0, 1, 2), (0, 1, 3)]
    info = {}
    frame = np.full((H, W, 3), 9, np.uint8)
    out = ov.wire_np(frame, verts[None], faces, [cam], [[0.8, 0.2, 0.2]], [0], info=info)
    cov = {(int(c), int(r)) for r, c in zip(*np.nonzero(info["ids"] >= 0))}
    expect = set()
    for a, b in ((0, 1), (0, 2), (1, 2), (0, 3), (1, 3)):
        expect |= ov.line_pixels(scr[a], scr[b], H, W)
    assert cov == expect and len(cov) > 40
    # the edge between the two back faces (vertical, col 16, rows 8 .. 23) leaves no pixel of its own
    back_edge = ov.line_pixels(scr[2], scr[3], H, W)
    assert len(back_edge) == 16 and len(back_edge - expect) >= 13 and not (back_edge - expect) & cov
    # every winner is an edge of a front face; untouched pixels keep their bytes
    assert set(np.unique(info["ids"][info["ids"] >= 0] >> 2)) <= set(np.nonzero(front)[0])
    assert np.array_equal(out[info["ids"] < 0], frame[info["ids"] < 0]) and (out[info["ids"] >= 0] != 9).any()
    # a zero-area triangle draws nothing
    flat = np.array([[0, 1, 1], [0, 0, 0]], np.int32)
    info2 = {}
    ov.wire_np(frame, verts[None], flat, [cam], [[1, 1, 1]], [0], info=info2)
    assert (info2["ids"] < 0).all()


def test_depth_and_culling_in_the_restatement():
    verts, faces, cam, (cc, cr) = ov.int_quads(H, W)
    for order in ([0, 1, 2, 3], [2, 3, 0, 1]):
        info = {}
        ov.wire_np(np.zeros((H, W, 3), np.uint8), verts[None], faces[order], [cam], [[1, 1, 1]], [1], info=info)
        tri = faces[order][info["ids"][cr, cc] >> 2]
        assert tri.max() <= 3, "the far quad's edge won the crossing"
    vb, fb, cam, _ = ov.int_quads(H, W, back=True)
    info = {}
    ov.wire_np(np.zeros((H, W, 3), np.uint8), vb[None], fb, [cam], [[1, 1, 1]], [1], info=info)
    assert (info["ids"] < 0).all()


def test_stamp_table():
    tab = ov.disc_table()
    assert tab.shape == (9, 9)
    assert list(tab[4, :5]) == [4, 4, 3, 3, 1]
    assert ov.stamp_rows(4) == [(-4, 1), (-3, 3), (-2, 3), (-1, 4), (0, 4), (1, 4), (2, 3), (3, 3), (4, 1)]
    for r in range(9):
        assert list(tab[r, :r + 1]) == ov.midpoint_circle(r), r
    for bad in (-1, 9):
        with pytest.raises(ValueError):
            ov.stamp_rows(bad)


def _stamp_set(out, colour):
    return {(int(c), int(r)) for r, c in zip(*np.nonzero((out == colour).all(-1)))}


def test_stamp_clips_orders_and_truncates():
    frame = np.zeros((24, 32, 3), np.uint8)
    full = {(dx, dy) for dy, hw in ov.stamp_rows(4) for dx in range(-hw, hw + 1)}
    assert len(full) == 9 + 2 * (9 + 7 + 7 + 3)
    for cx, cy in ((16, 12), (0, 12), (31, 12), (16, 0), (16, 23), (0, 0), (31, 23), (-3, 5), (34, 20), (-9, -9)):
        out = ov.draw_discs_np(frame, [[cx, cy]], [[255, 0, 0]], 4)
        want = {(cx + dx, cy + dy) for dx, dy in full if 0 <= cx + dx < 32 and 0 <= cy + dy < 24}
        assert _stamp_set(out, [255, 0, 0]) == want, (cx, cy)
    # the later index wins where two stamps overlap
    out = ov.draw_discs_np(frame, [[10, 10], [13, 11]], [[255, 0, 0], [0, 255, 0]], 4)
    green = {(13 + dx, 11 + dy) for dx, dy in full}
    assert _stamp_set(out, [0, 255, 0]) == green
    assert _stamp_set(out, [255, 0, 0]) == {(10 + dx, 10 + dy) for dx, dy in full} - green
    # truncation toward zero: -0.9 -> 0 (floor would give -1), -1.5 -> -1, 3.99 -> 3
    a = ov.draw_discs_np(frame, [[-0.9, 3.99]], [[1, 2, 3]], 4)
    assert np.array_equal(a, ov.draw_discs_np(frame, [[0, 3]], [[1, 2, 3]], 4))
    a = ov.draw_discs_np(frame, [[-1.5, -1.5]], [[1, 2, 3]], 4)
    assert np.array_equal(a, ov.draw_discs_np(frame, [[-1, -1]], [[1, 2, 3]], 4))
    assert not np.array_equal(a, ov.draw_discs_np(frame, [[-2, -2]], [[1, 2, 3]], 4))
    # a point that is not a number paints nothing
    assert np.array_equal(ov.draw_discs_np(frame, [[np.nan, 3], [np.inf, 3]], [[9, 9, 9]], 4), frame)


def test_demo_parse_args_overlay_flags():
    import demo
    base = ["--cfg", "c.yaml", "--ckpt", "x.pt"]
    a = demo.parse_args(base)
    assert not a.wireframe and not a.draw_keypoints and not a.render_crop
    a = demo.parse_args(base + ["--render", "--wireframe", "--draw_keypoints", "--render_crop"])
    assert a.wireframe and a.draw_keypoints and a.render_crop and demo.render_enabled(a)
    assert not demo.render_enabled(demo.parse_args(base + ["--render", "--wireframe", "--no_render"]))


def test_header_declares_overlay_symbols():
    syms = _lib.header_symbols()
    for s in ("poco_renderer_render_ex", "poco_renderer_draw_discs", "poco_renderer_render"):
        assert s in syms, s
    txt = _lib.HEADER.read_text()
    assert "#define POCO_ABI_VERSION 4" in txt                               # additions only: the ABI version is not bumped
    assert "#define POCO_RENDER_WIREFRAME 1u" in txt and "POCO_RENDER_MAX_WIRE_FACES ((1 << 20) - 1)" in txt
    L = _lib.lib()
    assert hasattr(L, "poco_renderer_render_ex") and hasattr(L, "poco_renderer_draw_discs")


def test_bad_arguments_need_no_gpu():
    """Validation happens on the host before any GPU call: needs the library, not a device."""
    import ctypes as C
    L = _lib.lib()
    L.poco_renderer_draw_discs.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    p = C.c_void_p(0x1000)                                                   # never dereferenced: every call below is refused
    for args in ((None, 8, 8, p, p, 1, 4), (p, 8, 8, None, p, 1, 4), (p, 8, 8, p, None, 1, 4), (p, 8, 8, p, p, -1, 4),
                 (p, 8, 8, p, p, 1, -1), (p, 8, 8, p, p, 1, 9), (p, 0, 8, p, p, 1, 4), (p, 8, 16385, p, p, 1, 4)):
        assert L.poco_renderer_draw_discs(*args, None) == 1, args
    assert b"poco_renderer_draw_discs" in L.poco_last_error()
    L.poco_renderer_render_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p, C.c_uint, C.c_void_p]
    assert L.poco_renderer_render_ex(None, p, 8, 8, p, 1, p, None, None, 1, None) == 1          # no handle
    assert L.poco_renderer_render_ex(None, p, 8, 8, p, 1, p, None, None, 4, None) == 1          # unknown flag bit
    assert b"unknown flag" in L.poco_last_error()


def test_keypoint_helpers():
    """The host rules around the stamp: which joints get which colour in which order, and the crop's coordinate frame."""
    from poco_amd import render
    from poco_amd.tester import crop_keypoints
    j = np.arange(49 * 3, dtype=np.float32).reshape(49, 3)                   # (x, y, confidence) rows as the results store them
    pts, rgb = render.folder_keypoints(j)
    assert pts.shape == (49, 2) and rgb.shape == (49, 3) and rgb.dtype == np.uint8
    assert np.array_equal(pts[:24], j[25:, :2]) and (rgb[:24] == 255).all()   # SMPL joints [25:] white, painted first
    assert np.array_equal(pts[24:], j[:25, :2]) and (rgb[24:] == 0).all()     # OpenPose joints [:25] black, on top
    # painted in that order, a black stamp covers a white one at the same place
    same = np.tile(np.float32([[10, 10, 1]]), (49, 1))
    out = ov.draw_discs_np(np.full((24, 24, 3), 7, np.uint8), *render.folder_keypoints(same), 4)
    assert (out[10, 10] == 0).all() and not (out == 255).any()
    pts, rgb = render.video_keypoints(j[:, :2])
    assert np.array_equal(pts, j[:, :2]) and (rgb == [0, 255, 0]).all() and rgb.shape == (49, 3)
    # crop frame: the box centre goes to the crop centre, the box's edges to the crop's edges, each axis by its own extent
    box = [80.0, 60.0, 40.0, 56.0]                                            # 224 / 40 and 224 / 56 are exact
    got = crop_keypoints(np.float32([[80, 60, 1], [60, 32, 1], [100, 88, 1], [90, 60, 1], [80, 74, 1]]), box, 224, 1.0)
    assert got.dtype == np.float32 and np.array_equal(got, np.float32([[112, 112], [0, 0], [224, 224], [168, 112], [112, 168]]))
    # bbox_scale widens the source window: the same point lands nearer the centre
    assert np.array_equal(crop_keypoints(np.float32([[100, 88]]), box, 224, 2.0), np.float32([[168, 168]]))
    # a joint outside the image maps outside the canvas, it is not pulled in
    assert crop_keypoints(np.float32([[-20, 60]]), box, 224, 1.0)[0, 0] == 112 - 100 * 224 / 40
