"""The demo's uncertainty-coloured mesh overlay (demo.py --render) on the GPU: a binding of poco_renderer_* (include/poco_hip.h,
csrc/render.hip) plus the small host-side rules around it - matplotlib's jet LUT, the reference's get_vertex_colors
(pocolib/utils/renderer.py:193-224), the side-view rotation and the painter's order of each mode.

The reference draws with pyrender + trimesh + EGL (pocolib/utils/vibe_renderer.py); none of them is needed here."""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import numpy as np
import torch

from ._lib import PocoHipError, check, lib

MATERIAL_UNCERT = 0.0          # pyrender's default material of a vertex-coloured trimesh (metallic 0.2, roughness 0.8)
MATERIAL_PLAIN = 1.0           # MetallicRoughnessMaterial(metallicFactor=0) of vibe_renderer.py:118-122 (roughness 1)
GREY = (0.70, 0.70, 0.70)      # --no_uncert_color (tester.py:288-290)
MAX_PEOPLE = 1024
FLAG_WIREFRAME = 1             # POCO_RENDER_WIREFRAME
FLAG_IDS = 2                   # POCO_RENDER_IDS (test hook)
MAX_WIRE_FACES = (1 << 20) - 1
DISC_RADIUS = 4                # cv2.circle(..., 4, ..., -1) of tester.py:324-328,552-554

# matplotlib's `jet` segment data (matplotlib/_cm.py): (x, value below x, value above x) per channel
_JET = {
    "red": ((0.00, 0, 0), (0.35, 0, 0), (0.66, 1, 1), (0.89, 1, 1), (1.00, 0.5, 0.5)),
    "green": ((0.000, 0, 0), (0.125, 0, 0), (0.375, 1, 1), (0.640, 1, 1), (0.910, 0, 0), (1.000, 0, 0)),
    "blue": ((0.00, 0.5, 0.5), (0.11, 1, 1), (0.34, 1, 1), (0.65, 0, 0), (1.00, 0, 0)),
}
_LUT = None


def _segment_lut(data, n: int = 256) -> np.ndarray:
    """LinearSegmentedColormap's lookup table of one channel (gamma 1), in matplotlib's own arithmetic (x scaled by N - 1)."""
    a = np.asarray(data, np.float64)
    x, y0, y1 = a[:, 0] * (n - 1), a[:, 1], a[:, 2]
    xind = (n - 1) * np.linspace(0, 1, n)
    ind = np.searchsorted(x, xind)[1:-1]
    dist = (xind[1:-1] - x[ind - 1]) / (x[ind] - x[ind - 1])
    lut = np.concatenate([[y1[0]], dist * (y0[ind] - y1[ind - 1]) + y1[ind - 1], [y0[-1]]])
    return np.clip(lut, 0.0, 1.0)


def jet_lut() -> np.ndarray:
    """[256, 3] float64: matplotlib.cm.jet's RGB table."""
    global _LUT
    if _LUT is None:
        _LUT = np.stack([_segment_lut(_JET[c]) for c in ("red", "green", "blue")], 1)
    return _LUT


def jet(x) -> np.ndarray:
    """cm.jet(x)[:3] of a float32 value: index trunc(x * 256) clamped to 0..255 (x = 1 is the last entry, below 0 the first)."""
    xa = np.float32(x) * np.float32(256)
    i = 0 if not xa >= 0 else min(int(xa), 255)
    return jet_lut()[i]


def vertex_color(var, backbone: str) -> np.ndarray:
    """The one colour get_vertex_colors (renderer.py:193-224, sensitivity 0.40) gives every vertex of a person, quantised to 8 bits
    as a trimesh vertex colour is stored: float64 [3] in [0, 1].
        cliff: jet(var[0] / vmax),    vmax = var[0] if var[0] > 0.8 else 1
        pare:  jet(mean(var) / vmax), vmax = var[0] if var[0] > 0.4 else 1
    var = the post-processed [24] vector stored in the results (postproc.folder_uncert / video_uncert)."""
    v = np.asarray(var, np.float32).reshape(-1)
    if v.shape[0] == 1:
        label, vmax = v[0], np.float32(1)
    elif "cliff" in backbone:
        label = v[0]
        vmax = v[0] if v[0] > 2 * 0.40 else np.float32(1)
    elif "pare" in backbone:
        label = v.mean(dtype=np.float32)
        vmax = v[0] if v[0] > 0.40 else np.float32(1)
    else:
        raise ValueError(f"vertex_color: backbone {backbone!r} is neither cliff nor pare")
    c = jet(np.float32(label) / np.float32(vmax))
    return np.round(c * 255.0) / 255.0


def side_rotation() -> np.ndarray:
    """trimesh.transformations.rotation_matrix(radians(270), [0, 1, 0])[:3, :3] (tester.py:335-348), float32 row-major."""
    a = np.radians(270.0)
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, 0, s], [0, 1, 0], [-s, 0, c]], np.float32)


def video_order(orig_cams: np.ndarray) -> np.ndarray:
    """Painter's order of the people of one video frame: ascending orig_cam[1] (sy), as demo_utils.py:307-313 sorts them;
    ties keep track order."""
    return np.argsort(np.asarray(orig_cams, np.float32).reshape(-1, 4)[:, 1], kind="stable")


class Renderer:
    """Rasteriser + compositor for meshes that share one triangle list (SMPL: V = 6890, F = 13776).

        r = Renderer(faces, 6890, device)
        r.render(frame_u8_cuda, verts, orig_cam, colors, materials, rotation=None)   # draws over frame, returns it
    """

    def __init__(self, faces, V: int, device=None):
        f = np.ascontiguousarray(np.asarray(faces).reshape(-1, 3), dtype=np.int64)
        if f.size and (f.min() < np.iinfo(np.int32).min or f.max() > np.iinfo(np.int32).max):
            raise PocoHipError("Renderer: face index out of int32 range")
        self.faces = np.ascontiguousarray(f, np.int32)
        self.V = int(V)
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        L = lib()
        L.poco_renderer_create.argtypes = [C.c_void_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.poco_renderer_render.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]
        L.poco_renderer_render_ex.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                              C.c_void_p, C.c_uint, C.c_void_p]
        L.poco_renderer_destroy.argtypes = [C.c_void_p]
        L.poco_renderer_destroy.restype = None
        self._h = C.c_void_p()
        with torch.cuda.device(self.device):
            check(L.poco_renderer_create(self.faces.ctypes.data, self.faces.shape[0], self.V, C.byref(self._h)),
                  "poco_renderer_create")

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().poco_renderer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def params(self, orig_cam, colors, materials) -> torch.Tensor:
        """[P, 8] float32 on the device: (sx, sy, tx, ty, r, g, b, material) per person."""
        cam = np.asarray(orig_cam, np.float32).reshape(-1, 4)
        P = cam.shape[0]
        col = np.asarray(colors, np.float32).reshape(P, 3)
        mat = np.broadcast_to(np.asarray(materials, np.float32).reshape(-1), (P,))
        host = np.concatenate([cam, col, mat[:, None]], 1)
        return torch.from_numpy(np.ascontiguousarray(host)).to(self.device)

    def render(self, frame: torch.Tensor, verts, orig_cam, colors, materials, rotation=None,
               frag_count: Optional[torch.Tensor] = None, wireframe: bool = False, ids: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Draw P people over `frame` (uint8 [H,W,3] RGB, contiguous, on the device) in place and return it.  verts [P,V,3]
        float32 (a device tensor is used as it is, anything else is uploaded); orig_cam [P,4]; colors [P,3] in [0,1]; materials
        [P] or a scalar (MATERIAL_UNCERT / MATERIAL_PLAIN); rotation: 3x3 or None.  Person p + 1 covers person p.
        frag_count: int32 [H,W] on the device, receives the fragments per pixel (a test hook).  wireframe: draw the edges of the
        front-facing triangles as one-pixel lines (--wireframe) through poco_renderer_render_ex; without it the call is
        poco_renderer_render as before.  ids: int32 [H,W] on the device, receives the id that won each pixel or -1 (a test hook,
        instead of frag_count).  Enqueued on the current stream."""
        if not (torch.is_tensor(frame) and frame.device.type == "cuda" and frame.dtype == torch.uint8 and frame.dim() == 3
                and frame.shape[2] == 3 and frame.is_contiguous()):
            raise PocoHipError("Renderer.render: frame must be a contiguous uint8 [H,W,3] device tensor")
        H, W = int(frame.shape[0]), int(frame.shape[1])
        if torch.is_tensor(verts) and verts.device == frame.device:
            v = verts.reshape(-1, self.V, 3)
            if v.dtype != torch.float32 or not v.is_contiguous():
                v = v.to(torch.float32).contiguous()
        else:
            v = torch.from_numpy(np.ascontiguousarray(np.asarray(verts, np.float32).reshape(-1, self.V, 3))).to(frame.device)
        P = int(v.shape[0])
        prm = self.params(orig_cam, colors, materials)
        if prm.shape[0] != P:
            raise PocoHipError(f"Renderer.render: {P} meshes but {prm.shape[0]} cameras")
        rot = None
        if rotation is not None:
            rot = np.ascontiguousarray(np.asarray(rotation, np.float32).reshape(3, 3))
        cnt = 0
        if frag_count is not None:
            assert frag_count.dtype == torch.int32 and frag_count.is_contiguous() and frag_count.numel() == H * W
            cnt = frag_count.data_ptr()
        flags = FLAG_WIREFRAME if wireframe else 0
        if ids is not None:
            assert frag_count is None and ids.dtype == torch.int32 and ids.is_contiguous() and ids.numel() == H * W
            cnt, flags = ids.data_ptr(), flags | FLAG_IDS
        stream = C.c_void_p(torch.cuda.current_stream(frame.device).cuda_stream)
        if flags:
            check(lib().poco_renderer_render_ex(self._h, frame.data_ptr(), H, W, v.data_ptr(), P, prm.data_ptr(),
                                                rot.ctypes.data if rot is not None else None, cnt or None, flags, stream),
                  "poco_renderer_render_ex")
        else:
            check(lib().poco_renderer_render(self._h, frame.data_ptr(), H, W, v.data_ptr(), P, prm.data_ptr(),
                                             rot.ctypes.data if rot is not None else None, cnt or None, stream),
                  "poco_renderer_render")
        return frame


_DISCS = None


def _draw_discs_fn():
    """poco_renderer_draw_discs with its argument types, bound once."""
    global _DISCS
    if _DISCS is None:
        fn = lib().poco_renderer_draw_discs
        fn.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
        _DISCS = fn
    return _DISCS


def draw_discs(frame: torch.Tensor, points, rgb, radius: int = DISC_RADIUS) -> torch.Tensor:
    """Stamp filled discs over `frame` (uint8 [H,W,3] contiguous device tensor) in place: points [N,2] (col, row) float32,
    truncated toward zero as the reference's int(pt[0]); rgb [N,3] uint8 or one colour for all.  Device tensors (float32 / uint8,
    contiguous, on the frame's device) are used as they are, anything else is uploaded.  Painted in index order, the later point
    on top (poco_renderer_draw_discs).  Enqueued on the current stream."""
    if not (torch.is_tensor(frame) and frame.device.type == "cuda" and frame.dtype == torch.uint8 and frame.dim() == 3
            and frame.shape[2] == 3 and frame.is_contiguous()):
        raise PocoHipError("draw_discs: frame must be a contiguous uint8 [H,W,3] device tensor")
    if torch.is_tensor(points) and torch.is_tensor(rgb):
        dp, dc = points, rgb
        if not (dp.device == frame.device and dc.device == frame.device and dp.dtype == torch.float32 and dc.dtype == torch.uint8
                and dp.is_contiguous() and dc.is_contiguous() and dp.dim() == 2 and dp.shape[1] == 2
                and tuple(dc.shape) == (dp.shape[0], 3)):
            raise PocoHipError("draw_discs: device points must be contiguous float32 [N,2] and colours uint8 [N,3] on the frame's device")
    else:
        pts = np.array(np.asarray(points, np.float32).reshape(-1, 2))
        col = np.array(np.broadcast_to(np.asarray(rgb, np.uint8).reshape(-1, 3), (pts.shape[0], 3)))      # a writable copy
        dp, dc = torch.from_numpy(pts).to(frame.device), torch.from_numpy(col).to(frame.device)
    check(_draw_discs_fn()(frame.data_ptr(), int(frame.shape[0]), int(frame.shape[1]), dp.data_ptr(), dc.data_ptr(), int(dp.shape[0]),
                           int(radius), C.c_void_p(torch.cuda.current_stream(frame.device).cuda_stream)),
          "poco_renderer_draw_discs")
    return frame


def folder_keypoints(joints2d):
    """(points [49,2], rgb [49,3]) of one person in folder mode (tester.py:324-328): the SMPL joints [25:] white first, then the
    OpenPose joints [:25] black on top."""
    j = np.asarray(joints2d, np.float32).reshape(49, -1)[:, :2]
    return (np.concatenate([j[25:], j[:25]], 0),
            np.concatenate([np.full((24, 3), 255, np.uint8), np.zeros((25, 3), np.uint8)], 0))


def video_keypoints(joints2d):
    """(points [49,2], rgb [49,3]) of one person in video mode (tester.py:552-554): all 49 joints in (0, 255, 0)."""
    j = np.asarray(joints2d, np.float32).reshape(49, -1)[:, :2]
    return j, np.tile(np.array([[0, 255, 0]], np.uint8), (49, 1))


def input_keypoints(joints2d, vis_thresh: float = 0.3):
    """(points [n,2], rgb [n,3]) of the keypoints a track came in with (video mode, --tracking_method pose): those of the
    [K,3] (x, y, confidence) rows whose confidence exceeds vis_thresh, in folder mode's OpenPose colour, black."""
    j = np.asarray(joints2d, np.float32).reshape(-1, 3)
    j = j[j[:, 2] > np.float32(vis_thresh)]
    return np.ascontiguousarray(j[:, :2]), np.zeros((j.shape[0], 3), np.uint8)


def person_style(var, backbone: str, uncert_color: bool = True):
    """(colour, material) of one person: the uncertainty colour (vertex_color) or the plain grey of --no_uncert_color."""
    if uncert_color and var is not None:
        return vertex_color(var, backbone), MATERIAL_UNCERT
    return np.asarray(GREY), MATERIAL_PLAIN


def render_people(renderer: Renderer, frame: torch.Tensor, verts, orig_cam, var: Optional[Sequence], backbone: str,
                  uncert_color: bool = True, sideview: bool = False, side_bg: int = 255, wireframe: bool = False,
                  keypoints: Optional[Sequence] = None) -> torch.Tensor:
    """The demo's picture of one frame: the people (already in painter's order) drawn over `frame` (a device uint8 [H,W,3],
    drawn on in place) and, with `sideview`, the Ry(270 deg) view on a canvas of value `side_bg` (folder mode white, video
    mode black) concatenated to its right.  wireframe: both views as wireframes.  keypoints: per person (points, rgb) of
    draw_discs, stamped on the main view after that person's mesh and before the next person's (tester.py:306-328,537-554),
    never on the side view.  Returns the device image [H, W or 2W, 3]."""
    cam = np.asarray(orig_cam, np.float32).reshape(-1, 4)
    P = cam.shape[0]
    styles = [person_style(None if var is None else var[i], backbone, uncert_color) for i in range(P)]
    colors = np.array([s[0] for s in styles], np.float32).reshape(P, 3)
    mats = np.array([s[1] for s in styles], np.float32)
    if keypoints is None:
        renderer.render(frame, verts, cam, colors, mats, wireframe=wireframe)
    else:                                  # a person's discs lie under the next person's mesh: one call per person
        # vertices, points and colours of all people go up in one transfer each; the calls below take slices
        if not (torch.is_tensor(verts) and verts.device == frame.device):
            verts = torch.from_numpy(np.ascontiguousarray(np.asarray(verts, np.float32).reshape(P, -1, 3))).to(frame.device)
        v = verts.reshape(P, -1, 3)
        counts = [int(np.asarray(k[0]).reshape(-1, 2).shape[0]) for k in keypoints]
        pts = np.concatenate([np.asarray(k[0], np.float32).reshape(-1, 2) for k in keypoints], 0)
        rgb = np.concatenate([np.broadcast_to(np.asarray(k[1], np.uint8).reshape(-1, 3), (n, 3)) for k, n in zip(keypoints, counts)], 0)
        dp, dc = torch.from_numpy(np.ascontiguousarray(pts)).to(frame.device), torch.from_numpy(np.ascontiguousarray(rgb)).to(frame.device)
        lo = 0
        for i in range(P):
            renderer.render(frame, v[i:i + 1], cam[i:i + 1], colors[i:i + 1], mats[i:i + 1], wireframe=wireframe)
            draw_discs(frame, dp[lo:lo + counts[i]], dc[lo:lo + counts[i]])
            lo += counts[i]
    if not sideview:
        return frame
    side = torch.full_like(frame, side_bg)
    renderer.render(side, verts, cam, colors, mats, rotation=side_rotation(), wireframe=wireframe)
    return torch.cat([frame, side], 1)
