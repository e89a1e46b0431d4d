"""The head kernels ALONE against fp64 numpy (tests/head_np.py): camera_kernel, the persistent regressor chain on hand-made programs,
part attention on planes smaller than its pixel splits, rot6d / lc2d / row copies / NHWC -> NCHW / pack_record at strides the
engine never uses.  Every operand lies in a NaN-filled buffer and every output between poisoned guard bands (ops.Wide / ops.Rows):
a read outside an operand turns the result NaN, a stray store changes a guard.

Errors are max |out - ref| / max(1, |ref|max).  Pure data movement is exact.  Linear layers of the chain keep the ALG 5 bound of
tests/test_conv_gpu.py::test_linear_small_m.  Every other bound in TOL is four times the larger of (a) the error of the same formula
evaluated in float32 numpy on the test's own inputs and (b) what the kernel showed on its first run on an MI355X; both figures
stand next to the bound, and every check prints its own (pytest -s).  NOTEBOOK.md ("Head kernels alone") has the table."""
import ctypes as C

import numpy as np
import pytest
import torch

from poco_amd import ops
from poco_amd._lib import PocoHipError, lib
from tests import head_np

pytestmark = pytest.mark.gpu

LINEAR_TOL = 2e-5              # tests/test_conv_gpu.py::test_linear_small_m: 2e-5 * max(1, |ref|max)
#        group                      bound        float32 numpy   kernel, first run
TOL = {
    "camera.pare.cam_t":           4.1e-7,    # 8.19e-08       1.02e-07
    "camera.pare.joints2d":        6.0e-7,    # 1.50e-07       1.50e-07
    "camera.cliff.cam_t":          2.4e-7,    # 5.97e-08       5.97e-08
    "camera.cliff.fullimg_cam_t":  5.8e-7,    # 1.44e-07       1.44e-07
    "camera.cliff.joints2d":       6.4e-7,    # 1.59e-07       1.50e-07
    "chain.sigmoid":               1.8e-6,    # 4.45e-07       2.66e-07   act = 2 layers: the Linear error through the sigmoid and __expf
    "chain.rot6d":                 5.5e-5,    # 1.37e-05       1.07e-05   rot6d jobs of a chain, on inputs and on a layer's output (130 x 24 rows: short columns amplify)
    "attention":                   9.6e-7,    # 2.29e-07       2.39e-07   relative form: bound * max(1, |ref|max)
    "attention.spread":            6.8e-7,    # 1.68e-07       1.32e-07
    "rot6d":                       6.9e-6,    # 1.71e-06       9.79e-07
    "rot6d.near_parallel":         1.1e-2,    # 2.13e-03       2.73e-03   the second column 1e-4 off the first: the projection cancels four digits
    "lc2d":                        2.1e-6,    # 5.08e-07       5.08e-07
    "record.confidence":           9.3e-8,    # 9.75e-09       2.31e-08
}


@pytest.fixture(scope="module")
def cuda():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _err(out, ref):
    return float(np.abs(np.asarray(out, np.float64) - ref).max() / max(1.0, np.abs(ref).max()))


class Acc:
    """Collects the comparisons of one test, prints every figure, asserts at the end (so that one run shows all of them)."""

    def __init__(self):
        self.bad = []

    def add(self, group, label, out, ref, ref32=None, bound=None):
        bound = TOL[group] if bound is None else bound
        out = np.asarray(out)
        e = _err(out, ref)
        e32 = float("nan") if ref32 is None else _err(ref32, ref)
        print(f"HEADK {group} [{label}] float32 {e32:.3e} kernel {e:.3e} bound {bound} |ref|max {np.abs(ref).max():.3e}")
        if not np.isfinite(out).all():
            self.bad.append((group, label, "NaN / inf in the output"))
        if not e <= bound:
            self.bad.append((group, label, e, bound))
        if not np.abs(ref).max() > 50 * bound:                       # not vacuous: the values stand well above what is tolerated
            self.bad.append((group, label, "vacuous reference", float(np.abs(ref).max())))

    def exact(self, label, out, ref):
        out, ref = np.asarray(out), np.asarray(ref, np.float32)
        if out.shape != ref.shape or not np.array_equal(out.view(np.int32), ref.view(np.int32)):
            self.bad.append((label, "not bitwise equal"))

    def true(self, label, cond):
        if not cond:
            self.bad.append((label, "failed"))

    def check(self):
        assert not self.bad, self.bad


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


# ---- camera ------------------------------------------------------------------------------------------------------------------
def _camera_inputs(B, seed):
    r = np.random.default_rng(seed)
    cam = np.stack([r.uniform(0.3, 1.5, B), r.uniform(-0.4, 0.4, B), r.uniform(-0.4, 0.4, B)], -1).astype(np.float32)
    j49 = r.uniform(-0.9, 0.9, (B, 49, 3)).astype(np.float32)
    return r, cam, j49


@pytest.mark.parametrize("cam_stride", [3, 7])
@pytest.mark.parametrize("B", [1, 3, 21])
def test_camera_pare(B, cam_stride, cuda):
    """smpl_head.py:63-78: B * 49 = 49, 147, 1029 threads, none a multiple of the 128-thread block; the CLIFF arrays are null and
    d_fullimg_cam_t, though given, is not written."""
    _, cam, j49 = _camera_inputs(B, 100 + B)
    ref = head_np.camera(cam, j49, False)
    r32 = head_np.camera(cam, j49, False, dtype=np.float32)
    o = ops.camera(_t(cam, cuda), _t(j49, cuda), cliff=False, cam_stride=cam_stride)
    a = Acc()
    a.add("camera.pare.cam_t", f"B{B}", o["cam_t"].cpu().numpy(), ref[0], r32[0])
    a.add("camera.pare.joints2d", f"B{B}", o["joints2d"].cpu().numpy(), ref[2], r32[2])
    wt, wf, w2 = o["bufs"]
    a.true("guards", wt.untouched([(0, B * 3)]) and wf.untouched([]) and w2.untouched([(0, B * 98)]))
    a.check()


@pytest.mark.parametrize("focal_kind", ["diag", "random"])
@pytest.mark.parametrize("shape", [(480, 640), (1080, 720)])
@pytest.mark.parametrize("B,cam_stride,fullimg", [(1, 3, True), (3, 7, False), (21, 7, True)])
def test_camera_cliff(B, cam_stride, fullimg, shape, focal_kind, cuda):
    """smplcam_head.py:65-90,123-139 on non-square images: crop boxes in the centre, in a corner and partly outside the image
    (crop b takes placement b % 3), focal = sqrt(h^2 + w^2) or a per-crop value.  fullimg = False: the nullable output is null
    and nothing else is written in its place."""
    r, cam, j49 = _camera_inputs(B, 200 + B)
    h, w = shape
    scale = r.uniform(0.6, 1.8, B).astype(np.float32)                     # box height = 200 scale pixels
    place = np.arange(B) % 3
    cx = np.where(place == 0, w / 2, np.where(place == 1, 100.0 * scale, w + 30.0 * scale))
    cy = np.where(place == 0, h / 2, np.where(place == 1, 100.0 * scale, -20.0 * scale))
    center = np.stack([cx, cy], -1).astype(np.float32)
    orig = np.tile(np.array([[h, w]], np.float32), (B, 1))
    focal = np.full(B, np.sqrt(h * h + w * w), np.float32) if focal_kind == "diag" else r.uniform(500.0, 3000.0, B).astype(np.float32)
    ref = head_np.camera(cam, j49, True, focal, scale, center, orig)
    r32 = head_np.camera(cam, j49, True, focal, scale, center, orig, dtype=np.float32)
    o = ops.camera(_t(cam, cuda), _t(j49, cuda), cliff=True, focal=_t(focal, cuda), scale=_t(scale, cuda), center=_t(center, cuda),
                   orig_shape=_t(orig, cuda), cam_stride=cam_stride, fullimg=fullimg)
    a = Acc()
    lab = f"B{B} {h}x{w} {focal_kind}"
    a.add("camera.cliff.cam_t", lab, o["cam_t"].cpu().numpy(), ref[0], r32[0])
    a.add("camera.cliff.joints2d", lab, o["joints2d"].cpu().numpy(), ref[2], r32[2])
    if fullimg:
        a.add("camera.cliff.fullimg_cam_t", lab, o["fullimg_cam_t"].cpu().numpy(), ref[1], r32[1])
    wt, wf, w2 = o["bufs"]
    a.true("guards", wt.untouched([(0, B * 3)]) and wf.untouched([(0, B * 3)] if fullimg else []) and w2.untouched([(0, B * 98)]))
    a.check()


# ---- the regressor chain on hand-made programs ---------------------------------------------------------------------------------
# A program: bufs = [(stride, fill)], inputs = [(buf, off, array [rows, n])] (a broadcast reads row 0 only),
# layers / rows / stages as ops.mlp_chain takes them, outs = [(buf, off, n, class)] with class "exact" | "linear" | "sigmoid" | "rot6d".
EXTRA_ROWS = 2


def _chain_ref(prog, B, dtype=np.float64):
    """The program in plain numpy: the stages in order, every job of a stage from the buffers as the stage found them."""
    bufs = [np.full((B, stride), np.nan, dtype) for stride, _ in prog["bufs"]]
    for b, off, x in prog["inputs"]:
        bufs[b][:x.shape[0], off:off + x.shape[1]] = x
    for l0, nl, r0, nr in prog["stages"]:
        writes = []
        for L in prog["layers"][l0:l0 + nl]:
            N, K = L["W"].shape
            x = bufs[L["src"][0]][:, L["src"][1]:L["src"][1] + K]
            res = None if L.get("res") is None else bufs[L["res"][0]][:, L["res"][1]:L["res"][1] + N]
            writes.append((L["dst"], head_np.linear(x, L["W"], L["b"], L.get("act", 0), res, dtype=dtype)))
        for J in prog["rows"][r0:r0 + nr]:
            sb, so = J["src"]
            if J["kind"] == 2:
                y = head_np.rot6d(bufs[sb][:, so:so + 144].reshape(B, 24, 6), dtype=dtype).reshape(B, 216)
            elif J["kind"] == 1:
                y = np.tile(bufs[sb][:1, so:so + J["n"]], (B, 1))
            else:
                y = bufs[sb][:, so:so + J["n"]].copy()
            for key in ("dst", "dst2"):
                if J.get(key) is not None:
                    writes.append((J[key], y))
        for (b, off), y in writes:
            bufs[b][:, off:off + y.shape[1]] = y
    return [bufs[b][:, off:off + n] for b, off, n, _ in prog["outs"]]


def _chain_run(prog, B, max_blocks, dev, calls=1):
    """-> (the outs as numpy, True if every buffer kept its fill outside the outs: other columns, rows >= B, guard bands)."""
    bufs = [ops.Rows(B, stride, dev, fill, extra_rows=EXTRA_ROWS) for stride, fill in prog["bufs"]]
    for b, off, x in prog["inputs"]:
        bufs[b].body[:x.shape[0], off:off + x.shape[1]] = _t(x, dev)
    for b, off, n, _ in prog["outs"]:
        bufs[b].mark(off, n)
    for _ in range(calls):
        assert ops.mlp_chain(prog["layers"], prog["rows"], prog["stages"], bufs, B, max_blocks) == 0
    outs = [bufs[b].get(off, n).cpu().numpy() for b, off, n, _ in prog["outs"]]
    clean = True
    for i, w in enumerate(bufs):
        written = [(off, n) for b, off, n, _ in prog["outs"] if b == i]
        given = [(off, x.shape[1]) for b, off, x in prog["inputs"] if b == i]
        clean &= w.untouched(written + given)
    return outs, clean


def _chain_compare(a, label, prog, B, outs):
    ref = _chain_ref(prog, B)
    r32 = _chain_ref(prog, B, np.float32)
    for (b, off, n, cls), o, rf, r3 in zip(prog["outs"], outs, ref, r32):
        lab = f"{label} buf{b}+{off}"
        if cls == "exact":
            a.exact(lab, o, rf)
        elif cls == "linear":
            a.add("chain.linear", lab, o, rf, r3, bound=LINEAR_TOL)
        else:
            a.add({"sigmoid": "chain.sigmoid", "rot6d": "chain.rot6d"}[cls], lab, o, rf, r3)
        if cls == "sigmoid":
            a.true(lab + " both sides of 0.5", rf.min() < 0.4 and rf.max() > 0.6)


def _linear_programs(K16, B, seed):
    """The 12 Linear layers N/16 in {1, 3} x act in {0, 1, 2} x residual {no, yes} on one input: each as a program of its own and all
    of them as ONE stage.  Input, residual and outputs are column slices of wider rows (every row stride exceeds the width)."""
    r = np.random.default_rng(seed)
    K = 16 * K16
    x = r.standard_normal((B, K)).astype(np.float32)
    res = r.standard_normal((B, 48)).astype(np.float32)
    layers, outs, cur = [], [], 4
    for N16 in (1, 3):
        for act in (0, 1, 2):
            for use_res in (False, True):
                N = 16 * N16
                layers.append(dict(W=(r.standard_normal((N, K)) / np.sqrt(K)).astype(np.float32), b=r.uniform(-0.5, 0.5, N).astype(np.float32),
                                   act=act, src=(0, 8), res=(1, 4) if use_res else None, dst=(2, cur)))
                outs.append((2, cur, N, "sigmoid" if act == 2 else "linear"))
                cur += N + 4
    base = dict(bufs=[(K + 24, "nan"), (60, "nan"), (cur + 8, "poison")], inputs=[(0, 8, x), (1, 4, res)], rows=[])
    singles = [dict(base, layers=[L], stages=[(0, 1, 0, 0)], outs=[o]) for L, o in zip(layers, outs)]
    return singles, dict(base, layers=layers, stages=[(0, 12, 0, 0)], outs=outs)


@pytest.mark.parametrize("B", [1, 16, 17, 130])
@pytest.mark.parametrize("K16", [1, 3, 8, 9, 65])
def test_chain_linear_layers(K16, B, cuda):
    """K/16 = 1, 3: most waves own no K slice; 8, 9: one slice per wave, and one wave with two; 65: a second trip of the unrolled
    slice loop, where the weights prefetched across the barrier must not be used again.  Each layer alone, then the twelve in one
    stage (decode_job walks from layer to layer) on grids of 1, 7 and 256 blocks: bitwise the same everywhere."""
    singles, combined = _linear_programs(K16, B, 1000 * K16 + B)
    a = Acc()
    alone = []
    for i, p in enumerate(singles):
        outs, clean = _chain_run(p, B, 256, cuda)
        _chain_compare(a, f"K16={K16} B={B} layer{i}", p, B, outs)
        a.true(f"layer{i} guards", clean)
        alone.append(outs[0])
    for nb in (1, 7, 256):
        outs, clean = _chain_run(combined, B, nb, cuda)
        a.true(f"combined guards nb={nb}", clean)
        for i, (o, s) in enumerate(zip(outs, alone)):
            a.exact(f"combined nb={nb} layer{i} against the layer alone", o, s)
    a.check()


def _mixed_program(B, seed):
    """Three stages on 17 crops and a grid of 7: stage 1 = two layers of different N (8 tile jobs) + a broadcast of 157 floats and an
    aligned copy; stage 2 = a layer that reads stage 1's output (residual: an input) + a scalar copy of what stage 1 broadcast
    (n = 157) + a one-destination rot6d; stage 3 = a sigmoid layer on stage 2's output with stage 1's second layer as the residual
    (2 tile jobs: blocks 2..6 have none, and their prefetched weights are stale) + a two-destination rot6d of stage 2's output, an
    aligned copy and a copy into rows of an odd stride, dealt to the blocks from the last one down."""
    r = np.random.default_rng(seed)
    w = lambda n, k: (r.standard_normal((n, k)) / np.sqrt(k)).astype(np.float32)
    bias = lambda n: r.uniform(-0.5, 0.5, n).astype(np.float32)
    x = r.standard_normal((B, 144)).astype(np.float32)
    p6 = r.standard_normal((B, 144)).astype(np.float32)
    init = np.tile(r.standard_normal((1, 157)).astype(np.float32), (B, 1))      # a broadcast reads row 0
    layers = [dict(W=w(48, 144), b=bias(48), act=1, src=(0, 4), dst=(1, 4)),                       # A  stage 1
              dict(W=w(16, 144), b=bias(16), act=0, src=(0, 4), dst=(1, 56)),                      # B  stage 1
              dict(W=w(144, 48), b=bias(144), act=0, src=(1, 4), res=(0, 160), dst=(2, 0)),        # C  stage 2: reads A
              dict(W=w(16, 144), b=bias(16), act=2, src=(2, 0), res=(1, 56), dst=(2, 148))]        # D  stage 3: reads C and B
    rows = [dict(kind=1, src=(5, 0), dst=(2, 200), n=157),                                         # stage 1: broadcast
            dict(kind=0, src=(0, 4), dst=(2, 360), n=144),                                         # stage 1: aligned copy
            dict(kind=0, src=(2, 200), dst=(3, 224), n=157),                                       # stage 2: scalar copy (n = 157) of the broadcast
            dict(kind=2, src=(0, 160), dst=(6, 4)),                                                # stage 2: rot6d, one destination
            dict(kind=2, src=(2, 0), dst=(3, 4), dst2=(4, 1)),                                     # stage 3: rot6d of C, two destinations
            dict(kind=0, src=(1, 4), dst=(3, 384), n=48),                                          # stage 3: aligned copy of A
            dict(kind=0, src=(1, 56), dst=(4, 218), n=16)]                                         # stage 3: copy of B into odd-stride rows
    return dict(bufs=[(340, "nan"), (100, "poison"), (520, "poison"), (440, "poison"), (237, "poison"), (157, "nan"), (224, "poison")],
                inputs=[(0, 4, x), (0, 160, p6), (5, 0, init)], layers=layers, rows=rows,
                stages=[(0, 2, 0, 2), (2, 1, 2, 2), (3, 1, 4, 3)],
                outs=[(1, 4, 48, "linear"), (1, 56, 16, "linear"), (2, 0, 144, "linear"), (2, 148, 16, "sigmoid"), (2, 200, 157, "exact"),
                      (2, 360, 144, "exact"), (3, 224, 157, "exact"), (6, 4, 216, "rot6d"), (3, 4, 216, "rot6d"), (4, 1, 216, "rot6d"),
                      (3, 384, 48, "linear"), (4, 218, 16, "linear")])


@pytest.mark.parametrize("B", [1, 16, 17, 130])
def test_chain_three_stages(B, cuda):
    """The barrier and the agent-scope loads: every stage reads what the one before it wrote, on grids of 1, 7 and 256 blocks and
    over three consecutive calls on the same buffers - bitwise the same, rows >= B and every guard untouched."""
    p = _mixed_program(B, 77 + B)
    a = Acc()
    first, clean = _chain_run(p, B, 256, cuda)
    _chain_compare(a, f"B={B}", p, B, first)
    a.true("guards nb=256", clean)
    two = [o for (b, off, n, _), o in zip(p["outs"], first) if (b, off) in ((3, 4), (4, 1))]
    a.exact("the two destinations of a rot6d job", two[0], two[1])
    for nb, calls in ((1, 1), (7, 1), (7, 3), (256, 3)):
        outs, clean = _chain_run(p, B, nb, cuda, calls=calls)
        a.true(f"guards nb={nb} calls={calls}", clean)
        for (b, off, n, _), o, f in zip(p["outs"], outs, first):
            a.exact(f"nb={nb} calls={calls} buf{b}+{off}", o, f)
    a.check()


def test_chain_resident_blocks(cuda):
    assert ops.mlp_chain_resident_blocks() >= 1


# ---- part attention on planes smaller than the 14 pixel splits -----------------------------------------------------------------
@pytest.mark.parametrize("heat_cs", [32, 48])
@pytest.mark.parametrize("H,W", [(1, 1), (2, 2), (3, 3), (1, 5), (4, 4)])
def test_part_attention_tiny_planes(H, W, heat_cs, cuda):
    """1 ... 16 pixels for 14 splits: most splits are empty (local max -inf, denominator 0) and the combine must drop them.
    C = 64, 128: the MFMA form; 16, 32, 48, 96, 112: the VALU form with one or two slices per wave and waves without a slice.
    The background channel, the channels above 24 and the guard rows of the heat buffer are NaN."""
    a = Acc()
    for Cc in (16, 32, 48, 64, 96, 112, 128):
        r = np.random.default_rng(H * 100 + W * 10 + Cc)
        feat = r.standard_normal((2, Cc, H, W)).astype(np.float32)
        heat = (4.0 * r.standard_normal((2, 24, H, W))).astype(np.float32)
        out = ops.part_attention(_t(feat, cuda), _t(heat, cuda), heat_cs=heat_cs, poison=True).cpu().numpy()
        a.add("attention", f"{H}x{W} C={Cc} cs={heat_cs}", out, head_np.part_attention(feat, heat),
              head_np.part_attention(feat, heat, np.float32))
    a.check()


@pytest.mark.parametrize("Cc", [48, 64])
def test_part_attention_spread_logits(Cc, cuda):
    """Logits over +-30 on a 4x4 plane with every part's peak on the last pixel: the last non-empty split of either form."""
    r = np.random.default_rng(Cc)
    feat = r.standard_normal((2, Cc, 4, 4)).astype(np.float32)
    heat = r.uniform(-30.0, 28.0, (2, 24, 4, 4)).astype(np.float32)
    heat[:, :, 3, 3] = 30.0
    out = ops.part_attention(_t(feat, cuda), _t(heat, cuda), heat_cs=48, poison=True).cpu().numpy()
    a = Acc()
    a.add("attention.spread", f"C={Cc}", out, head_np.part_attention(feat, heat), head_np.part_attention(feat, heat, np.float32))
    a.check()


# ---- rot6d -------------------------------------------------------------------------------------------------------------------------
def _rot6d_rows(B, seed):
    """[B,24,6]: generic rows; joint 0 = a zero first column, 1 = a zero row, 2 = a second column parallel to the first (chosen so
    that the projection cancels exactly), 3 = a second column within 1e-4 of parallel."""
    r = np.random.default_rng(seed)
    x = r.standard_normal((B, 24, 3, 2)).astype(np.float32)
    x[:, 0, :, 0] = 0.0
    x[:, 0, :, 1] = (0.0, 3.0, 4.0)
    x[:, 1] = 0.0
    x[:, 2, :, 0] = (2.0, 0.0, 0.0)
    x[:, 2, :, 1] = (-3.0, 0.0, 0.0)
    a1 = x[:, 3, :, 0].astype(np.float64)
    perp = np.cross(a1, np.array([0.3, -0.5, 0.8]))
    x[:, 3, :, 1] = (1.7 * a1 + 1e-4 * np.linalg.norm(a1, axis=-1, keepdims=True) * perp / np.linalg.norm(perp, axis=-1, keepdims=True)).astype(np.float32)
    return x.reshape(B, 24, 6)


# F.normalize's clamp written out: a zero column stays zero (0 / 1e-12), and so does everything built from it
ROT6D_DEGENERATE = {0: [[0, 0, 0], [0, 0.6, 0], [0, 0.8, 0]],          # b1 = 0, b2 = a2 / |a2|, b3 = 0 x b2 = 0
                    1: [[0, 0, 0], [0, 0, 0], [0, 0, 0]],
                    2: [[1, 0, 0], [0, 0, 0], [0, 0, 0]]}              # b1 = e_x, u = a2 - (a2 . b1) b1 = 0 exactly, b2 = b3 = 0


def _rot6d_compare(a, label, out, x):
    B = x.shape[0]
    out = out.reshape(B, 24, 3, 3)
    ref, r32 = head_np.rot6d(x), head_np.rot6d(x, np.float32)
    gen = [j for j in range(24) if j != 3]
    a.add("rot6d", label, out[:, gen], ref[:, gen], r32[:, gen])
    a.add("rot6d.near_parallel", label, out[:, 3], ref[:, 3], r32[:, 3])
    for j, want in ROT6D_DEGENERATE.items():
        want = np.tile(np.array(want, np.float64), (B, 1, 1))
        a.true(f"{label} joint {j}: the reference is the written-out value", np.abs(ref[:, j] - want).max() < 1e-15)
        a.true(f"{label} joint {j}: zeros are exact zeros", bool((out[:, j][want == 0] == 0).all()))
        if want.any():
            a.add("rot6d", f"{label} degenerate joint {j}", out[:, j], want, r32[:, j])


@pytest.mark.parametrize("dst", ["dst0", "dst1", "both"])
@pytest.mark.parametrize("B,in_stride", [(1, 144), (5, 160), (5, 144), (1, 160)])
def test_rot6d_ex(B, in_stride, dst, cuda):
    x = _rot6d_rows(B, 10 * B + in_stride)
    o0, o1, w0, w1 = ops.rot6d_ex(_t(x.reshape(B, 144), cuda), in_stride=in_stride, stride0=216 if B == 1 else 220, stride1=231,
                                  dst0=dst != "dst1", dst1=dst != "dst0")
    a = Acc()
    for name, o, w in (("dst0", o0, w0), ("dst1", o1, w1)):
        if o is not None:
            _rot6d_compare(a, f"B={B} {name}", o.cpu().numpy(), x)
            a.true(name + " guards", w.untouched([(0, 216)]))
    if dst == "both":
        a.exact("both destinations", o0.cpu().numpy(), o1.cpu().numpy())
    a.check()


def test_chain_rot6d_is_bitwise_the_rot6d_kernel(cuda):
    """csrc/mlp_chain.hip says rot6d_one has "the same operation order as rot6d_kernel": the same rows through an mlp_chain ROT6D
    job and through poco_op_rot6d_ex, degenerate rows included."""
    B = 5
    x = _rot6d_rows(B, 4242).reshape(B, 144)
    o0, _, _, _ = ops.rot6d_ex(_t(x, cuda), in_stride=160)
    p = dict(bufs=[(160, "nan"), (220, "poison")], inputs=[(0, 0, x)], layers=[], rows=[dict(kind=2, src=(0, 0), dst=(1, 4))],
             stages=[(0, 0, 0, 1)], outs=[(1, 4, 216, "rot6d")])
    outs, clean = _chain_run(p, B, 256, cuda)
    a = Acc()
    a.true("guards", clean)
    a.exact("rot6d_one against rot6d_kernel", outs[0], o0.cpu().numpy())
    a.check()


# ---- lc2d, row copies, NHWC -> NCHW, pack_record ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 7])
@pytest.mark.parametrize("x_stride", [3072, 3100])
def test_lc2d_pose_ex(x_stride, B, cuda):
    r = np.random.default_rng(B + x_stride)
    x = r.standard_normal((B, 128, 24)).astype(np.float32)
    w = (r.standard_normal((6, 128, 24)) / np.sqrt(128)).astype(np.float32)
    out, wo = ops.lc2d_pose_ex(_t(x, cuda), _t(w, cuda), x_stride=x_stride)
    a = Acc()
    a.add("lc2d", f"B={B} stride {x_stride}", out.cpu().numpy(), head_np.lc2d(x, w), head_np.lc2d(x, w, np.float32))
    a.true("guards", wo.untouched([(0, 144)]))
    a.check()


@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("n", [1, 3, 157, 1024])
def test_copy_and_broadcast_rows(n, B, cuda):
    r = np.random.default_rng(n + B)
    x = r.standard_normal((B, n)).astype(np.float32)
    a = Acc()
    out, wo = ops.copy_rows(_t(x, cuda), src_stride=n + 5, dst_stride=n + 12)
    a.exact("copy", out.cpu().numpy(), x)
    a.true("copy guards", wo.untouched([(0, n)]))
    out, wo = ops.broadcast_rows(_t(x[0], cuda), B, dst_stride=n + 3)
    a.exact("broadcast", out.cpu().numpy(), np.tile(x[:1], (B, 1)))
    a.true("broadcast guards", wo.untouched([(0, n)]))
    a.check()


@pytest.mark.parametrize("B,H,W,Cx,cs,Cc", [(2, 3, 5, 16, 48, 16), (1, 1, 1, 32, 32, 32), (3, 7, 7, 32, 64, 32)])
def test_nhwc_to_nchw(B, H, W, Cx, cs, Cc, cuda):
    """The first Cc channels of an L16 buffer with cs channels per pixel (the rest NaN) as dense NCHW; the third case is the
    PARE head's 24 part maps, padded to 32 channels, out of a 64-channel buffer."""
    x = np.random.default_rng(B * H + cs).standard_normal((B, H, W, Cx)).astype(np.float32)
    out, wo = ops.nhwc_to_nchw(_t(x, cuda), cs=cs, C_out=Cc)
    a = Acc()
    a.exact("nchw", out.cpu().numpy(), np.ascontiguousarray(x[..., :Cc].transpose(0, 3, 1, 2)))
    a.true("guards", wo.untouched([(0, B * Cc * H * W)]))
    a.check()


@pytest.mark.parametrize("B", [1, 9])
@pytest.mark.parametrize("kinematic", [0, 1])
@pytest.mark.parametrize("cliff", [0, 1])
def test_pack_record(cliff, kinematic, B, cuda):
    """The layout of poco_amd.dist.pack_records ([rotmat 216 | betas 10 | cam 3 | var 24 | confidence 1]) from rows of strides 220 /
    13 / 7 / 29: the copied fields bitwise, the confidence against fp64 with roots on both sides of the threshold."""
    from poco_amd import dist
    r = np.random.default_rng(17 * B + 2 * cliff + kinematic)
    rot, betas, cam = (r.standard_normal((B, k)).astype(np.float32) for k in (216, 10, 3))
    var = r.uniform(0.0, 0.06, (B, 24)).astype(np.float32)
    var[::2, 0] = r.uniform(0.1, 0.7, len(var[::2]))                       # B = 9: roots below and above thr and 2 thr
    var[-1, 0] = 1.3
    thr = 0.4
    rec, wo = ops.pack_record(_t(rot, cuda), _t(betas, cuda), _t(cam, cuda), _t(var, cuda), cliff=cliff, kinematic=kinematic, thr=thr,
                              rot_stride=220, betas_stride=13, cam_stride=7, var_stride=29)
    rec = rec.cpu().numpy()
    a = Acc()
    assert dist.REC == 254 and dist.FIELDS == (("pred_pose", 0, 216), ("pred_shape", 216, 226), ("pred_cam", 226, 229),
                                               ("var_pose", 229, 253), ("var_global", 253, 254))
    for (name, lo, hi), src in zip(dist.FIELDS[:4], (rot, betas, cam, var)):
        a.exact(name, rec[:, lo:hi], src)
    a.add("record.confidence", f"cliff={cliff} kin={kinematic} B={B}", rec[:, 253], head_np.confidence(var, cliff, kinematic, np.float32(thr)),
          head_np.confidence(var, cliff, kinematic, np.float32(thr), np.float32))
    a.true("guards", wo.untouched([(0, 254)]))
    a.check()


# ---- argument errors ---------------------------------------------------------------------------------------------------------------
def bad_calls(L, p, out):
    """[(entry, status)]: every new entry with a null pointer, B = 0 and one out-of-range size.  `p` = a readable operand, `out` =
    the output pointer (never reached: all of this is refused before any GPU work; tests/test_ops_capi_cpu.py runs the same list
    with fake pointers on a machine without a GPU)."""
    N, S, f = C.c_void_p(0), C.c_void_p(0), C.c_float(0.4)
    one = (C.c_int * 12)(16, 16, 0, 0, 0, 16, -1, 0, 0, 0, 16, 32)         # a 16 -> 16 layer: buffer 0 columns 0..15 -> 16..31
    bad_k = (C.c_int * 12)(24, 16, 0, 0, 0, 32, -1, 0, 0, 0, 0, 32)
    st = (C.c_int * 4)(0, 1, 0, 0)
    w = np.zeros(16 * 24, np.float32)
    wp, bp = (C.c_void_p * 1)(w.ctypes.data), (C.c_void_p * 1)(w.ctypes.data)
    bufs, sizes, small = (C.c_void_p * 1)(out.value), (C.c_longlong * 1)(64), (C.c_longlong * 1)(24)
    nobuf = (C.c_void_p * 1)(0)
    chain = lambda layers=one, nl=1, wts=wp, ns=1, bf=bufs, sz=sizes, B=1, nb=4: \
        L.poco_op_mlp_chain(layers, nl, wts, bp, None, 0, st, ns, bf, sz, 1, B, nb, S)
    return [
        ("rot6d_ex", L.poco_op_rot6d_ex(N, 144, out, 216, N, 0, 1, S)), ("rot6d_ex", L.poco_op_rot6d_ex(p, 144, N, 216, N, 216, 1, S)),
        ("rot6d_ex", L.poco_op_rot6d_ex(p, 144, out, 216, N, 0, 0, S)), ("rot6d_ex", L.poco_op_rot6d_ex(p, 143, out, 216, N, 0, 1, S)),
        ("rot6d_ex", L.poco_op_rot6d_ex(p, 144, out, 215, N, 0, 1, S)),
        ("lc2d_pose_ex", L.poco_op_lc2d_pose_ex(N, 3072, p, out, 1, S)), ("lc2d_pose_ex", L.poco_op_lc2d_pose_ex(p, 3072, p, N, 1, S)),
        ("lc2d_pose_ex", L.poco_op_lc2d_pose_ex(p, 3072, p, out, 0, S)), ("lc2d_pose_ex", L.poco_op_lc2d_pose_ex(p, 3071, p, out, 1, S)),
        ("copy_rows", L.poco_op_copy_rows(N, 8, out, 8, 8, 1, S)), ("copy_rows", L.poco_op_copy_rows(p, 8, N, 8, 8, 1, S)),
        ("copy_rows", L.poco_op_copy_rows(p, 8, out, 8, 8, 0, S)), ("copy_rows", L.poco_op_copy_rows(p, 8, out, 7, 8, 1, S)),
        ("copy_rows", L.poco_op_copy_rows(p, 8, out, 8, 0, 1, S)),
        ("broadcast_rows", L.poco_op_broadcast_rows(N, out, 8, 8, 1, S)), ("broadcast_rows", L.poco_op_broadcast_rows(p, N, 8, 8, 1, S)),
        ("broadcast_rows", L.poco_op_broadcast_rows(p, out, 8, 8, 0, S)), ("broadcast_rows", L.poco_op_broadcast_rows(p, out, 7, 8, 1, S)),
        ("nhwc_to_nchw", L.poco_op_nhwc_to_nchw(N, 16, out, 1, 1, 1, 16, S)), ("nhwc_to_nchw", L.poco_op_nhwc_to_nchw(p, 16, N, 1, 1, 1, 16, S)),
        ("nhwc_to_nchw", L.poco_op_nhwc_to_nchw(p, 16, out, 0, 1, 1, 16, S)), ("nhwc_to_nchw", L.poco_op_nhwc_to_nchw(p, 16, out, 1, 1, 1, 17, S)),
        ("nhwc_to_nchw", L.poco_op_nhwc_to_nchw(p, 24, out, 1, 1, 1, 16, S)),
        ("pack_record", L.poco_op_pack_record(N, 216, p, 10, p, 3, p, 24, out, 1, 1, f, 1, S)),
        ("pack_record", L.poco_op_pack_record(p, 216, p, 10, p, 3, p, 24, N, 1, 1, f, 1, S)),
        ("pack_record", L.poco_op_pack_record(p, 216, p, 10, p, 3, p, 24, out, 1, 1, f, 0, S)),
        ("pack_record", L.poco_op_pack_record(p, 216, p, 10, p, 3, p, 23, out, 1, 1, f, 1, S)),
        ("pack_record", L.poco_op_pack_record(p, 216, p, 10, p, 3, p, 24, out, 2, 1, f, 1, S)),
        ("camera", L.poco_op_camera(N, 3, p, 0, N, N, N, N, out, N, out, 1, S)), ("camera", L.poco_op_camera(p, 3, p, 0, N, N, N, N, N, N, out, 1, S)),
        ("camera", L.poco_op_camera(p, 3, p, 1, p, p, N, p, out, N, out, 1, S)),         # cliff without d_center
        ("camera", L.poco_op_camera(p, 3, p, 0, N, N, N, N, out, N, out, 0, S)), ("camera", L.poco_op_camera(p, 2, p, 0, N, N, N, N, out, N, out, 1, S)),
        ("mlp_chain", chain(wts=None)), ("mlp_chain", chain(bf=nobuf)), ("mlp_chain", chain(B=0)), ("mlp_chain", chain(nb=0)),
        ("mlp_chain", chain(layers=bad_k)),                                               # K = 24
        ("mlp_chain", chain(sz=small)),                                                   # the output slice ends beyond the buffer
        ("mlp_chain", chain(nl=17)), ("mlp_chain", chain(ns=15)), ("mlp_chain", chain(ns=0)),
    ]


def test_argument_errors_leave_the_output_untouched(cuda):
    L = lib()
    src = ops.Rows(1, 4096, cuda, "nan")
    out = ops.Rows(1, 4096, cuda, "poison")
    for who, rc in bad_calls(L, src.ptr(), out.ptr()):
        assert rc == 1, who
    torch.cuda.synchronize()
    assert out.untouched([])
    with pytest.raises(PocoHipError, match="mlp_chain"):
        ops.mlp_chain([dict(W=np.zeros((16, 16), np.float32), b=np.zeros(16, np.float32), src=(0, 2), dst=(0, 16))], [], [(0, 1, 0, 0)],
                      [ops.Rows(1, 32, cuda, "poison")], 1)
