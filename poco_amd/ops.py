"""Python wrappers of the stand-alone HIP operators (thin: pointers in, pointers out)."""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from ._lib import PocoHipError, check, current_stream, fptr, iptr, lib


def _cfg(cfg):
    if cfg is None:
        return C.c_void_p(0), None
    arr = (C.c_int * 7)(*(tuple(cfg) + (0,) * (7 - len(cfg))))
    return C.cast(arr, C.c_void_p), arr


def to_l16(x: torch.Tensor) -> torch.Tensor:
    """NHWC [B,H,W,C] (C % 16 == 0) -> the library's activation layout [B,H,C/16,W,16] (csrc/common.h)."""
    B, H, W, C = x.shape
    assert C % 16 == 0
    return x.view(B, H, W, C // 16, 16).permute(0, 1, 3, 2, 4).contiguous()


def from_l16(y: torch.Tensor) -> torch.Tensor:
    """[B,H,C/16,W,16] -> NHWC [B,H,W,C]."""
    B, H, C16, W, _ = y.shape
    return y.permute(0, 1, 3, 2, 4).reshape(B, H, W, C16 * 16).contiguous()


# ---- poisoned wide buffers (tests): what a kernel must not write keeps a bit pattern, what it must not read is NaN ----------
POISON_BITS = 0x5A5AA5A5          # a finite float (1.54e16): "nobody may write here"; compared bitwise


class Wide:
    """An L16 activation buffer [B,H,cs/16,W,16] inside one allocation with a guard band of `guard_rows` image rows of the buffer
    (cs * W floats each) before and after it.  fill = "nan" (inputs: everything outside the slice the kernel may read is NaN, so
    foreign memory that enters the arithmetic - even times a zero weight - shows in the result) or "poison" (outputs: POISON_BITS
    everywhere the kernel must not write; the slice it must write is NaN, so an unwritten element shows too)."""

    def __init__(self, B, H, W, cs, device, fill, guard_rows=1):
        assert fill in ("nan", "poison") and cs % 4 == 0 and (cs % 16 == 0 or H * W == 1)
        self.B, self.H, self.W, self.cs = B, H, W, cs
        self.guard = guard_rows * cs * W
        n = B * H * W * cs
        self.flat = torch.empty(n + 2 * self.guard, device=device, dtype=torch.float32)
        if fill == "nan":
            self.flat.fill_(float("nan"))
        else:
            self.flat.view(torch.int32).fill_(POISON_BITS)
        self.body = self.flat[self.guard:self.guard + n]

    def _mask_or_view(self, co, C):
        if self.H * self.W == 1:                       # rows: plain [B][cs], offsets in multiples of 4
            return self.body.view(self.B, self.cs)[:, co:co + C]
        assert co % 16 == 0 and C % 16 == 0
        return self.body.view(self.B, self.H, self.cs // 16, self.W, 16)[:, :, co // 16:(co + C) // 16]

    def put(self, co, x_nhwc):
        """Write an NHWC tensor into channels [co, co + C)."""
        C = x_nhwc.shape[-1]
        if self.H * self.W == 1:
            self._mask_or_view(co, C).copy_(x_nhwc.reshape(self.B, C))
        else:
            self._mask_or_view(co, C).copy_(to_l16(x_nhwc.contiguous()))
        return self

    def fill(self, co, C, value):
        self._mask_or_view(co, C).fill_(value)
        return self

    def get(self, co, C):
        """Channels [co, co + C) as NHWC."""
        v = self._mask_or_view(co, C)
        if self.H * self.W == 1:
            return v.reshape(self.B, 1, 1, C).contiguous()
        return from_l16(v.contiguous())

    def outside_bits(self, co, C):
        """int32 bits of every element of the allocation outside channels [co, co + C): guard bands and neighbouring channels."""
        keep = torch.ones_like(self.flat, dtype=torch.bool)
        kb = keep[self.guard:self.guard + self.body.numel()]
        if self.H * self.W == 1:
            kb.view(self.B, self.cs)[:, co:co + C] = False
        else:
            kb.view(self.B, self.H, self.cs // 16, self.W, 16)[:, :, co // 16:(co + C) // 16] = False
        return self.flat.view(torch.int32)[keep]

    def untouched(self, co, C):
        """True if nothing outside channels [co, co + C) was written (bitwise)."""
        return bool((self.outside_bits(co, C) == POISON_BITS).all())

    def ptr(self, co=0):
        """Device pointer of the first channel of the slice at `co` (csrc/common.h l16_chan_off), as the engine's aptr()."""
        off = (co >> 4) * self.W * 16 + (co & 15)
        return C.c_void_p(self.body.data_ptr() + 4 * off)

    def base(self):
        return C.c_void_p(self.body.data_ptr())


class Rows:
    """The flat form of Wide for row-vector data at any stride: `B + extra_rows` rows of `stride` floats in one allocation with a
    guard band (at least one row, a multiple of 4 floats: the body stays 16-byte aligned) before and after them.  fill = "nan"
    (operands: whatever the kernel may not read is NaN) or "poison" (POISON_BITS).  put() writes an operand into a column slice of
    the first B rows, mark() makes a slice NaN (an output the kernel must write: an element it leaves out shows), untouched()
    compares everything else - guard bands, the other columns, the rows from B on - bitwise with the fill."""

    def __init__(self, B, stride, device, fill, extra_rows=0):
        assert fill in ("nan", "poison") and B >= 1 and stride >= 1
        self.B, self.stride, self.rows = B, stride, B + extra_rows
        self.guard = (max(stride, 64) + 3) // 4 * 4
        n = self.rows * stride
        self.flat = torch.empty(n + 2 * self.guard, device=device, dtype=torch.float32)
        if fill == "nan":
            self.flat.fill_(float("nan"))
        else:
            self.flat.view(torch.int32).fill_(POISON_BITS)
        self.fill_bits = int(self.flat[:1].view(torch.int32).item())
        self.body = self.flat[self.guard:self.guard + n].view(self.rows, stride)

    def put(self, off, x):
        x = x.reshape(self.B, -1)
        self.body[:self.B, off:off + x.shape[1]].copy_(x)
        return self

    def mark(self, off, n):
        self.body[:self.B, off:off + n].fill_(float("nan"))
        return self

    def get(self, off, n):
        return self.body[:self.B, off:off + n].contiguous()

    def untouched(self, slices):
        """True if nothing outside the column slices [(off, n), ...] of the first B rows differs from the fill (bitwise)."""
        keep = torch.ones_like(self.flat, dtype=torch.bool)
        kb = keep[self.guard:self.guard + self.rows * self.stride].view(self.rows, self.stride)
        for off, n in slices:
            kb[:self.B, off:off + n] = False
        return bool((self.flat.view(torch.int32)[keep] == self.fill_bits).all())

    def ptr(self, off=0):
        return C.c_void_p(self.body.data_ptr() + 4 * off)


def _out_hw(H, W, ks, stride):
    pad = (ks - 1) // 2
    return (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1


def conv2d_view(x: torch.Tensor, weight: np.ndarray, scale=None, shift=None, stride=1, residual=None, *, in_cs=None, in_co=0,
                res_cs=None, res_co=0, out_cs=None, out_co=0, act=0, relu_from=0, res_after_act=0, cfg=None):
    """poco_op_conv2d_ex: the conv on channel slices of wider L16 buffers, with every epilogue form (include/poco_hip.h).
    x [B,H,W,Cin] / residual [B,Ho,Wo,Cout] NHWC cuda tensors are placed at channel offset in_co / res_co of poisoned buffers with
    in_cs / res_cs channels; residual = "input" makes the input buffer double as the residual (BasicBlock conv2: needs Cin == Cout,
    stride 1).  Returns (out NHWC [B,Ho,Wo,Cout] = channels [out_co, out_co + Cout) of the output buffer, that buffer as a Wide):
    the caller checks `wide.untouched(out_co, Cout)` and that `out` holds no NaN."""
    assert x.is_cuda and x.dtype == torch.float32
    B, H, W, Cin = x.shape
    Cout, Cin2, ks, ks2 = weight.shape
    assert Cin2 == Cin and ks == ks2
    Ho, Wo = _out_hw(H, W, ks, stride)
    in_cs = Cin if in_cs is None else in_cs
    out_cs = Cout if out_cs is None else out_cs
    res_cs = Cout if res_cs is None else res_cs
    win = Wide(B, H, W, in_cs, x.device, "nan").put(in_co, x)
    if isinstance(residual, str):
        assert residual == "input" and Cin == Cout and stride == 1
        wres, res_cs, res_co = win, in_cs, in_co
    elif residual is not None:
        wres = Wide(B, Ho, Wo, res_cs, x.device, "nan").put(res_co, residual)
    else:
        wres = None
    wout = Wide(B, Ho, Wo, out_cs, x.device, "poison").fill(out_co, Cout, float("nan"))
    weight = np.ascontiguousarray(weight, dtype=np.float32)
    scale = None if scale is None else np.ascontiguousarray(scale, dtype=np.float32)
    shift = None if shift is None else np.ascontiguousarray(shift, dtype=np.float32)
    cptr, _keep = _cfg(cfg)
    rc = lib().poco_op_conv2d_ex(win.base(), B, H, W, Cin, in_cs, in_co, fptr(weight), fptr(scale), fptr(shift), Cout, ks, stride,
                                 C.c_void_p(0) if wres is None else wres.base(), res_cs, res_co, int(act), int(relu_from),
                                 int(res_after_act), wout.base(), out_cs, out_co, cptr, current_stream())
    check(rc, "poco_op_conv2d_ex")
    return wout.get(out_co, Cout), wout


def conv2d_nhwc(x: torch.Tensor, weight: np.ndarray, scale=None, shift=None, stride=1, residual=None,
                relu=False, cfg=None) -> torch.Tensor:
    """x [B,H,W,Cin] cuda fp32 NHWC; weight OIHW numpy fp32 (host). Returns NHWC output."""
    assert x.is_cuda and x.dtype == torch.float32 and x.is_contiguous()
    B, H, W, Cin = x.shape
    Cout, Cin2, ks, ks2 = weight.shape
    assert Cin2 == Cin and ks == ks2
    Ho, Wo = _out_hw(H, W, ks, stride)
    # the operator works on the library's L16 layout; Cin/Cout are padded to multiples of 16 inside the op,
    # so NHWC tensors are converted here (tests / tuning only - the engine never leaves L16)
    assert Cin % 16 == 0 and Cout % 16 == 0, "conv2d_nhwc: channel counts must be multiples of 16"
    # the output starts as NaN between poisoned guard bands: an element the kernel leaves unwritten stays NaN in the result (the
    # caching allocator would otherwise hand back the previous, correct answer), a store outside the tensor raises below
    wout = Wide(B, Ho, Wo, Cout, x.device, "poison").fill(0, Cout, float("nan"))
    weight = np.ascontiguousarray(weight, dtype=np.float32)
    scale = None if scale is None else np.ascontiguousarray(scale, dtype=np.float32)
    shift = None if shift is None else np.ascontiguousarray(shift, dtype=np.float32)
    cptr, _keep = _cfg(cfg)
    xl = to_l16(x)
    rl = None if residual is None else to_l16(residual)
    rc = lib().poco_op_conv2d(fptr(xl), B, H, W, Cin, fptr(weight), fptr(scale), fptr(shift), Cout, ks,
                              stride, fptr(rl), int(relu), wout.base(), cptr, current_stream())
    check(rc, "poco_op_conv2d")
    if not wout.untouched(0, Cout):
        raise PocoHipError("poco_op_conv2d wrote outside its output tensor (guard band changed)")
    return wout.get(0, Cout)


def bench_conv2d(x: torch.Tensor, weight: np.ndarray, stride=1, cfg=None, iters=20):
    B, H, W, Cin = x.shape
    Cout, _, ks, _ = weight.shape
    pad = (ks - 1) // 2
    Ho = (H + 2 * pad - ks) // stride + 1
    Wo = (W + 2 * pad - ks) // stride + 1
    out = torch.empty((B, Ho, Wo, Cout), device=x.device, dtype=torch.float32)
    weight = np.ascontiguousarray(weight, dtype=np.float32)
    ms = C.c_float(0)
    used = (C.c_int * 7)()
    cptr, _keep = _cfg(cfg)
    rc = lib().poco_bench_conv2d(fptr(x), B, H, W, Cin, fptr(weight), Cout, ks, stride, fptr(out), cptr,
                                 iters, C.byref(ms), used, current_stream())
    check(rc, "poco_bench_conv2d")
    flops = 2.0 * B * Ho * Wo * Cout * Cin * ks * ks
    return ms.value, flops / (ms.value * 1e-3) / 1e12, tuple(used)


def part_attention(feat_nchw: torch.Tensor, heat_nchw: torch.Tensor, *, heat_cs: int = 32, poison: bool = False) -> torch.Tensor:
    """KeypointAttention as the PARE head uses it: feat [B,C,H,W], heat [B,24,H,W] (the 24 part maps, no background channel)
    -> [B,C,24].  Channels are padded to the library's L16 layout here (tests only; the engine never leaves L16).  The heat map
    is channels 1..24 of a buffer with heat_cs channels per pixel.  poison: every other channel of that buffer (the background
    channel 0, 25 and above) and the guard rows around both inputs are NaN, and the output lies between poisoned guard bands
    (a store outside it raises)."""
    B, Cc, H, W = feat_nchw.shape
    assert heat_nchw.shape == (B, 24, H, W) and feat_nchw.is_cuda and heat_cs >= 32 and heat_cs % 16 == 0
    dev = feat_nchw.device
    C16 = (Cc + 15) // 16 * 16
    f = torch.zeros((B, H, W, C16), device=dev)
    f[..., :Cc] = feat_nchw.permute(0, 2, 3, 1)
    h = torch.full((B, H, W, heat_cs), float("nan") if poison else 0.0, device=dev)
    h[..., 1:25] = heat_nchw.permute(0, 2, 3, 1)            # channel 0 = background, skipped by the kernel
    if not poison:
        fl, hl = to_l16(f), to_l16(h)
        out = torch.empty((B, C16, 24), device=dev)
        check(lib().poco_op_part_attention(fptr(hl), heat_cs, fptr(fl), C16, B, H, W, fptr(out), current_stream()),
              "poco_op_part_attention")
        return out[:, :Cc]
    wh = Wide(B, H, W, heat_cs, dev, "nan").put(0, h)
    wf = Wide(B, H, W, C16, dev, "nan").put(0, f)
    wo = Rows(B, C16 * 24, dev, "poison").mark(0, C16 * 24)
    check(lib().poco_op_part_attention(wh.base(), heat_cs, wf.base(), C16, B, H, W, wo.ptr(), current_stream()),
          "poco_op_part_attention")
    if not wo.untouched([(0, C16 * 24)]):
        raise PocoHipError("poco_op_part_attention wrote outside its output tensor (guard band changed)")
    return wo.get(0, C16 * 24).view(B, C16, 24)[:, :Cc]


def lc2d_pose(x: torch.Tensor, w: torch.Tensor) -> torch.Tensor:
    """x [B,128,24] , w [6,128,24] -> [B,24,6] (LocallyConnected2d 128 -> 6 per joint)."""
    B = x.shape[0]
    assert x.shape[1:] == (128, 24) and w.shape == (6, 128, 24) and x.is_cuda
    out = torch.empty((B, 24, 6), device=x.device)
    check(lib().poco_op_lc2d_pose(fptr(x.contiguous()), fptr(w.contiguous()), fptr(out), B, current_stream()), "poco_op_lc2d_pose")
    return out


def rot6d(x: torch.Tensor) -> torch.Tensor:
    """x [B,24,6] (each row = a 3x2 matrix, row-major as in the reference) -> rotation matrices [B,24,3,3]."""
    B = x.shape[0]
    assert x.shape[1:] == (24, 6) and x.is_cuda
    out = torch.empty((B, 24, 3, 3), device=x.device)
    check(lib().poco_op_rot6d(fptr(x.contiguous()), fptr(out), B, current_stream()), "poco_op_rot6d")
    return out


def rodrigues(aa: torch.Tensor) -> torch.Tensor:
    """batch_rodrigues (geometry.py:207-244): axis-angle [..., 3] -> rotation matrices [..., 3, 3]; [B,72] gives [B,24,3,3]."""
    assert aa.is_cuda and aa.dtype == torch.float32 and aa.shape[-1] % 3 == 0 and aa.numel() > 0
    a = aa.contiguous().view(-1, 3)
    out = torch.empty((a.shape[0], 3, 3), device=aa.device)
    check(lib().poco_op_rodrigues(fptr(a), fptr(out), a.shape[0], current_stream()), "poco_op_rodrigues")
    if aa.shape[-1] == 3:
        return out.view(*aa.shape[:-1], 3, 3)
    return out.view(*aa.shape[:-1], aa.shape[-1] // 3, 3, 3)


def rotmat_to_aa(rotmat: torch.Tensor) -> torch.Tensor:
    """rotation_matrix_to_angle_axis (geometry.py:264-429, the reference's quaternion route): rotation matrices [..., 3, 3] ->
    axis-angle [..., 3]; a matrix holding a NaN gives zeros."""
    assert rotmat.is_cuda and rotmat.dtype == torch.float32 and rotmat.shape[-2:] == (3, 3) and rotmat.numel() > 0
    r = rotmat.contiguous().view(-1, 3, 3)
    out = torch.empty((r.shape[0], 3), device=rotmat.device)
    check(lib().poco_op_rotmat_to_aa(fptr(r), fptr(out), r.shape[0], current_stream()), "poco_op_rotmat_to_aa")
    return out.view(*rotmat.shape[:-2], 3)


# ---- backbone side kernels and fused launches on their own (include/poco_hip.h; tests/test_engine_kernels_gpu.py) -----------
def _f32(a):
    return None if a is None else np.ascontiguousarray(a, dtype=np.float32)


def bneck_chain(t, res, w3, scale3, shift3, w1, scale1, shift1, *, t_cs=64, t_co=0, res_cs=256, res_co=0, y_cs=256, y_co=0,
                u_cs=64, u_co=0):
    """y = ReLU(bn3(conv3(t)) + res), u = ReLU(bn1(conv1(y))) (poco_op_bneck_chain): t [B,H,W,64], res [B,H,W,256] NHWC, each
    operand a slice at *_co of a poisoned buffer with *_cs channels.  Returns (y, u, y buffer, u buffer)."""
    B, H, W, _ = t.shape
    wt = Wide(B, H, W, t_cs, t.device, "nan").put(t_co, t)
    wr = Wide(B, H, W, res_cs, t.device, "nan").put(res_co, res)
    wy = Wide(B, H, W, y_cs, t.device, "poison").fill(y_co, 256, float("nan"))
    wu = Wide(B, H, W, u_cs, t.device, "poison").fill(u_co, 64, float("nan"))
    w3, scale3, shift3, w1, scale1, shift1 = map(_f32, (w3, scale3, shift3, w1, scale1, shift1))
    check(lib().poco_op_bneck_chain(wt.ptr(t_co), t_cs, wr.ptr(res_co), res_cs, wy.ptr(y_co), y_cs, wu.ptr(u_co), u_cs, fptr(w3),
                                    fptr(scale3), fptr(shift3), fptr(w1), fptr(scale1), fptr(shift1), B, H, W, current_stream()),
          "poco_op_bneck_chain")
    return wy.get(y_co, 256), wu.get(u_co, 64), wy, wu


def bneck_chain_resident_tiles() -> int:
    return int(lib().poco_op_bneck_chain_resident_tiles())


def conv1x1_dual(a, b, wa, scale_a, shift_a, wb, scale_b, shift_b, stride2=2, act=1, wave_layout=0, *, a_cs=None, a_co=0,
                 b_cs=None, b_co=0, out_cs=None, out_co=0):
    """act(bn3(conv3(a)) + bn_d(conv_d(b, stride2))) as one GEMM (poco_op_conv1x1_dual): a [B,Ho,Wo,Ca], b [B,H2,W2,Cb] NHWC.
    Returns (out NHWC, output buffer)."""
    B, Ho, Wo, Ca = a.shape
    _, H2, W2, Cb = b.shape
    Cout = wa.shape[0]
    a_cs, b_cs, out_cs = a_cs or Ca, b_cs or Cb, out_cs or Cout
    wa_ = Wide(B, Ho, Wo, a_cs, a.device, "nan").put(a_co, a)
    wb_ = Wide(B, H2, W2, b_cs, a.device, "nan").put(b_co, b)
    wo = Wide(B, Ho, Wo, out_cs, a.device, "poison").fill(out_co, Cout, float("nan"))
    wa, scale_a, shift_a, wb, scale_b, shift_b = map(_f32, (wa, scale_a, shift_a, wb, scale_b, shift_b))
    check(lib().poco_op_conv1x1_dual(wa_.ptr(a_co), a_cs, Ca, wb_.ptr(b_co), b_cs, Cb, H2, W2, stride2, fptr(wa), fptr(scale_a),
                                     fptr(shift_a), fptr(wb), fptr(scale_b), fptr(shift_b), wo.ptr(out_co), out_cs, Cout, B, Ho, Wo,
                                     int(act), int(wave_layout), current_stream()), "poco_op_conv1x1_dual")
    return wo.get(out_co, Cout), wo


def fuse_sum(terms, shifts, relu, *, src_cs=None, src_co=None, out_cs=None, out_co=0):
    """[ReLU](sum_k term_k upsampled by 2^shift_k) (poco_op_fuse_sum): terms = NHWC tensors [B, H >> s, W >> s, C].
    Returns (out NHWC [B,H,W,C], output buffer)."""
    n = len(terms)
    Cc = terms[0].shape[-1]
    B = terms[0].shape[0]
    H, W = max(t.shape[1] << s for t, s in zip(terms, shifts)), max(t.shape[2] << s for t, s in zip(terms, shifts))
    src_cs = list(src_cs or [Cc] * n)
    src_co = list(src_co or [0] * n)
    out_cs = out_cs or Cc
    ws = [Wide(B, t.shape[1], t.shape[2], cs, t.device, "nan").put(co, t) for t, cs, co in zip(terms, src_cs, src_co)]
    wo = Wide(B, H, W, out_cs, terms[0].device, "poison").fill(out_co, Cc, float("nan"))
    ptrs = (C.c_void_p * n)(*[w.ptr(co).value for w, co in zip(ws, src_co)])
    check(lib().poco_op_fuse_sum(n, ptrs, (C.c_int * n)(*src_cs), (C.c_int * n)(*shifts), wo.ptr(out_co), out_cs, B, H, W, Cc,
                                 int(relu), current_stream()), "poco_op_fuse_sum")
    return wo.get(out_co, Cc), wo


def bilinear_up2x(x):
    """x2 bilinear, align_corners=True (poco_op_bilinear_up2x): NHWC [B,H,W,C] -> ([B,2H,2W,C], output buffer)."""
    B, H, W, Cc = x.shape
    wi = Wide(B, H, W, Cc, x.device, "nan").put(0, x)
    wo = Wide(B, 2 * H, 2 * W, Cc, x.device, "poison").fill(0, Cc, float("nan"))
    check(lib().poco_op_bilinear_up2x(wi.ptr(), wo.ptr(), B, H, W, Cc, current_stream()), "poco_op_bilinear_up2x")
    return wo.get(0, Cc), wo


def maxpool3x3s2(x, *, out_cs=None, out_co=0):
    """3x3 stride-2 pad-1 max pool (poco_op_maxpool3x3s2): NHWC -> (NHWC [B,Ho,Wo,C], output buffer)."""
    B, H, W, Cc = x.shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    out_cs = out_cs or Cc
    wi = Wide(B, H, W, Cc, x.device, "nan").put(0, x)
    wo = Wide(B, Ho, Wo, out_cs, x.device, "poison").fill(out_co, Cc, float("nan"))
    check(lib().poco_op_maxpool3x3s2(wi.ptr(), wo.ptr(out_co), B, H, W, Cc, out_cs, current_stream()), "poco_op_maxpool3x3s2")
    return wo.get(out_co, Cc), wo


def avgpool(x, *, dst_stride=None, dst_off=0):
    """Global average pool (poco_op_avgpool): NHWC [B,H,W,C] -> ([B,C] = columns [dst_off, dst_off + C) of rows of dst_stride
    floats, the destination as a Wide of 1x1 planes)."""
    B, H, W, Cc = x.shape
    dst_stride = dst_stride or Cc
    wi = Wide(B, H, W, Cc, x.device, "nan").put(0, x)
    wo = Wide(B, 1, 1, dst_stride, x.device, "poison").fill(dst_off, Cc, float("nan"))
    check(lib().poco_op_avgpool(wi.ptr(), wo.ptr(dst_off), B, H, W, Cc, dst_stride, current_stream()), "poco_op_avgpool")
    return wo.get(dst_off, Cc).reshape(B, Cc), wo


def stem_conv(img, weight, scale, shift, use_mfma=1):
    """Stem conv + BN + ReLU (poco_op_stem_conv): img [B,3,H,W] NCHW cuda, weight [64,3,ks,ks] -> (NHWC [B,Ho,Wo,64], buffer)."""
    B, _, H, W = img.shape
    ks = weight.shape[-1]
    Ho, Wo = _out_hw(H, W, ks, 2)
    n = img.numel()
    g = -(-3 * W // 64) * 64                                 # guard: NaN around the image, at least one row of all channels (keeps 256-byte alignment)
    flat = torch.full((n + 2 * g,), float("nan"), device=img.device)
    flat[g:g + n] = img.reshape(-1)
    wo = Wide(B, Ho, Wo, 64, img.device, "poison").fill(0, 64, float("nan"))
    check(lib().poco_op_stem_conv(C.c_void_p(flat.data_ptr() + 4 * g), fptr(_f32(weight)), fptr(_f32(scale)), fptr(_f32(shift)),
                                  wo.ptr(), B, H, W, ks, int(use_mfma), current_stream()), "poco_op_stem_conv")
    return wo.get(0, 64), wo


# ---- body-part labels, their crop camera and the segmentation score (include/poco_hip.h; poco_amd/segm.py is the user's side) -----
def _u8(t: torch.Tensor, what: str) -> torch.Tensor:
    if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.uint8):
        raise PocoHipError(f"{what} must be a CUDA uint8 tensor")
    return t.contiguous()


def part_labels(verts: torch.Tensor, cam_t: torch.Tensor, faces: torch.Tensor, face_part: torch.Tensor, focal: float = 5000.0,
                res: int = 224, out: torch.Tensor = None) -> torch.Tensor:
    """poco_op_part_labels: verts [B,V,3], cam_t [B,3] fp32, faces int32 [F,3], face_part uint8 [F] -> labels uint8 [B,res,res]
    (0 = background, part + 1 elsewhere).  `out`: a contiguous uint8 [B,res,res] view to write into."""
    assert verts.is_cuda and verts.dtype == torch.float32 and verts.dim() == 3 and verts.shape[2] == 3
    B, V = int(verts.shape[0]), int(verts.shape[1])
    assert cam_t.shape == (B, 3) and cam_t.dtype == torch.float32 and cam_t.is_cuda
    assert faces.is_cuda and faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3
    F = int(faces.shape[0])
    face_part = _u8(face_part, "face_part")
    assert face_part.shape == (F,)
    if out is None:
        out = torch.empty((B, res, res), device=verts.device, dtype=torch.uint8)
    assert out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous() and out.shape == (B, res, res)
    keys = torch.empty((B, res, res), device=verts.device, dtype=torch.int64)
    check(lib().poco_op_part_labels(fptr(verts.contiguous()), B, V, fptr(cam_t.contiguous()), iptr(faces.contiguous()), F,
                                    C.c_void_p(face_part.data_ptr()), C.c_float(focal), int(res), C.c_void_p(keys.data_ptr()),
                                    C.c_void_p(out.data_ptr()), current_stream()), "poco_op_part_labels")
    return out


VIS_TOTAL, VIS_AREA, VIS_FRONT, VIS_SEEN = 0, 1, 2, 3      # the last axis of part_visibility's counts


def part_visibility_scratch_bytes(B: int, res: int, margin: int) -> int:
    """poco_op_part_visibility_scratch_bytes: the scratch a call needs; 0 for a shape the operator refuses."""
    L = lib()
    L.poco_op_part_visibility_scratch_bytes.restype = C.c_size_t
    return int(L.poco_op_part_visibility_scratch_bytes(int(B), int(res), int(margin)))


def part_visibility(verts: torch.Tensor, cam_t: torch.Tensor, faces: torch.Tensor, face_part: torch.Tensor, focal: float = 5000.0,
                    res: int = 224, margin: int = 112, occ_mask: torch.Tensor = None, out: torch.Tensor = None,
                    scratch: torch.Tensor = None, h_face_part=None) -> torch.Tensor:
    """poco_op_part_visibility: verts [B,V,3], cam_t [B,3] fp32, faces int32 [F,3], face_part uint8 [F] -> counts int32 [B,24,4] =
    (total, area, front, seen) per crop and part: pixels of the part in the window [-margin, res + margin)^2, of those inside the
    crop, of those nearest to the camera, of those where occ_mask (uint8 [B,res,res] or None = nothing occluded) is 0.
    `out`: a contiguous int32 [B,24,4] view to write into; `scratch`: a uint8 tensor of at least part_visibility_scratch_bytes
    bytes (allocated here when None); h_face_part: the host copy of face_part (numpy uint8 [F]) for the argument check.
    Argument errors raise PocoHipError before any GPU work."""
    def need(ok, what):
        if not ok:
            raise PocoHipError(f"part_visibility: {what}")
    need(torch.is_tensor(verts) and verts.is_cuda and verts.dtype == torch.float32 and verts.dim() == 3 and verts.shape[2] == 3,
         "verts must be a CUDA float32 tensor [B,V,3]")
    B, V = int(verts.shape[0]), int(verts.shape[1])
    need(torch.is_tensor(cam_t) and cam_t.is_cuda and cam_t.dtype == torch.float32 and tuple(cam_t.shape) == (B, 3), "cam_t must be a CUDA float32 tensor [B,3]")
    need(torch.is_tensor(faces) and faces.is_cuda and faces.dtype == torch.int32 and faces.dim() == 2 and faces.shape[1] == 3,
         "faces must be a CUDA int32 tensor [F,3]")
    F = int(faces.shape[0])
    face_part = _u8(face_part, "face_part")
    need(tuple(face_part.shape) == (F,), "face_part must be [F]")
    res, margin = int(res), int(margin)
    nbytes = part_visibility_scratch_bytes(B, res, margin)
    need(nbytes > 0, f"needs 1 <= B <= 65535, 1 <= res <= 4096 and 0 <= margin <= res, got B {B}, res {res}, margin {margin}")
    if occ_mask is not None:
        occ_mask = _u8(occ_mask, "occ_mask")
        need(tuple(occ_mask.shape) == (B, res, res), f"occ_mask must be [{B},{res},{res}], got {tuple(occ_mask.shape)}")
    if out is None:
        out = torch.empty((B, 24, 4), device=verts.device, dtype=torch.int32)
    need(out.is_cuda and out.dtype == torch.int32 and out.is_contiguous() and tuple(out.shape) == (B, 24, 4), "out must be a contiguous CUDA int32 [B,24,4]")
    if scratch is None:
        scratch = torch.empty(nbytes, device=verts.device, dtype=torch.uint8)
    need(scratch.is_cuda and scratch.dtype == torch.uint8 and scratch.is_contiguous() and scratch.numel() >= nbytes,
         f"scratch must be a contiguous CUDA uint8 tensor of at least {nbytes} bytes")
    hfp = None
    if h_face_part is not None:
        hfp = np.ascontiguousarray(np.asarray(h_face_part, np.uint8).reshape(-1))
        need(hfp.shape[0] == F, "h_face_part must be [F]")
    check(lib().poco_op_part_visibility(fptr(verts.contiguous()), B, V, fptr(cam_t.contiguous()), iptr(faces.contiguous()), F,
                                        C.c_void_p(face_part.data_ptr()), C.c_void_p(hfp.ctypes.data if hfp is not None else 0),
                                        C.c_float(focal), res, margin, C.c_void_p(occ_mask.data_ptr() if occ_mask is not None else 0),
                                        C.c_void_p(scratch.data_ptr()), C.c_void_p(out.data_ptr()), current_stream()),
          "poco_op_part_visibility")
    return out


def estimate_translation(joints3d: torch.Tensor, joints2d: torch.Tensor, focal: float = 5000.0, res: int = 224) -> torch.Tensor:
    """poco_op_estimate_translation: joints3d [B,J,3], joints2d [B,J,3] = (x, y, confidence) in crop pixels -> cam_t [B,3]."""
    assert joints3d.is_cuda and joints3d.dtype == torch.float32 and joints3d.dim() == 3 and joints3d.shape[2] == 3
    assert joints2d.is_cuda and joints2d.dtype == torch.float32 and joints2d.shape == joints3d.shape
    B, J = int(joints3d.shape[0]), int(joints3d.shape[1])
    out = torch.empty((B, 3), device=joints3d.device, dtype=torch.float32)
    check(lib().poco_op_estimate_translation(fptr(joints3d.contiguous()), fptr(joints2d.contiguous()), B, J, C.c_float(focal), int(res),
                                             fptr(out), current_stream()), "poco_op_estimate_translation")
    return out


def segm_record_words(num_classes: int) -> int:
    return 2 + 3 * int(num_classes)


def segm_score(logits: torch.Tensor, labels: torch.Tensor, out: torch.Tensor = None) -> torch.Tensor:
    """poco_op_segm_score: logits [B,C,h,w] fp32, labels uint8 [B,H,W] -> records int64 [B, 2 + 3C]: word 0 holds the bits of the
    fp64 cross-entropy sum (records[:, 0].view(torch.float64)), word 1 the correct pixels, then per class intersection / predicted /
    ground-truth counts.  `out`: a contiguous int64 [B, 2 + 3C] view to write into."""
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 4
    labels = _u8(labels, "labels")
    B, Cc, h, w = (int(x) for x in logits.shape)
    assert labels.dim() == 3 and labels.shape[0] == B
    H, W = int(labels.shape[1]), int(labels.shape[2])
    words = segm_record_words(Cc)
    if out is None:
        out = torch.empty((B, words), device=logits.device, dtype=torch.int64)
    assert out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and out.shape == (B, words)
    L = lib()
    partials = torch.empty((B, max(int(L.poco_op_segm_score_partials(h, H)), 1)), device=logits.device, dtype=torch.float64)
    check(L.poco_op_segm_score(fptr(logits.contiguous()), B, Cc, h, w, C.c_void_p(labels.data_ptr()), H, W, C.c_void_p(out.data_ptr()),
                               C.c_void_p(partials.data_ptr()), current_stream()), "poco_op_segm_score")
    return out


def segm_argmax(logits: torch.Tensor, H: int, W: int) -> torch.Tensor:
    """poco_op_segm_argmax: logits [B,C,h,w] -> uint8 [B,H,W], the class segm_score calls predicted at every pixel."""
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 4
    B, Cc, h, w = (int(x) for x in logits.shape)
    out = torch.empty((B, int(H), int(W)), device=logits.device, dtype=torch.uint8)
    check(lib().poco_op_segm_argmax(fptr(logits.contiguous()), B, Cc, h, w, int(H), int(W), C.c_void_p(out.data_ptr()), current_stream()),
          "poco_op_segm_argmax")
    return out


# ---- video mode's in-fill of unreliable joint rotations (include/poco_hip.h; poco_amd/infill.py is the user's side) -------------
INFILL_MAX_LIN = 16


def track_infill(pose: torch.Tensor, u: torch.Tensor, frames: torch.Tensor, offsets: torch.Tensor, lin: torch.Tensor, thresh: float,
                 max_gap: int, *, rows: bool = False, out=None):
    """poco_op_track_infill on device tensors: pose [N,24,3,3], u [N,24] fp32, frames int32 [N], offsets int32 [P+1] (0 .. N,
    strictly increasing; a host tensor is taken as it is, a device tensor is read back once for the check), lin [N,L] fp32, L <= 16
    -> (pose', lin', flags uint8 [N,24], touched uint8 [N]); rows=True adds (rows int32 [N], count int32 [1]): the first `count`
    words of rows are the touched rows in ascending order.  out = (pose', lin', flags, touched[, rows, count]): contiguous tensors
    to write into (tests: views into guarded buffers).  Argument errors raise PocoHipError before any GPU work."""
    def need(ok, what):
        if not ok:
            raise PocoHipError(f"track_infill: {what}")
    for name, t, dt in (("pose", pose, torch.float32), ("u", u, torch.float32), ("frames", frames, torch.int32),
                        ("lin", lin, torch.float32)):
        need(torch.is_tensor(t) and t.is_cuda, f"{name} must be a CUDA tensor")
        need(t.dtype == dt, f"{name} must be {dt}, got {t.dtype}")
    need(torch.is_tensor(offsets) and offsets.dtype == torch.int32 and offsets.dim() == 1 and offsets.numel() >= 2,
         "offsets must be an int32 tensor [P+1], P >= 1")
    need(pose.dim() == 4 and tuple(pose.shape[1:]) == (24, 3, 3) and pose.shape[0] >= 1, f"pose must be [N,24,3,3], got {tuple(pose.shape)}")
    N, P = int(pose.shape[0]), int(offsets.numel()) - 1
    need(tuple(u.shape) == (N, 24), f"u must be [{N},24], got {tuple(u.shape)}")
    need(tuple(frames.shape) == (N,), f"frames must be [{N}], got {tuple(frames.shape)}")
    need(lin.dim() == 2 and lin.shape[0] == N, f"lin must be [{N},L], got {tuple(lin.shape)}")
    L = int(lin.shape[1])
    need(L <= INFILL_MAX_LIN, f"L = {L} exceeds {INFILL_MAX_LIN}")
    need(isinstance(max_gap, (int, np.integer)) and max_gap >= 1, f"max_gap must be an integer >= 1, got {max_gap!r}")
    off = offsets.cpu().numpy()
    need(off[0] == 0 and off[-1] == N and bool(np.all(np.diff(off) > 0)), "offsets must start at 0, end at N and increase strictly")
    dev = pose.device
    if out is None:
        out = [torch.empty_like(pose), torch.empty_like(lin), torch.empty((N, 24), device=dev, dtype=torch.uint8),
               torch.empty((N,), device=dev, dtype=torch.uint8)]
        if rows:
            out += [torch.empty((N,), device=dev, dtype=torch.int32), torch.empty((1,), device=dev, dtype=torch.int32)]
    need(len(out) == (6 if rows else 4), "out must hold pose', lin', flags, touched (and rows, count with rows=True)")
    shapes = [((N, 24, 3, 3), torch.float32), ((N, L), torch.float32), ((N, 24), torch.uint8), ((N,), torch.uint8), ((N,), torch.int32),
              ((1,), torch.int32)]
    for t, (shp, dt) in zip(out, shapes):
        need(t.is_cuda and t.is_contiguous() and tuple(t.shape) == shp and t.dtype == dt, f"an output must be a contiguous CUDA {dt} {shp}")
    scratch = torch.empty((24 * N,), device=dev, dtype=torch.int32)
    p = lambda t: C.c_void_p(t.data_ptr())                                    # noqa: E731
    null = C.c_void_p(0)
    check(lib().poco_op_track_infill(p(pose.contiguous()), p(u.contiguous()), p(frames.contiguous()), p(offsets.to(dev).contiguous()), P, N,
                                     p(lin.contiguous()) if L else null, L, C.c_float(thresh), int(max_gap), p(scratch), p(out[0]),
                                     p(out[1]) if L else null, p(out[2]), p(out[3]), p(out[4]) if rows else null,
                                     p(out[5]) if rows else null, current_stream()), "poco_op_track_infill")
    return tuple(out)


# ---- choosing between two regressors by their uncertainty (include/poco_hip.h; poco_amd/select.py is the user's side) -----------
SELECT_MAX_PAYLOADS = 8
SELECT_MODES = {"crop": 0, "joint": 1}


class _SelectPayload(C.Structure):
    _fields_ = [("src0", C.c_void_p), ("src1", C.c_void_p), ("dst", C.c_void_p), ("width", C.c_int64)]


class _SelectPayloads(C.Structure):
    _fields_ = [("count", C.c_int64), ("p", _SelectPayload * SELECT_MAX_PAYLOADS)]


SELECT_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                   _SelectPayloads] + [C.c_void_p] * 7 + [C.c_int, C.c_void_p]


def select_payloads(triples):
    """The by-value descriptor of poco_op_select_regressor from [(src0 pointer, src1 pointer, dst pointer, width), ...]; more than
    SELECT_MAX_PAYLOADS entries keep their count (the entry refuses it) but only the first eight are stored."""
    d = _SelectPayloads()
    d.count = len(triples)
    for k, (a, b, o, w) in enumerate(triples[:SELECT_MAX_PAYLOADS]):
        d.p[k] = _SelectPayload(a, b, o, int(w))
    return d


def select_regressor(pose0: torch.Tensor, var0: torch.Tensor, kind0: int, pose1: torch.Tensor, var1: torch.Tensor, kind1: int,
                     payloads=(), *, kinematic: bool = True, thr: float = 0.40, scale: float = 1.0, mode="crop", rows: bool = False,
                     out=None, max_blocks: int = 0) -> dict:
    """poco_op_select_regressor on device tensors: pose_m [B,24,3,3], var_m [B,24] fp32 (the raw var_pose), kind_m 0 = the mean rule
    (pare) | 1 = the root rule (cliff), payloads = [(src0, src1), ...] of up to 8 pairs of contiguous fp32 tensors with B rows each
    (any trailing shape, the same in a pair), mode "crop" | "joint" (or 0 | 1)
    -> dict(pose, var, choice uint8 [B,24], score [B,2], mixed uint8 [B], payloads = [dst, ...]); rows=True adds rows int32 [B] and
    count int32 [1]: the first `count` words of rows are the mixed rows in ascending order.  out = a dict with the same keys:
    contiguous tensors to write into (tests: views into guarded buffers).  max_blocks > 0 bounds the grid of the first launch (the
    result does not depend on it).  Argument errors raise PocoHipError before any GPU work."""
    def need(ok, what):
        if not ok:
            raise PocoHipError(f"select_regressor: {what}")
    for name, t in (("pose0", pose0), ("var0", var0), ("pose1", pose1), ("var1", var1)):
        need(torch.is_tensor(t) and t.is_cuda, f"{name} must be a CUDA tensor")
        need(t.dtype == torch.float32, f"{name} must be float32, got {t.dtype}")
    need(pose0.dim() == 4 and tuple(pose0.shape[1:]) == (24, 3, 3) and pose0.shape[0] >= 1, f"pose0 must be [B,24,3,3], got {tuple(pose0.shape)}")
    B = int(pose0.shape[0])
    need(tuple(pose1.shape) == (B, 24, 3, 3), f"pose1 must be [{B},24,3,3], got {tuple(pose1.shape)}")
    for name, t in (("var0", var0), ("var1", var1)):
        need(tuple(t.shape) == (B, 24), f"{name} must be [{B},24] (SIGMA_DIM 1), got {tuple(t.shape)}")
    mode = SELECT_MODES.get(mode, mode)
    need(mode in (0, 1), "mode must be 'crop' or 'joint'")
    need(kind0 in (0, 1) and kind1 in (0, 1), "kind0 and kind1 must be 0 (mean rule) or 1 (root rule)")
    need(isinstance(scale, (int, float)) and np.isfinite(scale) and scale > 0, f"scale must be finite and > 0, got {scale!r}")
    payloads = list(payloads)
    need(len(payloads) <= SELECT_MAX_PAYLOADS, f"at most {SELECT_MAX_PAYLOADS} payloads, got {len(payloads)}")
    for k, (a, b) in enumerate(payloads):
        for t in (a, b):
            need(torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float32 and t.is_contiguous(),
                 f"payload {k} must be a pair of contiguous float32 CUDA tensors")
        need(a.shape == b.shape and a.dim() >= 1 and a.shape[0] == B and a.numel() >= B, f"payload {k} must be two [{B}, ...] tensors of one shape")
    dev = pose0.device
    if out is None:
        out = {"pose": torch.empty_like(pose0), "var": torch.empty_like(var0), "choice": torch.empty((B, 24), device=dev, dtype=torch.uint8),
               "score": torch.empty((B, 2), device=dev, dtype=torch.float32), "mixed": torch.empty((B,), device=dev, dtype=torch.uint8),
               "payloads": [torch.empty_like(a) for a, _ in payloads]}
        if rows:
            out["rows"] = torch.empty((B,), device=dev, dtype=torch.int32)
            out["count"] = torch.empty((1,), device=dev, dtype=torch.int32)
    shapes = {"pose": ((B, 24, 3, 3), torch.float32), "var": ((B, 24), torch.float32), "choice": ((B, 24), torch.uint8),
              "score": ((B, 2), torch.float32), "mixed": ((B,), torch.uint8)}
    if rows:
        shapes.update(rows=((B,), torch.int32), count=((1,), torch.int32))
    for key, (shp, dt) in shapes.items():
        t = out.get(key)
        need(torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shp and t.dtype == dt,
             f"out[{key!r}] must be a contiguous CUDA {dt} {shp}")
    need(len(out.get("payloads", [])) == len(payloads), "out['payloads'] must hold one destination per payload")
    for k, ((a, _), o) in enumerate(zip(payloads, out["payloads"])):
        need(torch.is_tensor(o) and o.is_cuda and o.is_contiguous() and o.shape == a.shape and o.dtype == torch.float32,
             f"out['payloads'][{k}] must be a contiguous float32 CUDA tensor of the payload's shape")
    p = lambda t: t.data_ptr()                                                # noqa: E731
    pose0, var0, pose1, var1 = pose0.contiguous(), var0.contiguous(), pose1.contiguous(), var1.contiguous()
    desc = select_payloads([(p(a), p(b), p(o), a.numel() // B) for (a, b), o in zip(payloads, out["payloads"])])
    fn = lib().poco_op_select_regressor
    fn.argtypes = SELECT_ARGTYPES
    check(fn(p(pose0), p(var0), int(kind0), p(pose1), p(var1), int(kind1), B, int(bool(kinematic)), float(thr), float(scale), int(mode),
             desc, p(out["pose"]), p(out["var"]), p(out["choice"]), p(out["score"]), p(out["mixed"]),
             p(out["rows"]) if rows else None, p(out["count"]) if rows else None, int(max_blocks), current_stream()),
          "poco_op_select_regressor")
    return out


# ---- test-time augmentation: fusing K views of a crop (include/poco_hip.h; poco_amd/tta.py is the user's side) ---------------------
TTA_MAX_VIEWS = 8
TTA_WEIGHTS = {"uniform": 0, "uncert": 1}


class _TtaView(C.Structure):
    _fields_ = [("flip", C.c_int32), ("pad_", C.c_int32), ("c", C.c_double), ("s", C.c_double)]


class _TtaViews(C.Structure):
    _fields_ = [("count", C.c_int64), ("v", _TtaView * TTA_MAX_VIEWS)]


TTA_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, _TtaViews, C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p]


def tta_view_cs(rot: float):
    """(cos, sin) of +rot degrees in float64, exact at the quarter turns: rot = 0 gives (1.0, 0.0).  tests/tta_np.view_cs restates this
    on purpose instead of importing it; what pins both is the comparison with cos / sin of pi / 12 in tests/test_tta_cpu.py."""
    import math
    q, r = divmod(float(rot), 90.0)
    if r == 0.0:
        return ((1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0))[int(q) % 4]
    a = math.radians(float(rot))
    return math.cos(a), math.sin(a)


def tta_views(views):
    """The by-value view table of poco_op_tta_fuse from [(flip, c, s), ...]; more than TTA_MAX_VIEWS entries keep their count (the
    entry refuses it) but only the first eight are stored."""
    d = _TtaViews()
    d.count = len(views)
    for k, (f, c, s) in enumerate(views[:TTA_MAX_VIEWS]):
        d.v[k] = _TtaView(int(f), 0, float(c), float(s))
    return d


def tta_fuse(pose: torch.Tensor, var: torch.Tensor, betas: torch.Tensor, views, weight="uncert", *, out=None, max_blocks: int = 0) -> dict:
    """poco_op_tta_fuse on device tensors: K views of B crops, view-major (row k * B + b): pose [K*B,24,3,3], var [K*B,24] (the raw
    var_pose), betas [K*B,10], fp32 and contiguous; views = [(flip, rot degrees), ...] with view 0 = (0, 0); weight "uncert" |
    "uniform" (or 1 | 0) -> dict(pose [B,24,3,3], var [B,24], spread [B,24], betas [B,10]).  out = a dict with the same keys:
    contiguous tensors to write into (tests: views into guarded buffers).  max_blocks > 0 bounds the grid (the result does not
    depend on it).  Argument errors raise PocoHipError before any GPU work."""
    def need(ok, what):
        if not ok:
            raise PocoHipError(f"tta_fuse: {what}")
    for name, t in (("pose", pose), ("var", var), ("betas", betas)):
        need(torch.is_tensor(t) and t.is_cuda, f"{name} must be a CUDA tensor")
        need(t.dtype == torch.float32 and t.is_contiguous(), f"{name} must be contiguous float32, got {t.dtype}")
    views = list(views)
    K = len(views)
    need(2 <= K <= TTA_MAX_VIEWS, f"2 to {TTA_MAX_VIEWS} views are needed, got {K}")
    need(all(len(v) == 2 and v[0] in (0, 1, False, True) and np.isfinite(float(v[1])) for v in views), "a view is (flip 0 | 1, rot in finite degrees)")
    need(int(views[0][0]) == 0 and float(views[0][1]) == 0.0, "view 0 must be the identity (flip 0, rot 0)")
    need(pose.dim() == 4 and tuple(pose.shape[1:]) == (24, 3, 3) and pose.shape[0] >= K and pose.shape[0] % K == 0,
         f"pose must be [K*B,24,3,3] with K = {K}, got {tuple(pose.shape)}")
    B = int(pose.shape[0]) // K
    need(tuple(var.shape) == (K * B, 24), f"var must be [{K * B},24] (SIGMA_DIM 1), got {tuple(var.shape)}")
    need(tuple(betas.shape) == (K * B, 10), f"betas must be [{K * B},10], got {tuple(betas.shape)}")
    weight = TTA_WEIGHTS.get(weight, weight)
    need(weight in (0, 1), "weight must be 'uncert' or 'uniform'")
    dev = pose.device
    shapes = {"pose": (B, 24, 3, 3), "var": (B, 24), "spread": (B, 24), "betas": (B, 10)}
    if out is None:
        out = {k: torch.empty(s, device=dev, dtype=torch.float32) for k, s in shapes.items()}
    for key, shp in shapes.items():
        t = out.get(key)
        need(torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shp and t.dtype == torch.float32,
             f"out[{key!r}] must be a contiguous CUDA float32 {shp}")
    p = lambda t: t.data_ptr()                                                # noqa: E731
    fn = lib().poco_op_tta_fuse
    fn.argtypes = TTA_ARGTYPES
    with torch.cuda.device(dev):
        check(fn(p(pose), p(var), p(betas), B, tta_views([(int(f), *tta_view_cs(r)) for f, r in views]), int(weight), p(out["pose"]),
                 p(out["var"]), p(out["spread"]), p(out["betas"]), int(max_blocks), current_stream()), "poco_op_tta_fuse")
    return out


# ---- rank-based uncertainty metrics: sort, midranks, cut sums (include/poco_hip.h; poco_amd/ranking.py is the user's side) ----------
RANK_TILE = 2048                  # POCO_RANK_TILE: rows per tile of the sort (tests sit on its edges)
RANK_MAX_N, RANK_MAX_PLANES, RANK_MAX_CUTS = 1 << 24, 4, 1024
RANK_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_void_p, C.c_size_t] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p]
PEARSON64_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p]


def rank_curve_scratch_bytes(n: int, E: int) -> int:
    """poco_op_rank_curve_scratch_bytes: the bytes of scratch poco_op_rank_curve needs for n rows and E planes (0: out of range)."""
    fn = lib().poco_op_rank_curve_scratch_bytes
    fn.argtypes, fn.restype = [C.c_int64, C.c_int], C.c_size_t
    return int(fn(int(n), int(E)))


def rank_curve(key: torch.Tensor, vals=None, K: int = 20, max_blocks: int = 0, *, out=None, scratch=None) -> dict:
    """poco_op_rank_curve on device tensors: key [n] fp32 and vals [E,n] fp32 (None or E = 0: no planes) -> dict(order int32 [n] =
    the stable argsort of the canonical keys, rank float64 [n] = 1-based midranks, cuts float64 [E+1,K+1] = sums of the key (plane 0)
    and of each value plane over the first floor(k n / K) sorted rows, cut_keys fp32 [K+1]).  out = a dict with the same keys:
    contiguous tensors to write into; scratch = a uint8 CUDA tensor of at least rank_curve_scratch_bytes(n, E) bytes (default: one
    is allocated here, before the call).  max_blocks > 0 bounds the grid (the result does not depend on it).  Argument errors raise
    PocoHipError before any GPU work."""
    def need(ok, what):
        if not ok:
            raise PocoHipError(f"rank_curve: {what}")
    need(torch.is_tensor(key) and key.is_cuda and key.dtype == torch.float32 and key.is_contiguous() and key.dim() == 1,
         "key must be a contiguous float32 CUDA vector")
    n = int(key.shape[0])
    E = 0 if vals is None else int(vals.shape[0]) if torch.is_tensor(vals) and vals.dim() == 2 else -1
    need(E >= 0, "vals must be None or [E,n]")
    if E > 0:
        need(vals.is_cuda and vals.dtype == torch.float32 and vals.is_contiguous() and int(vals.shape[1]) == n,
             f"vals must be a contiguous float32 CUDA [E,{n}], got {tuple(vals.shape)} {vals.dtype}")
    need(1 <= n <= RANK_MAX_N, f"n must be in 1..2^24, got {n}")
    need(E <= RANK_MAX_PLANES, f"at most {RANK_MAX_PLANES} value planes, got {E}")
    need(isinstance(K, (int, np.integer)) and 1 <= K <= RANK_MAX_CUTS, f"K must be in 1..{RANK_MAX_CUTS}, got {K}")
    dev = key.device
    shapes = {"order": ((n,), torch.int32), "rank": ((n,), torch.float64), "cuts": ((E + 1, K + 1), torch.float64),
              "cut_keys": ((K + 1,), torch.float32)}
    if out is None:
        out = {k: torch.empty(s, device=dev, dtype=dt) for k, (s, dt) in shapes.items()}
    for k, (shp, dt) in shapes.items():
        t = out.get(k)
        need(torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shp and t.dtype == dt,
             f"out[{k!r}] must be a contiguous CUDA {dt} {shp}")
    nbytes = rank_curve_scratch_bytes(n, E)
    if scratch is None:
        scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    need(torch.is_tensor(scratch) and scratch.is_cuda and scratch.dtype == torch.uint8 and scratch.is_contiguous(),
         "scratch must be a contiguous uint8 CUDA tensor")
    p = lambda t: t.data_ptr()                                                # noqa: E731
    fn = lib().poco_op_rank_curve
    fn.argtypes = RANK_ARGTYPES
    with torch.cuda.device(dev):
        check(fn(p(key), p(vals) if E > 0 else None, n, E, int(K), p(scratch), int(scratch.numel()), p(out["order"]), p(out["rank"]),
                 p(out["cuts"]), p(out["cut_keys"]), int(max_blocks), current_stream()), "poco_op_rank_curve")
    return out


def pearson64(x: torch.Tensor, y: torch.Tensor, max_blocks: int = 0, *, out=None) -> torch.Tensor:
    """poco_op_pearson64: Pearson's r of two float64 CUDA vectors of one length, as a float64 CUDA tensor [1] (clipped to [-1, 1];
    NaN where either side is constant).  Applied to two `rank` arrays of rank_curve it is Spearman's rho.  Nothing is read back."""
    for name, t in (("x", x), ("y", y)):
        if not (torch.is_tensor(t) and t.is_cuda and t.dtype == torch.float64 and t.is_contiguous() and t.dim() == 1):
            raise PocoHipError(f"pearson64: {name} must be a contiguous float64 CUDA vector")
    if x.shape != y.shape or not 1 <= int(x.shape[0]) <= RANK_MAX_N:
        raise PocoHipError(f"pearson64: x and y must have one length in 1..2^24, got {tuple(x.shape)} and {tuple(y.shape)}")
    if out is None:
        out = torch.empty(1, device=x.device, dtype=torch.float64)
    fn = lib().poco_op_pearson64
    fn.argtypes = PEARSON64_ARGTYPES
    with torch.cuda.device(x.device):
        check(fn(x.data_ptr(), y.data_ptr(), int(x.shape[0]), out.data_ptr(), int(max_blocks), current_stream()), "poco_op_pearson64")
    return out


# ---- calibration: isotonic regression over ragged segments, fitted maps evaluated (include/poco_hip.h; poco_amd/calibrate.py) -------
ISO_TILE = 2048                   # POCO_ISO_TILE: positions per tile of the fit (tests sit on its edges)
ISO_MAX_N, ISO_MAX_SEGS = 1 << 26, 4096
ISOTONIC_ARGTYPES = ([C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int, C.c_void_p, C.c_size_t] +
                     [C.c_void_p] * 4 + [C.c_int, C.c_void_p])
CALIB_APPLY_ARGTYPES = [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_void_p, C.c_int,
                        C.c_void_p]


def isotonic_scratch_bytes(N: int, S: int) -> int:
    """poco_op_isotonic_scratch_bytes: the bytes of scratch poco_op_isotonic needs for N positions in S segments (0: out of range)."""
    fn = lib().poco_op_isotonic_scratch_bytes
    fn.argtypes, fn.restype = [C.c_int64, C.c_int], C.c_size_t
    return int(fn(int(N), int(S)))


def check_offsets(seg_offsets, N: int, what: str) -> np.ndarray:
    """A table of offsets as a host int64 array (a device tensor is read back once), refused unless it runs from 0 to N without a
    step down."""
    off = seg_offsets.detach().cpu().numpy() if torch.is_tensor(seg_offsets) else np.asarray(seg_offsets)
    if off.ndim != 1 or len(off) < 2 or not np.issubdtype(off.dtype, np.integer):
        raise PocoHipError(f"{what} must be an integer vector of at least two entries")
    off = off.astype(np.int64)
    if off[0] != 0 or off[-1] != N or np.any(np.diff(off) < 0):
        raise PocoHipError(f"{what} must be non-decreasing from 0 to {N}, got {off[:4].tolist()} .. {off[-2:].tolist()}")
    return off


def isotonic(key: torch.Tensor, y: torch.Tensor, order: torch.Tensor, seg_offsets, max_blocks: int = 0, *, out=None, scratch=None) -> dict:
    """poco_op_isotonic on device tensors: key, y fp32 [M], order int32 [N] (entries in [0, M): segment s's rows in ascending order of
    canonical key at positions [seg_offsets[s], seg_offsets[s+1])), seg_offsets int32 [S+1] (a device tensor is read back once for
    the check, a host array is checked and uploaded) -> dict(block int32 [N], fit float64 [N], seg_blocks int32 [S+1], knots float64
    [N,4] of which the first seg_blocks[S] rows are written).  out = a dict with the same keys to write into; scratch = a uint8 CUDA
    tensor of at least isotonic_scratch_bytes(N, S) bytes.  Argument errors raise PocoHipError before any GPU work.  Rows with a
    non-finite key or y must be taken out by the CALLER (calibrate.finite_rows drops and counts them): the kernels stay inside their
    buffers on such rows, but the values are unspecified."""
    def need(ok, what):
        if not ok:
            raise PocoHipError(f"isotonic: {what}")
    for name, t, dt in (("key", key, torch.float32), ("y", y, torch.float32), ("order", order, torch.int32)):
        need(torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.is_contiguous() and t.dim() == 1,
             f"{name} must be a contiguous {dt} CUDA vector")
    M, N = int(key.shape[0]), int(order.shape[0])
    need(int(y.shape[0]) == M, f"key and y must have one length, got {M} and {int(y.shape[0])}")
    need(N <= ISO_MAX_N and M <= ISO_MAX_N and (N == 0 or M >= 1), f"N and M must be at most 2^26 and M >= 1 when N >= 1, got N {N}, M {M}")
    off = check_offsets(seg_offsets, N, "isotonic: seg_offsets")
    S = len(off) - 1
    need(1 <= S <= ISO_MAX_SEGS, f"S must be in 1..{ISO_MAX_SEGS}, got {S}")
    dev = key.device
    if torch.is_tensor(seg_offsets) and seg_offsets.is_cuda and seg_offsets.dtype == torch.int32 and seg_offsets.is_contiguous():
        d_off = seg_offsets
    else:
        d_off = torch.from_numpy(off.astype(np.int32)).to(dev)
    shapes = {"block": ((N,), torch.int32), "fit": ((N,), torch.float64), "seg_blocks": ((S + 1,), torch.int32),
              "knots": ((N, 4), torch.float64)}
    if out is None:
        out = {k: torch.empty(s, device=dev, dtype=dt) for k, (s, dt) in shapes.items()}
    for k, (shp, dt) in shapes.items():
        t = out.get(k)
        need(torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shp and t.dtype == dt,
             f"out[{k!r}] must be a contiguous CUDA {dt} {shp}")
    nbytes = isotonic_scratch_bytes(N, S)
    if scratch is None:
        scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    need(torch.is_tensor(scratch) and scratch.is_cuda and scratch.dtype == torch.uint8 and scratch.is_contiguous(),
         "scratch must be a contiguous uint8 CUDA tensor")
    p = lambda t: t.data_ptr() if t.numel() else None                          # noqa: E731
    fn = lib().poco_op_isotonic
    fn.argtypes = ISOTONIC_ARGTYPES
    with torch.cuda.device(dev):
        check(fn(p(key), p(y), M, p(order), N, d_off.data_ptr(), S, scratch.data_ptr(), int(scratch.numel()), p(out["block"]),
                 p(out["fit"]), out["seg_blocks"].data_ptr(), p(out["knots"]), int(max_blocks), current_stream()), "poco_op_isotonic")
    return out


def calib_apply(x: torch.Tensor, map_ids: torch.Tensor, map_offsets: torch.Tensor, knots: torch.Tensor, max_blocks: int = 0, *,
                out=None) -> torch.Tensor:
    """poco_op_calib_apply on device tensors: x fp32 [R,S], map_ids int32 [S], map_offsets int32 [P+1], knots float64 [B,4] as
    poco_op_isotonic writes them -> fp32 [R,S], out[r][c] = the map map_ids[c] at x[r][c].  Argument errors raise PocoHipError
    before any GPU work."""
    def need(ok, what):
        if not ok:
            raise PocoHipError(f"calib_apply: {what}")
    for name, t, dt, nd in (("x", x, torch.float32, 2), ("map_ids", map_ids, torch.int32, 1), ("map_offsets", map_offsets, torch.int32, 1),
                            ("knots", knots, torch.float64, 2)):
        need(torch.is_tensor(t) and t.is_cuda and t.dtype == dt and t.is_contiguous() and t.dim() == nd,
             f"{name} must be a contiguous {dt} CUDA tensor of {nd} dimension(s)")
    R, S = (int(v) for v in x.shape)
    P, B = int(map_offsets.shape[0]) - 1, int(knots.shape[0])
    need(int(map_ids.shape[0]) == S, f"map_ids must have one entry per column, got {int(map_ids.shape[0])} for {S}")
    need(int(knots.shape[1]) == 4, "knots must be [B,4]")
    need(R >= 1 and 1 <= S <= ISO_MAX_SEGS and 1 <= P <= ISO_MAX_SEGS, f"needs R >= 1, S and P in 1..{ISO_MAX_SEGS}, got {R}, {S}, {P}")
    if out is None:
        out = torch.empty((R, S), device=x.device, dtype=torch.float32)
    need(torch.is_tensor(out) and out.is_cuda and out.is_contiguous() and tuple(out.shape) == (R, S) and out.dtype == torch.float32,
         f"out must be a contiguous CUDA float32 {(R, S)}")
    fn = lib().poco_op_calib_apply
    fn.argtypes = CALIB_APPLY_ARGTYPES
    with torch.cuda.device(x.device):
        check(fn(x.data_ptr(), R, S, map_ids.data_ptr(), map_offsets.data_ptr(), P, knots.data_ptr() if B else None, B, out.data_ptr(),
                 int(max_blocks), current_stream()), "poco_op_calib_apply")
    return out


# ---- the cluster bootstrap: unit moments and resamples (include/poco_hip.h; poco_amd/bootstrap.py is the user's side) ---------------
BOOT_MAX_N, BOOT_MAX_PLANES, BOOT_MAX_PAIRS, BOOT_MAX_B = 1 << 24, 16, 16, 65536
BOOTSTRAP_ARGTYPES = ([C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_uint64, C.c_void_p,
                       C.c_size_t] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p])


def bootstrap_scratch_bytes(n: int, E: int, P: int, U: int) -> int:
    """poco_op_bootstrap_scratch_bytes: the bytes of scratch poco_op_bootstrap needs (0: an argument out of range)."""
    fn = lib().poco_op_bootstrap_scratch_bytes
    fn.argtypes, fn.restype = [C.c_int64, C.c_int, C.c_int, C.c_int64], C.c_size_t
    return int(fn(int(n), int(E), int(P), int(U)))


def bootstrap(planes: torch.Tensor, pairs=(), unit_offsets=None, B: int = 0, seed: int = 0, max_blocks: int = 0, *, out=None,
              scratch=None, draw_counts: bool = False) -> dict:
    """poco_op_bootstrap on device tensors: planes fp32 [E,n], pairs = up to 16 (a, b) plane indices (host), unit_offsets int32 [U+1]
    (None: every row is its own unit; a device tensor is read back once for the check, a host array is checked and uploaded), B
    replicates, seed in 0..2^64-1 -> dict(center float64 [E], unit_mom float64 [U,M], out float64 [B+1,M], M = 1 + E + P, and with
    draw_counts=True or out["draw_counts"] given: draw_counts int32 [B,U], the bits of the header's uint32).  out = a dict with the
    same keys to write into; scratch = a uint8 CUDA tensor of at least bootstrap_scratch_bytes(n, E, P, U) bytes.  max_blocks > 0
    bounds the grid (the result does not depend on it).  Argument errors raise PocoHipError before any GPU work."""
    def need(ok, what):
        if not ok:
            raise PocoHipError(f"bootstrap: {what}")
    need(torch.is_tensor(planes) and planes.is_cuda and planes.dtype == torch.float32 and planes.is_contiguous() and planes.dim() == 2,
         "planes must be a contiguous float32 CUDA [E,n]")
    E, n = (int(v) for v in planes.shape)
    need(1 <= E <= BOOT_MAX_PLANES and 1 <= n <= BOOT_MAX_N, f"E must be in 1..{BOOT_MAX_PLANES} and n in 1..2^24, got E {E}, n {n}")
    try:
        pr = np.ascontiguousarray(np.asarray(list(pairs), np.int64).reshape(-1, 2))
    except (TypeError, ValueError):
        pr = None
    need(pr is not None and len(pr) <= BOOT_MAX_PAIRS, f"pairs must be at most {BOOT_MAX_PAIRS} (a, b) plane indices")
    P = len(pr)
    need(P == 0 or (pr.min() >= 0 and pr.max() < E), f"a pair names a plane outside 0..{E - 1}")
    pr = np.ascontiguousarray(pr.astype(np.int32))
    need(isinstance(B, (int, np.integer)) and 0 <= B <= BOOT_MAX_B, f"B must be in 0..{BOOT_MAX_B}, got {B}")
    need(isinstance(seed, (int, np.integer)) and 0 <= int(seed) < 1 << 64, f"seed must be in 0..2^64-1, got {seed}")
    dev = planes.device
    d_off = None
    U = n
    if unit_offsets is not None:
        off = check_offsets(unit_offsets, n, "bootstrap: unit_offsets")
        U = len(off) - 1
        need(U <= n, f"at most n = {n} units, got {U}")
        if torch.is_tensor(unit_offsets) and unit_offsets.is_cuda and unit_offsets.dtype == torch.int32 and unit_offsets.is_contiguous():
            d_off = unit_offsets
        else:
            d_off = torch.from_numpy(off.astype(np.int32)).to(dev)
    M = 1 + E + P
    shapes = {"center": ((E,), torch.float64), "unit_mom": ((U, M), torch.float64), "out": ((int(B) + 1, M), torch.float64)}
    if draw_counts or (out is not None and out.get("draw_counts") is not None):
        shapes["draw_counts"] = ((int(B), U), torch.int32)
    if out is None:
        out = {k: torch.empty(s, device=dev, dtype=dt) for k, (s, dt) in shapes.items()}
    for k, (shp, dt) in shapes.items():
        t = out.get(k)
        need(torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shp and t.dtype == dt,
             f"out[{k!r}] must be a contiguous CUDA {dt} {shp}")
    nbytes = bootstrap_scratch_bytes(n, E, P, U)
    if scratch is None:
        scratch = torch.empty(nbytes, device=dev, dtype=torch.uint8)
    need(torch.is_tensor(scratch) and scratch.is_cuda and scratch.dtype == torch.uint8 and scratch.is_contiguous(),
         "scratch must be a contiguous uint8 CUDA tensor")
    counts = out.get("draw_counts") if "draw_counts" in shapes else None
    fn = lib().poco_op_bootstrap
    fn.argtypes = BOOTSTRAP_ARGTYPES
    with torch.cuda.device(dev):
        check(fn(planes.data_ptr(), n, E, pr.ctypes.data if P else None, P, None if d_off is None else d_off.data_ptr(), U, int(B),
                 int(seed), scratch.data_ptr(), int(scratch.numel()), out["center"].data_ptr(), out["unit_mom"].data_ptr(),
                 out["out"].data_ptr(), counts.data_ptr() if counts is not None and counts.numel() else None, int(max_blocks),
                 current_stream()), "poco_op_bootstrap")
    return out


# ---- video mode's uncertainty-weighted smoother (include/poco_hip.h; poco_amd/usmooth.py is the user's side) --------------------
SMOOTH_MAX_LIN = 16
SMOOTH_MAX_LAMBDA = 1e4


def smooth_scratch_doubles(N: int, L: int) -> int:
    """POCO_SMOOTH_SCRATCH_DOUBLES of include/poco_hip.h."""
    return int(N) * (266 + int(L))


def track_smooth(pose: torch.Tensor, u: torch.Tensor, frames: torch.Tensor, offsets: torch.Tensor, lin: torch.Tensor, lam: float,
                 u_ref: float, max_gap: int, *, out=None, max_blocks: int = 0):
    """poco_op_track_smooth on device tensors: pose [N,24,3,3], u [N,24] fp32, frames int32 [N], offsets int32 [P+1] (0 .. N,
    strictly increasing; a host tensor is taken as it is, a device tensor is read back once for the check), lin [N,L] fp32, L <= 16
    -> (pose', lin', shift [N,24] in degrees).  out = (pose', lin', shift): contiguous tensors to write into (tests: poisoned
    buffers); max_blocks > 0 caps the grid.  Argument errors raise PocoHipError before any GPU work."""
    def need(ok, what):
        if not ok:
            raise PocoHipError(f"track_smooth: {what}")
    for name, t, dt in (("pose", pose, torch.float32), ("u", u, torch.float32), ("frames", frames, torch.int32),
                        ("lin", lin, torch.float32)):
        need(torch.is_tensor(t) and t.is_cuda, f"{name} must be a CUDA tensor")
        need(t.dtype == dt, f"{name} must be {dt}, got {t.dtype}")
    need(torch.is_tensor(offsets) and offsets.dtype == torch.int32 and offsets.dim() == 1 and offsets.numel() >= 2,
         "offsets must be an int32 tensor [P+1], P >= 1")
    need(pose.dim() == 4 and tuple(pose.shape[1:]) == (24, 3, 3) and pose.shape[0] >= 1, f"pose must be [N,24,3,3], got {tuple(pose.shape)}")
    N, P = int(pose.shape[0]), int(offsets.numel()) - 1
    need(tuple(u.shape) == (N, 24), f"u must be [{N},24], got {tuple(u.shape)}")
    need(tuple(frames.shape) == (N,), f"frames must be [{N}], got {tuple(frames.shape)}")
    need(lin.dim() == 2 and lin.shape[0] == N, f"lin must be [{N},L], got {tuple(lin.shape)}")
    L = int(lin.shape[1])
    need(L <= SMOOTH_MAX_LIN, f"L = {L} exceeds {SMOOTH_MAX_LIN}")
    need(isinstance(max_gap, (int, np.integer)) and max_gap >= 1, f"max_gap must be an integer >= 1, got {max_gap!r}")
    lam, u_ref = float(lam), float(u_ref)
    need(0.0 < lam <= SMOOTH_MAX_LAMBDA, f"lambda must be in (0, {SMOOTH_MAX_LAMBDA:g}], got {lam!r}")
    need(np.isfinite(u_ref) and u_ref > 0.0, f"u_ref must be finite and > 0, got {u_ref!r}")
    off = offsets.cpu().numpy()
    need(off[0] == 0 and off[-1] == N and bool(np.all(np.diff(off) > 0)), "offsets must start at 0, end at N and increase strictly")
    dev = pose.device
    if out is None:
        out = [torch.empty_like(pose), torch.empty_like(lin), torch.empty((N, 24), device=dev, dtype=torch.float32)]
    need(len(out) == 3, "out must hold pose', lin' and shift")
    for t, shp in zip(out, ((N, 24, 3, 3), (N, L), (N, 24))):
        need(t.is_cuda and t.is_contiguous() and tuple(t.shape) == shp and t.dtype == torch.float32,
             f"an output must be a contiguous CUDA float32 {shp}")
    scratch = torch.empty((smooth_scratch_doubles(N, L),), device=dev, dtype=torch.float64)
    p = lambda t: C.c_void_p(t.data_ptr())                                    # noqa: E731
    null = C.c_void_p(0)
    check(lib().poco_op_track_smooth(p(pose.contiguous()), p(u.contiguous()), p(frames.contiguous()), p(offsets.to(dev).contiguous()), P, N,
                                     p(lin.contiguous()) if L else null, L, C.c_double(lam), C.c_double(u_ref), int(max_gap), p(scratch),
                                     p(out[0]), p(out[1]) if L else null, p(out[2]), int(max_blocks), current_stream()),
          "poco_op_track_smooth")
    return tuple(out)


# ---- the keypoint refit (include/poco_hip.h; poco_amd/refit.py is the user's side) -------------------------------------------------
REFIT_MAX_KP = 32                 # POCO_REFIT_MAX_KP
REFIT_MAX_ITERS = 32              # POCO_REFIT_MAX_ITERS


def kp_refit(pose: torch.Tensor, u: torch.Tensor, jrest: torch.Tensor, kp: torch.Tensor, cam: torch.Tensor, norm: torch.Tensor, kp_joint,
             parents, lam: float, u_ref: float = 0.3, rho: float = 0.1, cam_prior: float = 1.0, conf_thresh: float = 0.3, min_kp: int = 4,
             iters: int = 10, *, out=None, max_blocks: int = 0) -> dict:
    """poco_op_kp_refit on device tensors: pose [N,24,3,3], u [N,24], jrest [N,24,3], kp [N,K,3], cam [N,5] = (a, tx, ty, px, py),
    norm [N], all fp32; kp_joint [K] and parents [24] host integers -> dict(pose [N,24,3,3], cam [N,3], shift [N,24] in degrees, cost
    [N,2], info int32 [N,2] = (accepted steps, flag)).  out = the same dict of contiguous tensors to write into (tests: poisoned
    buffers); max_blocks > 0 caps the grid.  Argument errors raise PocoHipError before any GPU work."""
    def need(ok, what):
        if not ok:
            raise PocoHipError(f"kp_refit: {what}")
    for name, t in (("pose", pose), ("u", u), ("jrest", jrest), ("kp", kp), ("cam", cam), ("norm", norm)):
        need(torch.is_tensor(t) and t.is_cuda, f"{name} must be a CUDA tensor")
        need(t.dtype == torch.float32, f"{name} must be float32, got {t.dtype}")
    need(pose.dim() == 4 and tuple(pose.shape[1:]) == (24, 3, 3) and pose.shape[0] >= 1, f"pose must be [N,24,3,3], got {tuple(pose.shape)}")
    N = int(pose.shape[0])
    need(kp.dim() == 3 and kp.shape[0] == N and kp.shape[2] == 3, f"kp must be [{N},K,3], got {tuple(kp.shape)}")
    K = int(kp.shape[1])
    need(1 <= K <= REFIT_MAX_KP, f"K = {K} is outside 1..{REFIT_MAX_KP}")
    for name, t, shp in (("u", u, (N, 24)), ("jrest", jrest, (N, 24, 3)), ("cam", cam, (N, 5)), ("norm", norm, (N,))):
        need(tuple(t.shape) == shp, f"{name} must be {list(shp)}, got {tuple(t.shape)}")
    kpj = np.ascontiguousarray(np.asarray(kp_joint).reshape(-1), np.int32)
    par = np.ascontiguousarray(np.asarray(parents).reshape(-1).astype(np.int64).astype(np.int32))
    need(kpj.shape == (K,) and bool(((kpj >= -1) & (kpj <= 23)).all()), f"kp_joint must hold {K} joints in -1..23")
    need(par.shape == (24,) and par[0] < 0 and bool(((par[1:] >= 0) & (par[1:] < np.arange(1, 24))).all()),
         "parents must be a tree of 24 joints rooted at joint 0 with parent < child")
    lam, u_ref, rho, cam_prior, conf_thresh = float(lam), float(u_ref), float(rho), float(cam_prior), float(conf_thresh)
    need(np.isfinite(lam) and lam > 0.0, f"lambda must be finite and > 0, got {lam!r}")
    need(np.isfinite(u_ref) and u_ref > 0.0, f"u_ref must be finite and > 0, got {u_ref!r}")
    need(np.isfinite(rho), f"rho must be finite, got {rho!r}")
    need(np.isfinite(cam_prior) and cam_prior > 0.0, f"cam_prior must be finite and > 0, got {cam_prior!r}")
    need(np.isfinite(conf_thresh), f"conf_thresh must be finite, got {conf_thresh!r}")
    need(isinstance(min_kp, (int, np.integer)) and min_kp >= 2, f"min_kp must be an integer >= 2, got {min_kp!r}")
    need(isinstance(iters, (int, np.integer)) and 1 <= iters <= REFIT_MAX_ITERS, f"iters must be an integer in 1..{REFIT_MAX_ITERS}, got {iters!r}")
    need(isinstance(max_blocks, (int, np.integer)) and max_blocks >= 0, f"max_blocks must be an integer >= 0, got {max_blocks!r}")
    dev = pose.device
    shapes = {"pose": ((N, 24, 3, 3), torch.float32), "cam": ((N, 3), torch.float32), "shift": ((N, 24), torch.float32),
              "cost": ((N, 2), torch.float32), "info": ((N, 2), torch.int32)}
    if out is None:
        out = {k: torch.empty(s, device=dev, dtype=dt) for k, (s, dt) in shapes.items()}
    for k, (shp, dt) in shapes.items():
        t = out.get(k)
        need(torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shp and t.dtype == dt,
             f"out[{k!r}] must be a contiguous CUDA {dt} {shp}")
    p = lambda t: C.c_void_p(t.data_ptr())                                    # noqa: E731
    ins = [t.contiguous() for t in (pose, u, jrest, kp, cam, norm)]
    with torch.cuda.device(dev):
        check(lib().poco_op_kp_refit(*[p(t) for t in ins], N, K, C.c_void_p(kpj.ctypes.data), C.c_void_p(par.ctypes.data), C.c_double(lam),
                                     C.c_double(u_ref), C.c_double(rho), C.c_double(cam_prior), C.c_double(conf_thresh), int(min_kp),
                                     int(iters), p(out["pose"]), p(out["cam"]), p(out["shift"]), p(out["cost"]), p(out["info"]),
                                     int(max_blocks), current_stream()), "poco_op_kp_refit")
    return {k: out[k] for k in shapes}


ACCEL_MAX_JOINTS = 32             # POCO_ACCEL_MAX_JOINTS


def accel_scratch_doubles(N: int) -> int:
    """POCO_ACCEL_SCRATCH_DOUBLES of include/poco_hip.h."""
    return int(N) * 3


def _joint_rows(t, name, need):
    """(N, M, row stride in floats) of joints given as [N,M,3] or as [N,3M] rows; the rows may be a view into wider rows (the
    evaluator's records: records[:, 116:116 + 3 * M]), the floats of a row must be adjacent."""
    need(torch.is_tensor(t) and t.dtype == torch.float32, f"{name} must be a float32 tensor")
    need(t.dim() in (2, 3) and t.shape[0] >= 1, f"{name} must be [N,M,3] or [N,3M], got {tuple(t.shape)}")
    if t.dim() == 3:
        need(t.shape[2] == 3 and t.stride(2) == 1 and t.stride(1) == 3, f"{name} [N,M,3]: the floats of a row must be adjacent")
        M = int(t.shape[1])
    else:
        need(t.shape[1] % 3 == 0 and t.stride(1) == 1, f"{name} [N,3M]: 3M floats per row, adjacent")
        M = int(t.shape[1]) // 3
    need(1 <= M <= ACCEL_MAX_JOINTS, f"{name}: M = {M} is outside 1..{ACCEL_MAX_JOINTS}")
    stride = int(t.stride(0)) if t.shape[0] > 1 else max(int(t.stride(0)), 3 * M)
    need(3 * M <= stride <= 65536, f"{name}: the row stride {stride} must be in 3M = {3 * M} .. 65536")
    return int(t.shape[0]), M, stride


def track_accel(pred: torch.Tensor, gt, frames: torch.Tensor, offsets: torch.Tensor, *, out=None, max_blocks: int = 0):
    """poco_op_track_accel on device tensors: pred and gt (or None) fp32 joints of track-major rows, [N,M,3] or [N,3M] rows that may
    be a view into wider rows (both at the same row stride), frames int32 [N], offsets int32 [P+1] (0 .. N, strictly increasing; a
    host tensor is taken as it is, a device tensor is read back once for the check) -> dict(accel [N], accel_err [N] | None,
    track_sums float64 [P,3], total float64 [3]): per track and over all tracks the sum of accel_err, the sum of accel and the
    number of valid rows.  out = (accel, accel_err | None, track_sums, total): contiguous tensors to write into (tests: guarded
    buffers); max_blocks > 0 caps the grids.  Argument errors raise PocoHipError before any GPU work."""
    def need(ok, what):
        if not ok:
            raise PocoHipError(f"track_accel: {what}")
    N, M, stride = _joint_rows(pred, "pred", need)
    if gt is not None:
        need(_joint_rows(gt, "gt", need) == (N, M, stride), "gt must have pred's shape and row stride")
    need(torch.is_tensor(frames) and frames.dtype == torch.int32 and tuple(frames.shape) == (N,), f"frames must be int32 [{N}]")
    need(torch.is_tensor(offsets) and offsets.dtype == torch.int32 and offsets.dim() == 1 and offsets.numel() >= 2,
         "offsets must be an int32 tensor [P+1], P >= 1")
    need(isinstance(max_blocks, (int, np.integer)) and max_blocks >= 0, f"max_blocks must be an integer >= 0, got {max_blocks!r}")
    P = int(offsets.numel()) - 1
    off = offsets.cpu().numpy()
    need(off[0] == 0 and off[-1] == N and bool(np.all(np.diff(off) > 0)), "offsets must start at 0, end at N and increase strictly")
    for name, t in (("pred", pred), ("gt", gt), ("frames", frames)):
        need(t is None or t.is_cuda, f"{name} must be a CUDA tensor")
    dev = pred.device
    if out is None:
        out = (torch.empty(N, device=dev, dtype=torch.float32), None if gt is None else torch.empty(N, device=dev, dtype=torch.float32),
               torch.empty((P, 3), device=dev, dtype=torch.float64), torch.empty(3, device=dev, dtype=torch.float64))
    need(len(out) == 4, "out must hold accel, accel_err, track_sums and total")
    for t, shp, dt in zip(out, ((N,), (N,), (P, 3), (3,)), (torch.float32, torch.float32, torch.float64, torch.float64)):
        if t is None and shp == (N,) and gt is None:
            continue
        need(t is not None and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shp and t.dtype == dt,
             f"an output must be a contiguous CUDA {dt} {shp}")
    need(out[0] is not None, "accel is needed")
    scratch = torch.empty((accel_scratch_doubles(N),), device=dev, dtype=torch.float64)
    p = lambda t: C.c_void_p(0) if t is None else C.c_void_p(t.data_ptr())      # noqa: E731
    check(lib().poco_op_track_accel(p(pred), p(gt), stride, M, p(frames.contiguous()), p(offsets.to(dev).contiguous()), P, N, p(scratch),
                                    p(out[0]), p(out[1] if gt is not None else None), p(out[2]), p(out[3]), int(max_blocks),
                                    current_stream()), "poco_op_track_accel")
    return {"accel": out[0], "accel_err": out[1] if gt is not None else None, "track_sums": out[2], "total": out[3]}


# ---- SORT: tracks from per-frame detections (include/poco_hip.h; poco_amd/sort.py is the user's side) ---------------------------------
SORT_MAX = 64                     # POCO_SORT_MAX


def sort_tracks(dets: torch.Tensor, frame_offsets, clip_offsets=None, *, iou_thresh: float = 0.3, max_age: int = 1, min_hits: int = 3,
                max_trackers: int = 64, out=None) -> dict:
    """poco_op_sort_tracks: dets fp64 [N,4] (cx, cy, w, h) on the device, frame_offsets int32 [F+1] over the detections and
    clip_offsets int32 [C+1] over the frames (None: one clip), each a host array / list (taken as it is) or a tensor (a device tensor
    is downloaded once for the checks) -> dict(tracker int32 [N], id int32 [N], box fp64 [N,4], count int32 [C], status int32 [C])
    on the device.  out = the same dict of contiguous tensors to write into (tests: guarded buffers).  Refused with PocoHipError
    before any GPU work, the frame named: a frame of more than 64 detections, offsets that are not monotone, a box that is not
    finite or has w <= 0 or h <= 0 (the boxes are downloaded once for that check)."""
    def need(ok, what):
        if not ok:
            raise PocoHipError(f"sort_tracks: {what}")

    def table(t, name):
        dev_t = t if torch.is_tensor(t) and t.is_cuda else None
        a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        need(a.ndim == 1 and a.size >= 1 and a.dtype.kind in "iu", f"{name} must be a 1-D integer table, got {a.dtype} {a.shape}")
        need(bool((a >= 0).all()) and int(a.max()) < (1 << 31), f"{name} must hold int32 values >= 0")
        return np.ascontiguousarray(a, np.int32), dev_t

    need(torch.is_tensor(dets) and dets.dtype == torch.float64, "dets must be a float64 tensor")
    need(dets.dim() == 2 and dets.shape[1] == 4, f"dets must be [N,4] (cx, cy, w, h), got {tuple(dets.shape)}")
    N = int(dets.shape[0])
    fo, fo_dev = table(frame_offsets, "frame_offsets")
    F = int(fo.size) - 1
    co, co_dev = table(np.array([0, F], np.int32) if clip_offsets is None else clip_offsets, "clip_offsets")
    Cn = int(co.size) - 1
    need(Cn >= 1, "clip_offsets must be [C+1] with C >= 1")
    need(co[0] == 0 and co[-1] == F, f"clip_offsets must start at 0 and end at F = {F}")
    bad = np.nonzero(np.diff(co) < 0)[0]
    need(bad.size == 0, f"clip_offsets are not monotone at clip {int(bad[0]) if bad.size else 0}")
    need(fo[0] == 0 and fo[-1] == N, f"frame_offsets must start at 0 and end at N = {N}")
    per = np.diff(fo)
    bad = np.nonzero(per < 0)[0]
    need(bad.size == 0, f"frame_offsets are not monotone at frame {int(bad[0]) if bad.size else 0}")
    bad = np.nonzero(per > SORT_MAX)[0]
    need(bad.size == 0, f"frame {int(bad[0]) if bad.size else 0} holds {int(per[bad[0]]) if bad.size else 0} detections, more than {SORT_MAX}")
    iou_thresh = float(iou_thresh)
    need(np.isfinite(iou_thresh) and 0.0 < iou_thresh < 1.0, f"iou_thresh must be in (0, 1), got {iou_thresh!r}")
    for name, v, lo, hi in (("max_age", max_age, 0, None), ("min_hits", min_hits, 0, None), ("max_trackers", max_trackers, 1, SORT_MAX)):
        need(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and v >= lo and (hi is None or v <= hi) and v < (1 << 31),
             f"{name} must be an integer {'>= ' + str(lo) if hi is None else 'in ' + str(lo) + '..' + str(hi)}, got {v!r}")
    h = dets.detach().cpu().numpy()
    ok = np.isfinite(h).all(1) & (h[:, 2] > 0) & (h[:, 3] > 0) if N else np.ones(0, bool)
    if not ok.all():
        i = int(np.nonzero(~ok)[0][0])
        need(False, f"detection {i} of frame {int(np.searchsorted(fo, i, side='right')) - 1} is not a finite box with w, h > 0: {h[i].tolist()}")
    need(dets.is_cuda, "dets must be a CUDA tensor")
    dev = dets.device
    shapes = {"tracker": ((N,), torch.int32), "id": ((N,), torch.int32), "box": ((N, 4), torch.float64), "count": ((Cn,), torch.int32),
              "status": ((Cn,), torch.int32)}
    if out is None:
        out = {k: torch.empty(s, device=dev, dtype=dt) for k, (s, dt) in shapes.items()}
    for k, (shp, dt) in shapes.items():
        t = out.get(k)
        need(torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shp and t.dtype == dt,
             f"out[{k!r}] must be a contiguous CUDA {dt} {shp}")
    d_fo = fo_dev.to(torch.int32).contiguous() if fo_dev is not None else torch.from_numpy(fo).to(dev)
    d_co = co_dev.to(torch.int32).contiguous() if co_dev is not None else torch.from_numpy(co).to(dev)
    p = lambda t: C.c_void_p(t.data_ptr())                                      # noqa: E731
    with torch.cuda.device(dev):
        check(lib().poco_op_sort_tracks(p(dets.contiguous()), p(d_fo), p(d_co), C.c_int64(Cn), C.c_int64(F), C.c_int64(N),
                                        C.c_double(iou_thresh), int(max_age), int(min_hits), int(max_trackers), p(out["tracker"]),
                                        p(out["id"]), p(out["box"]), p(out["count"]), p(out["status"]), current_stream()),
              "poco_op_sort_tracks")
    return {k: out[k] for k in shapes}


# ---- track stitching: fragments joined into chains (include/poco_hip.h; poco_amd/stitch.py is the user's side) -------------------------
STITCH_MAX_FRAGS = 256            # POCO_STITCH_MAX_FRAGS
STITCH_DESC = 28                  # POCO_STITCH_DESC
STITCH_DEFAULTS = {"max_gap": 30, "fit_len": 8, "u_ref": 0.3, "motion_tol": 0.5, "shape_tol": 1.0, "shape_floor": 0.05, "shape_w": 1.0}


def track_stitch(clip_offsets, frag_offsets, frames: torch.Tensor, boxes: torch.Tensor, betas: torch.Tensor, var: torch.Tensor, *,
                 max_gap: int = 30, fit_len: int = 8, u_ref: float = 0.3, motion_tol: float = 0.5, shape_tol: float = 1.0,
                 shape_floor: float = 0.05, shape_w: float = 1.0, out=None) -> dict:
    """poco_op_track_stitch: clip_offsets int32 [C+1] over the fragments (None: one clip) and frag_offsets int32 [P+1] over the rows,
    each a host array / list or a tensor (a device tensor is downloaded once for the checks); frames int32 [N], boxes fp64 [N,4]
    (cx, cy, w, h), betas fp32 [N,10], var fp32 [N,24] on the device -> dict(succ, pred, chain int32 [P], gain fp64 [P], desc fp64
    [P,28], status int32 [C]) on the device.  out = the same dict of contiguous tensors to write into (tests: guarded buffers).
    Refused with PocoHipError before any GPU work, the fragment named: more than 256 fragments in a clip, an empty fragment, frames
    that do not increase strictly, offsets that are not monotone, a box that is not finite or has w <= 0 or h <= 0, betas or var
    that are not finite, a negative var (the rows are downloaded once for these checks)."""
    def need(ok, what):
        if not ok:
            raise PocoHipError(f"track_stitch: {what}")

    def table(t, name):
        a = t.detach().cpu().numpy() if torch.is_tensor(t) else np.asarray(t)
        need(a.ndim == 1 and a.size >= 1 and a.dtype.kind in "iu", f"{name} must be a 1-D integer table, got {a.dtype} {a.shape}")
        need(bool((a >= 0).all()) and int(a.max()) < (1 << 31), f"{name} must hold int32 values >= 0")
        return np.ascontiguousarray(a, np.int32)

    for name, t, dt, cols in (("frames", frames, torch.int32, None), ("boxes", boxes, torch.float64, 4), ("betas", betas, torch.float32, 10),
                              ("var", var, torch.float32, 24)):
        need(torch.is_tensor(t) and t.dtype == dt, f"{name} must be a {str(dt).replace('torch.', '')} tensor")
        need(t.dim() == 1 if cols is None else (t.dim() == 2 and t.shape[1] == cols),
             f"{name} must be [N]" if cols is None else f"{name} must be [N,{cols}], got {tuple(t.shape)}")
    N = int(frames.shape[0])
    need(boxes.shape[0] == N and betas.shape[0] == N and var.shape[0] == N, f"boxes, betas and var must hold N = {N} rows like frames")
    fo = table(frag_offsets, "frag_offsets")
    P = int(fo.size) - 1
    co = table(np.array([0, P], np.int32) if clip_offsets is None else clip_offsets, "clip_offsets")
    Cn = int(co.size) - 1
    need(Cn >= 1, "clip_offsets must be [C+1] with C >= 1")
    need(co[0] == 0 and co[-1] == P, f"clip_offsets must start at 0 and end at P = {P}")
    per = np.diff(co)
    bad = np.nonzero(per < 0)[0]
    need(bad.size == 0, f"clip_offsets are not monotone at clip {int(bad[0]) if bad.size else 0}")
    bad = np.nonzero(per > STITCH_MAX_FRAGS)[0]
    need(bad.size == 0, f"clip {int(bad[0]) if bad.size else 0} holds {int(per[bad[0]]) if bad.size else 0} fragments, more than {STITCH_MAX_FRAGS}")
    need(fo[0] == 0 and fo[-1] == N, f"frag_offsets must start at 0 and end at N = {N}")
    rows = np.diff(fo)
    bad = np.nonzero(rows < 0)[0]
    need(bad.size == 0, f"frag_offsets are not monotone at fragment {int(bad[0]) if bad.size else 0}")
    bad = np.nonzero(rows == 0)[0]
    need(bad.size == 0, f"fragment {int(bad[0]) if bad.size else 0} is empty")
    for name, v, lo, hi in (("max_gap", max_gap, 0, 1 << 30), ("fit_len", fit_len, 1, 32)):
        need(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and lo <= v <= hi, f"{name} must be an integer in {lo}..{hi}, got {v!r}")
    real = {}
    for name, v, strict in (("u_ref", u_ref, True), ("motion_tol", motion_tol, True), ("shape_tol", shape_tol, True),
                            ("shape_floor", shape_floor, True), ("shape_w", shape_w, False)):
        ok = isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool) and np.isfinite(v) and (v > 0 if strict else v >= 0)
        need(ok, f"{name} must be finite and {'> 0' if strict else '>= 0'}, got {v!r}")
        real[name] = float(v)
    frag_of = lambda i: int(np.searchsorted(fo, i, side="right")) - 1               # noqa: E731
    if N:
        fr = frames.detach().cpu().numpy()
        step = np.diff(fr.astype(np.int64)) > 0
        step[fo[1:-1] - 1] = True                                                   # between two fragments: anything goes
        if not step.all():
            i = int(np.nonzero(~step)[0][0]) + 1
            need(False, f"the frames of fragment {frag_of(i)} do not increase strictly at row {i} ({int(fr[i - 1])} then {int(fr[i])})")
        h = boxes.detach().cpu().numpy()
        ok = np.isfinite(h).all(1) & (h[:, 2] > 0) & (h[:, 3] > 0)
        if not ok.all():
            i = int(np.nonzero(~ok)[0][0])
            need(False, f"row {i} of fragment {frag_of(i)} is not a finite box with w, h > 0: {h[i].tolist()}")
        for name, t in (("betas", betas), ("var", var)):
            a = t.detach().cpu().numpy()
            ok = np.isfinite(a).all(1) & ((a >= 0).all(1) if name == "var" else True)
            if not ok.all():
                i = int(np.nonzero(~ok)[0][0])
                need(False, f"row {i} of fragment {frag_of(i)}: {name} must be finite{' and >= 0' if name == 'var' else ''}")
    for name, t in (("frames", frames), ("boxes", boxes), ("betas", betas), ("var", var)):
        need(t.is_cuda, f"{name} must be a CUDA tensor")
    dev = frames.device
    shapes = {"succ": ((P,), torch.int32), "pred": ((P,), torch.int32), "chain": ((P,), torch.int32), "gain": ((P,), torch.float64),
              "desc": ((P, STITCH_DESC), torch.float64), "status": ((Cn,), torch.int32)}
    if out is None:
        out = {k: torch.empty(s, device=dev, dtype=dt) for k, (s, dt) in shapes.items()}
    for k, (shp, dt) in shapes.items():
        t = out.get(k)
        need(torch.is_tensor(t) and t.is_cuda and t.is_contiguous() and tuple(t.shape) == shp and t.dtype == dt,
             f"out[{k!r}] must be a contiguous CUDA {dt} {shp}")
    d_fo, d_co = torch.from_numpy(fo).to(dev), torch.from_numpy(co).to(dev)
    scratch = torch.empty((max(P, 1) * STITCH_MAX_FRAGS,), device=dev, dtype=torch.float64)
    p = lambda t: C.c_void_p(t.data_ptr())                                      # noqa: E731
    with torch.cuda.device(dev):
        check(lib().poco_op_track_stitch(p(d_co), p(d_fo), p(frames.contiguous()), p(boxes.contiguous()), p(betas.contiguous()),
                                         p(var.contiguous()), C.c_int64(Cn), C.c_int64(P), C.c_int64(N), int(max_gap), int(fit_len),
                                         C.c_double(real["u_ref"]), C.c_double(real["motion_tol"]), C.c_double(real["shape_tol"]),
                                         C.c_double(real["shape_floor"]), C.c_double(real["shape_w"]), p(scratch), p(out["succ"]),
                                         p(out["pred"]), p(out["chain"]), p(out["gain"]), p(out["desc"]), p(out["status"]),
                                         current_stream()), "poco_op_track_stitch")
    return {k: out[k] for k in shapes}


# ---- head kernels on their own, at any stride (include/poco_hip.h; tests/test_head_kernels_gpu.py) ------------------------------
# Every operand lies in a NaN-filled Rows buffer, every output between poisoned guard bands; the output buffers are returned so
# that the caller can check `untouched`.
def rot6d_ex(x, *, in_stride=144, stride0=216, stride1=216, dst0=True, dst1=False):
    """poco_op_rot6d_ex: x [B,144] cuda -> (out0 | None, out1 | None, buffer 0 | None, buffer 1 | None), outputs [B,216]."""
    B = x.shape[0]
    wi = Rows(B, in_stride, x.device, "nan").put(0, x)
    w0 = Rows(B, stride0, x.device, "poison").mark(0, 216) if dst0 else None
    w1 = Rows(B, stride1, x.device, "poison").mark(0, 216) if dst1 else None
    check(lib().poco_op_rot6d_ex(wi.ptr(), in_stride, w0.ptr() if w0 else C.c_void_p(0), stride0, w1.ptr() if w1 else C.c_void_p(0),
                                 stride1, B, current_stream()), "poco_op_rot6d_ex")
    return (w0.get(0, 216) if w0 else None), (w1.get(0, 216) if w1 else None), w0, w1


def lc2d_pose_ex(x, w, *, x_stride=3072):
    """poco_op_lc2d_pose_ex: x [B,128,24], w [6,128,24] -> ([B,24,6], output buffer)."""
    B = x.shape[0]
    wi = Rows(B, x_stride, x.device, "nan").put(0, x)
    ww = Rows(1, 6 * 128 * 24, x.device, "nan").put(0, w)
    wo = Rows(B, 144, x.device, "poison").mark(0, 144)
    check(lib().poco_op_lc2d_pose_ex(wi.ptr(), x_stride, ww.ptr(), wo.ptr(), B, current_stream()), "poco_op_lc2d_pose_ex")
    return wo.get(0, 144).view(B, 24, 6), wo


def copy_rows(x, *, src_stride, dst_stride):
    """poco_op_copy_rows: x [B,n] -> ([B,n], output buffer)."""
    B, n = x.shape
    wi = Rows(B, src_stride, x.device, "nan").put(0, x)
    wo = Rows(B, dst_stride, x.device, "poison").mark(0, n)
    check(lib().poco_op_copy_rows(wi.ptr(), src_stride, wo.ptr(), dst_stride, n, B, current_stream()), "poco_op_copy_rows")
    return wo.get(0, n), wo


def broadcast_rows(v, B, *, dst_stride):
    """poco_op_broadcast_rows: v [n] -> ([B,n], output buffer)."""
    n = v.numel()
    wi = Rows(1, n, v.device, "nan").put(0, v)
    wo = Rows(B, dst_stride, v.device, "poison").mark(0, n)
    check(lib().poco_op_broadcast_rows(wi.ptr(), wo.ptr(), dst_stride, n, B, current_stream()), "poco_op_broadcast_rows")
    return wo.get(0, n), wo


def nhwc_to_nchw(x, *, cs, C_out=None):
    """poco_op_nhwc_to_nchw: x NHWC [B,H,W,Cx] at channel 0 of an L16 buffer with cs channels; its first C_out (default Cx)
    channels -> (NCHW [B,C_out,H,W], output buffer)."""
    B, H, W, Cx = x.shape
    Cc = Cx if C_out is None else C_out
    wi = Wide(B, H, W, cs, x.device, "nan").put(0, x)
    wo = Rows(1, B * Cc * H * W, x.device, "poison").mark(0, B * Cc * H * W)
    check(lib().poco_op_nhwc_to_nchw(wi.base(), cs, wo.ptr(), B, H, W, Cc, current_stream()), "poco_op_nhwc_to_nchw")
    return wo.get(0, B * Cc * H * W).view(B, Cc, H, W), wo


def pack_record(rot, betas, cam, var, *, cliff, kinematic, thr=0.4, rot_stride=216, betas_stride=10, cam_stride=3, var_stride=24):
    """poco_op_pack_record: rot [B,216], betas [B,10], cam [B,3], var [B,24] -> (records [B,254], output buffer)."""
    B = rot.shape[0]
    wr = Rows(B, rot_stride, rot.device, "nan").put(0, rot)
    wb = Rows(B, betas_stride, rot.device, "nan").put(0, betas)
    wc = Rows(B, cam_stride, rot.device, "nan").put(0, cam)
    wv = Rows(B, var_stride, rot.device, "nan").put(0, var)
    wo = Rows(B, 254, rot.device, "poison").mark(0, 254)
    check(lib().poco_op_pack_record(wr.ptr(), rot_stride, wb.ptr(), betas_stride, wc.ptr(), cam_stride, wv.ptr(), var_stride, wo.ptr(),
                                    int(cliff), int(kinematic), C.c_float(thr), B, current_stream()), "poco_op_pack_record")
    return wo.get(0, 254), wo


def camera(cam, joints49, *, cliff=False, focal=None, scale=None, center=None, orig_shape=None, cam_stride=3, fullimg=True):
    """poco_op_camera: cam [B,3] = (s, tx, ty), joints49 [B,49,3]; cliff: focal [B], scale [B], center [B,2], orig_shape [B,2] ->
    dict(cam_t [B,3], fullimg_cam_t [B,3] | None, joints2d [B,49,2], bufs = the three output buffers).  fullimg = False passes a
    null d_fullimg_cam_t."""
    B, dev = cam.shape[0], cam.device
    wc = Rows(B, cam_stride, dev, "nan").put(0, cam)
    wj = Rows(1, B * 147, dev, "nan").put(0, joints49.reshape(1, -1))
    side = [None if t is None else Rows(1, t.numel(), dev, "nan").put(0, t.reshape(1, -1)) for t in (focal, scale, center, orig_shape)]
    wt = Rows(1, B * 3, dev, "poison").mark(0, B * 3)
    wf = Rows(1, B * 3, dev, "poison")
    if cliff and fullimg:
        wf.mark(0, B * 3)
    w2 = Rows(1, B * 98, dev, "poison").mark(0, B * 98)
    null = C.c_void_p(0)
    check(lib().poco_op_camera(wc.ptr(), cam_stride, wj.ptr(), int(cliff), *[null if w is None else w.ptr() for w in side], wt.ptr(),
                               wf.ptr() if fullimg else null, w2.ptr(), B, current_stream()), "poco_op_camera")
    return dict(cam_t=wt.get(0, B * 3).view(B, 3), fullimg_cam_t=wf.get(0, B * 3).view(B, 3) if cliff and fullimg else None,
                joints2d=w2.get(0, B * 98).view(B, 49, 2), bufs=(wt, wf, w2))


def mlp_chain_resident_blocks() -> int:
    return int(lib().poco_op_mlp_chain_resident_blocks())


def mlp_chain(layers, rows, stages, bufs, B, max_blocks=256):
    """poco_op_mlp_chain on Rows buffers (the row stride of an operand is its buffer's):
    layers = [dict(W=[N,K] numpy, b=[N] numpy, act=0|1|2, src=(buf, off), res=(buf, off) | None, dst=(buf, off)), ...],
    rows   = [dict(kind=0|1|2, src=(buf, off), dst=(buf, off) | None, dst2=(buf, off) | None, n=...), ...] (a broadcast source is
             one row: its buffer's stride is not used),
    stages = [(layer0, nlayers, row0, nrows), ...].  Returns the status (0 = ok); PocoHipError on a refused program."""
    li, ws, bs = [], [], []
    for L in layers:
        W = np.ascontiguousarray(L["W"], dtype=np.float32)
        b = np.ascontiguousarray(L["b"], dtype=np.float32)
        N, K = W.shape
        res = L.get("res")
        li += [K, N, int(L.get("act", 0)), L["src"][0], L["src"][1], bufs[L["src"][0]].stride]
        li += [-1, 0, 0] if res is None else [res[0], res[1], bufs[res[0]].stride]
        li += [L["dst"][0], L["dst"][1], bufs[L["dst"][0]].stride]
        ws.append(W)
        bs.append(b)
    ri = []
    for J in rows:
        ri += [int(J["kind"]), J["src"][0], J["src"][1], bufs[J["src"][0]].stride]
        for key in ("dst", "dst2"):
            d = J.get(key)
            ri += [-1, 0, 0] if d is None else [d[0], d[1], bufs[d[0]].stride]
        ri.append(int(J.get("n", 0)))
    si = [int(v) for st in stages for v in st]
    nl, nr, ns, nb = len(layers), len(rows), len(stages), len(bufs)
    arr = lambda v: (C.c_int * max(len(v), 1))(*v)
    wp = (C.c_void_p * max(nl, 1))(*[w.ctypes.data for w in ws])
    bp = (C.c_void_p * max(nl, 1))(*[b.ctypes.data for b in bs])
    dp = (C.c_void_p * nb)(*[w.ptr().value for w in bufs])
    # what the entry may touch: the rows and nothing of the guard bands
    sizes = (C.c_longlong * nb)(*[w.rows * w.stride for w in bufs])
    rc = lib().poco_op_mlp_chain(arr(li), nl, wp, bp, arr(ri), nr, arr(si), ns, dp, sizes, nb, int(B), int(max_blocks), current_stream())
    check(rc, "poco_op_mlp_chain")
    return rc


# ---- image degradation of raw crops (include/poco_hip.h poco_op_corrupt; poco_amd/corrupt.py is the user's side) ------------------
CORRUPT_MAX_STEPS = 4
CORRUPT_KINDS = ("none", "gaussian_blur", "motion_blur", "pixelate", "contrast", "gamma", "gaussian_noise", "jpeg")
CORRUPT_JPEG = CORRUPT_KINDS.index("jpeg")
# poco_corrupt_step_t
CORRUPT_STEP = np.dtype([("kind", np.int32), ("ival", np.int32), ("p0", np.float32), ("p1", np.float32), ("seed", np.uint32, (2,)),
                         ("stream", np.uint32)])
assert CORRUPT_STEP.itemsize == 28
_corrupt_codecs = {}


def _corrupt_codec(device, res: int):
    """The JPEG encoder and decoder of res x res crops on `device`, made once."""
    from . import jpeg
    key = (str(device), int(res))
    if key not in _corrupt_codecs:
        # quality 100 on a noisy crop: the stream can approach the encoder's worst case, far above the decoder's default room
        _corrupt_codecs[key] = (jpeg.JpegEncoder(device, res, res),
                                jpeg.JpegDecoder(device, res, res, 1, max_bytes=jpeg.worst_case_bytes(res, res)))
    return _corrupt_codecs[key]


def _corrupt_jpeg_round_trip(buf: torch.Tensor, crops, qualities) -> None:
    """buf fp32 [N,3,res,res] holding whole numbers in [0, 255] in the crops named: each goes through poco_jpeg_encode and the
    decoder as a picture of its own (4:2:0 fancy upsampling looks across a seam of stacked pictures), in place.  The decoder
    parses the stream on the host, so every picture costs one read-back of its bytes."""
    enc, dec = _corrupt_codec(buf.device, int(buf.shape[-1]))
    for n, q in zip(crops, qualities):
        frame = buf[n].permute(1, 2, 0).to(torch.uint8).contiguous()
        pix, status = dec.decode([enc.encode(frame, int(q))], return_status=True)
        if status[0] != 0:
            raise PocoHipError(f"corrupt: the decoder refused the encoder's stream of crop {n} (status {status[0]})")
        buf[n].copy_(pix[0].permute(2, 0, 1))


def corrupt(x: torch.Tensor, steps: np.ndarray, normalize: bool = False, *, out: torch.Tensor = None, tmp: torch.Tensor = None) -> torch.Tensor:
    """poco_op_corrupt on raw crops: x fp32 [N,3,res,res] in [0, 255] on the device, steps = a host array [N,L] of CORRUPT_STEP
    records (L <= 4; a chain ends at its first `none`) -> fp32 [N,3,res,res], raw or with normalize=True mapped as
    oracle/crop_np.normalize_np.  out and tmp: the two buffers the launches ping-pong between (made here if not given; x is only
    read).  Chains without a jpeg step are one call: no allocation beyond the buffers, no synchronisation.  With a jpeg step the
    chain positions are run one by one and the crops whose step at that position is jpeg take the round trip through the
    encoder and the decoder in between (this reads their bytes back).  Argument errors raise PocoHipError before any GPU work."""
    def need(ok, what):
        if not ok:
            raise PocoHipError(f"corrupt: {what}")
    need(torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 and x.is_contiguous() and x.dim() == 4 and x.shape[1] == 3
         and x.shape[2] == x.shape[3], "x must be a contiguous float32 CUDA [N,3,res,res]")
    N, res = int(x.shape[0]), int(x.shape[2])
    need(isinstance(steps, np.ndarray) and steps.dtype == CORRUPT_STEP and steps.ndim == 2 and steps.shape[0] == N,
         f"steps must be a numpy array [{N},L] of ops.CORRUPT_STEP records")
    L = int(steps.shape[1])
    need(1 <= L <= CORRUPT_MAX_STEPS, f"a chain holds 1..{CORRUPT_MAX_STEPS} steps, got {L}")
    steps = np.ascontiguousarray(steps)
    bufs = {}
    for name, b in (("out", out), ("tmp", tmp)):
        if b is None:
            b = torch.empty_like(x)
        need(torch.is_tensor(b) and b.is_cuda and b.device == x.device and b.dtype == torch.float32 and b.is_contiguous() and b.shape == x.shape,
             f"{name} must be a contiguous float32 CUDA tensor of x's shape on x's device")
        bufs[name] = b
    out, tmp = bufs["out"], bufs["tmp"]
    need(len({x.data_ptr(), out.data_ptr(), tmp.data_ptr()}) == 3, "x, out and tmp must be three buffers")
    d_steps = torch.from_numpy(steps.view(np.uint8).reshape(-1)).to(x.device)
    fn = lib().poco_op_corrupt
    fn.argtypes = [C.c_void_p] * 3 + [C.c_int] * 6 + [C.c_void_p] * 3

    def call(src, lo, hi, norm, scratch, dst):
        with torch.cuda.device(x.device):
            check(fn(src.data_ptr(), d_steps.data_ptr(), steps.ctypes.data, N, L, lo, hi, res, int(bool(norm)), scratch.data_ptr(),
                     dst.data_ptr(), current_stream()), "poco_op_corrupt")
    kinds = steps["kind"]
    if not (kinds == CORRUPT_JPEG).any():
        call(x, 0, L, normalize, tmp, out)
        return out
    # with a jpeg step: one call per position, the round trips in between.  Every call is a single launch src -> dst (its scratch
    # buffer is not written), the targets alternate so that the last one is `out`: the last position's, or the normalising copy's.
    P = int((kinds != 0).sum(1).max())
    spare = torch.empty_like(x)
    last = tmp if normalize else out
    src = x
    for p in range(P):
        dst = last if (P - 1 - p) % 2 == 0 else (out if last is tmp else tmp)
        call(src, p, p + 1, False, spare, dst)
        jp = np.nonzero(kinds[:, p] == CORRUPT_JPEG)[0]
        _corrupt_jpeg_round_trip(dst, jp.tolist(), steps["ival"][jp, p].tolist())
        src = dst
    if normalize:
        call(src, L, L, True, spare, out)
    return out
