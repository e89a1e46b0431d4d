"""The kernels only the engine launches - bneck_chain, the two-source 1x1 GEMM, fuse_sum, bilinear x2, the 3x3 max pool, the
global average pool, both stem convs - each on its own through its poco_op_* entry, against fp64 torch on the CPU.

Until now they were compared only as fused engine against separate engine, or engine against oracle, on the final pose / shape /
camera / vertices: after global pooling and several MLPs.  (The ResNet max pool only ever sees post-ReLU input in the model: a
kernel padding with 0 instead of -inf passes all of that.)  Every operand lives in a poisoned buffer (ops.Wide): NaN wherever the
kernel has no business reading, a bit pattern wherever it must not write, NaN where it must write.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def _check(out, wide, co, C, ref, tol, floor=1.0):
    """|out - ref|max <= tol * max(floor, |ref|max): floor = 1 is the project's convention for the conv kernels; floor = 0 makes the
    bound plainly relative to the largest reference value (the pools and sums whose tolerance is stated as relative)."""
    out = out.cpu().numpy()
    assert out.shape == ref.shape, (out.shape, ref.shape)
    nan = int(np.isnan(out).sum())
    assert nan == 0, f"{nan} NaN of {out.size}: unwritten elements, or NaN-poisoned foreign memory in the arithmetic"
    assert wide.untouched(co, C), "stray write outside the output slice (neighbour channels / guard band)"
    err = np.abs(out - ref).max() / max(floor, np.abs(ref).max())
    print(f"rel err {err:.2e}")
    assert err <= tol, err


def _bn(rng, C):
    return rng.uniform(0.5, 1.5, C).astype(np.float32), rng.uniform(-0.3, 0.3, C).astype(np.float32)


# ---- bneck_chain ---------------------------------------------------------------------------------------------------------------
def _chain_case(B, H, W, slices, cuda):
    from poco_amd import ops
    rng = np.random.default_rng(B * 100 + H + W)
    t = rng.standard_normal((B, H, W, 64)).astype(np.float32)
    res = rng.standard_normal((B, H, W, 256)).astype(np.float32)
    w3 = (rng.standard_normal((256, 64, 1, 1)) / 8).astype(np.float32)
    w1 = (rng.standard_normal((64, 256, 1, 1)) / 16).astype(np.float32)
    s3, b3 = _bn(rng, 256)
    s1, b1 = _bn(rng, 64)
    kw = dict(t_cs=128, t_co=32, res_cs=320, res_co=48, y_cs=288, y_co=16, u_cs=96, u_co=32) if slices else {}
    y, u, wy, wu = ops.bneck_chain(torch.from_numpy(t).to(cuda), torch.from_numpy(res).to(cuda), w3, s3, b3, w1, s1, b1, **kw)
    td, rd = torch.from_numpy(t).double(), torch.from_numpy(res).double()
    yr = ((td @ torch.from_numpy(w3[:, :, 0, 0]).double().t()) * torch.from_numpy(s3).double() + torch.from_numpy(b3).double() + rd).clamp_min(0)
    ur = ((yr @ torch.from_numpy(w1[:, :, 0, 0]).double().t()) * torch.from_numpy(s1).double() + torch.from_numpy(b1).double()).clamp_min(0)
    _check(y, wy, kw.get("y_co", 0), 256, yr.numpy(), 2e-5)
    _check(u, wu, kw.get("u_co", 0), 64, ur.numpy(), 2e-5)


@pytest.mark.parametrize("slices", [False, True])
@pytest.mark.parametrize("shape", [(1, 3, 3), (1, 1, 1), (3, 13, 9)], ids=lambda s: "x".join(map(str, s)))
def test_bneck_chain(shape, slices, cuda):
    """9 and 1 pixels: below one 16-pixel sub-tile; 3 x 13 x 9 = 351 pixels: ragged, sub-tiles straddle rows and images."""
    _chain_case(*shape, slices, cuda)


def test_bneck_chain_waves_walk_several_tiles(cuda):
    """More 16-pixel sub-tiles than the persistent grid holds (the count comes from the launcher): every wave walks at least two,
    most of them three, and the last sub-tile is partial."""
    from poco_amd import ops
    resident = ops.bneck_chain_resident_tiles()
    W = 9
    rows = -(-(2 * resident * 16 + 100) // W)           # pixels > 2 x resident sub-tiles, not a multiple of 16
    assert rows * W > 2 * resident * 16 and (rows * W) % 16
    _chain_case(1, rows, W, True, cuda)


# ---- two-source 1x1 GEMM -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("act", [0, 1])
@pytest.mark.parametrize("layout", [0, 41, 12, 322, 618])
@pytest.mark.parametrize("B", [1, 5])
@pytest.mark.parametrize("H2", [14, 13])
def test_conv1x1_dual(H2, B, layout, act, cuda):
    """Stride-2 second source from an even and an odd plane (14 -> 7, 13 -> 7); output as a slice of a wider buffer; wave layouts:
    the one-wave default, the engine's 41, and 1 x 2, 2 x 2 with schedule 3, 1 x 8 with schedule 6 (more n-waves than n-groups)."""
    from poco_amd import ops
    Ho, Ca, Cb, Cout = 7, 32, 48, 128
    rng = np.random.default_rng(H2 * 10 + B)
    a = rng.standard_normal((B, Ho, Ho, Ca)).astype(np.float32)
    b = rng.standard_normal((B, H2, H2, Cb)).astype(np.float32)
    wa = (rng.standard_normal((Cout, Ca, 1, 1)) / np.sqrt(Ca + Cb)).astype(np.float32)
    wb = (rng.standard_normal((Cout, Cb, 1, 1)) / np.sqrt(Ca + Cb)).astype(np.float32)
    sa, ba = _bn(rng, Cout)
    sb, bb = _bn(rng, Cout)
    out, wo = ops.conv1x1_dual(torch.from_numpy(a).to(cuda), torch.from_numpy(b).to(cuda), wa, sa, ba, wb, sb, bb, 2, act, layout,
                               a_cs=64, a_co=16, b_cs=96, b_co=32, out_cs=Cout + 48, out_co=32)
    d = lambda v: torch.from_numpy(v).double()
    ya = F.conv2d(d(a).permute(0, 3, 1, 2), d(wa)) * d(sa).view(1, -1, 1, 1) + d(ba).view(1, -1, 1, 1)
    yb = F.conv2d(d(b).permute(0, 3, 1, 2), d(wb), stride=2) * d(sb).view(1, -1, 1, 1) + d(bb).view(1, -1, 1, 1)
    ref = (ya + yb).permute(0, 2, 3, 1)
    if act:
        ref = ref.clamp_min(0)
    _check(out, wo, 32, Cout, ref.numpy(), 2e-5)


def test_conv1x1_dual_refuses_unknown_layout(cuda):
    from poco_amd import ops
    z = torch.zeros(1, 7, 7, 16, device=cuda)
    w = np.zeros((64, 16, 1, 1), np.float32)
    for layout in (99, 242, 7, -1):      # 9 x 9 waves; load schedule 2; WM = 0; negative
        with pytest.raises(RuntimeError):
            ops.conv1x1_dual(z, torch.zeros(1, 14, 14, 16, device=cuda), w, None, None, w, None, None, 2, 1, layout)


# ---- fuse_sum ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("C", [16, 48])
@pytest.mark.parametrize("n", [1, 2, 3, 4])
@pytest.mark.parametrize("H", [8, 56])
def test_fuse_sum(H, n, C, relu, cuda):
    """1 to 4 terms, term k upsampled by 2^k onto an H x H plane, every term and the output a slice of a wider buffer.  fp32 sums of
    at most four addends in a fixed order: within 1e-6 relative of the fp64 sum."""
    from poco_amd import ops
    B = 2
    rng = np.random.default_rng(H + 10 * n + C)
    terms = [rng.standard_normal((B, H >> k, H >> k, C)).astype(np.float32) for k in range(n)]
    shifts = list(range(n))
    out, wo = ops.fuse_sum([torch.from_numpy(t).to(cuda) for t in terms], shifts, relu,
                           src_cs=[C + 16 * (k + 1) for k in range(n)], src_co=[16 * (k % 2) for k in range(n)], out_cs=C + 32, out_co=16)
    ref = sum(np.repeat(np.repeat(t.astype(np.float64), 1 << k, 1), 1 << k, 2) for k, t in enumerate(terms))
    if relu:
        ref = np.maximum(ref, 0)
    _check(out, wo, 16, C, ref, 1e-6, floor=0.0)


# ---- bilinear x2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 7, 7, 32), (3, 13, 9, 16), (2, 1, 1, 16), (1, 1, 5, 16)], ids=lambda s: "x".join(map(str, s)))
def test_bilinear_up2x(shape, cuda):
    """align_corners=True divides by H - 1: the 1 x 1 plane (and a 1 x 5 one) must come out as the plain replication torch gives."""
    from poco_amd import ops
    B, H, W, C = shape
    x = np.random.default_rng(H * W).standard_normal(shape).astype(np.float32)
    out, wo = ops.bilinear_up2x(torch.from_numpy(x).to(cuda))
    ref = F.interpolate(torch.from_numpy(x).double().permute(0, 3, 1, 2), scale_factor=2, mode="bilinear", align_corners=True)
    _check(out, wo, 0, C, ref.permute(0, 2, 3, 1).numpy(), 1e-6)


# ---- max pool ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 7, 7, 32), (2, 8, 8, 16), (3, 1, 1, 16), (1, 112, 112, 64), (2, 13, 9, 16)],
                         ids=lambda s: "x".join(map(str, s)))
def test_maxpool_negative_input(shape, cuda):
    """All-negative input: a pool that pads with 0 instead of -inf returns 0 along the border.  Bitwise the fp64 reference rounded
    to fp32 (a max of fp32 values is exact); output as a slice of a wider buffer."""
    from poco_amd import ops
    B, H, W, C = shape
    x = (-np.abs(np.random.default_rng(H + W).standard_normal(shape)) - 0.5).astype(np.float32)
    out, wo = ops.maxpool3x3s2(torch.from_numpy(x).to(cuda), out_cs=C + 32, out_co=16)
    ref = F.max_pool2d(torch.from_numpy(x).double().permute(0, 3, 1, 2), 3, 2, 1).permute(0, 2, 3, 1).numpy().astype(np.float32)
    assert out.shape == ref.shape
    assert wo.untouched(16, C)
    assert np.array_equal(out.cpu().numpy(), ref)


# ---- global average pool -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("C", [16, 2048])
@pytest.mark.parametrize("hw", [(1, 1), (7, 7), (56, 56)], ids=lambda s: "x".join(map(str, s)))
def test_avgpool(hw, C, cuda):
    """H W = 1, 49, 3136; rows of dst_stride > C floats with the pool at a column offset: the gaps keep their bit pattern.
    Post-ReLU-like input (|N(0,1)|, mean 0.8), as the pools of the models see; 2e-6 relative to |ref|max (about 0.85 for the planes, the largest input for H W = 1)."""
    from poco_amd import ops
    B = 3
    x = np.abs(np.random.default_rng(C + hw[0]).standard_normal((B, *hw, C))).astype(np.float32)
    out, wo = ops.avgpool(torch.from_numpy(x).to(cuda), dst_stride=C + 24, dst_off=8)
    ref = x.astype(np.float64).mean((1, 2))
    _check(out, wo, 8, C, ref, 2e-6, floor=0.0)


# ---- stem convs ----------------------------------------------------------------------------------------------------------------
def _stem(B, H, W, ks, use_mfma, cuda):
    from poco_amd import ops
    rng = np.random.default_rng(ks * 1000 + H + B)
    img = rng.standard_normal((B, 3, H, W)).astype(np.float32)
    w = (rng.standard_normal((64, 3, ks, ks)) / np.sqrt(3 * ks * ks)).astype(np.float32)
    scale, shift = _bn(rng, 64)
    out, wo = ops.stem_conv(torch.from_numpy(img).to(cuda), w, scale, shift, use_mfma)
    d = lambda v: torch.from_numpy(v).double()
    ref = (F.conv2d(d(img), d(w), stride=2, padding=(ks - 1) // 2) * d(scale).view(1, -1, 1, 1) + d(shift).view(1, -1, 1, 1)).clamp_min(0)
    _check(out, wo, 0, 64, ref.permute(0, 2, 3, 1).numpy(), 2e-5)


@pytest.mark.parametrize("use_mfma", [0, 1])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("ks", [3, 7])
def test_stem_conv_224(ks, B, use_mfma, cuda):
    _stem(B, 224, 224, ks, use_mfma, cuda)


@pytest.mark.parametrize("use_mfma", [0, 1])
@pytest.mark.parametrize("hw", [(15, 11), (16, 16), (9, 30)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("ks", [3, 7])
def test_stem_conv_small_images(ks, hw, use_mfma, cuda):
    """15 x 11 -> 8 x 6 (one pixel per thread), 16 x 16 -> 8 x 8 and 9 x 30 -> 5 x 15 | 5 x 16 (four pixels per thread where the
    output width allows).  The MFMA form does not cover these widths: asking for it must give the same answer through the fallback."""
    _stem(2, hw[0], hw[1], ks, use_mfma, cuda)
