"""CPU: the stand-alone operator entries of the view conv and the backbone side kernels (include/poco_hip.h) are declared, exported
and refuse bad arguments with POCO_ERR_ARG (1) and a message before any GPU work - so all of it runs on a machine without a GPU,
with fake device pointers that are never dereferenced (as tests/test_eval_cpu.py does for poco_op_rodrigues)."""
import ctypes as C

import numpy as np
import pytest

from poco_amd import _lib

NEW = ["poco_op_conv2d_ex", "poco_op_bneck_chain", "poco_op_bneck_chain_resident_tiles", "poco_op_conv1x1_dual", "poco_op_fuse_sum",
       "poco_op_bilinear_up2x", "poco_op_maxpool3x3s2", "poco_op_avgpool", "poco_op_stem_conv",
       # the head kernels on their own (tests/test_head_kernels_gpu.py)
       "poco_op_camera", "poco_op_mlp_chain", "poco_op_mlp_chain_resident_blocks", "poco_op_rot6d_ex", "poco_op_lc2d_pose_ex",
       "poco_op_copy_rows", "poco_op_broadcast_rows", "poco_op_nhwc_to_nchw", "poco_op_pack_record"]
FAKE = C.c_void_p(4096)          # never dereferenced: every call below is refused before a pointer is used
NULL = C.c_void_p(0)
ERR_ARG = 1


@pytest.fixture(scope="module")
def L():
    return _lib.lib()


def _msg(L):
    return L.poco_last_error().decode()


def test_new_entries_are_declared_and_exported(L):
    syms = _lib.header_symbols()
    for s in NEW:
        assert s in syms, s
        assert hasattr(L, s), s
    assert "#define POCO_ABI_VERSION 4" in _lib.HEADER.read_text()         # additions only: the ABI version is not bumped
    abi = (_lib.ROOT.parent / "tests" / "c_abi" / "abi_check.c").read_text()
    for s in NEW:
        assert s in abi, s


def _conv_ex(L, d_in=FAKE, B=2, H=5, W=3, Cin=32, in_cs=64, in_co=16, w=True, Cout=32, ks=3, stride=1, d_res=FAKE, res_cs=64, res_co=16,
             act=1, relu_from=0, res_after=0, d_out=FAKE, out_cs=64, out_co=32, cfg=None):
    wt = np.zeros((Cout if Cout > 0 else 1, max(Cin, 1), ks, ks), np.float32)
    arr = None if cfg is None else (C.c_int * 7)(*cfg)
    return L.poco_op_conv2d_ex(d_in, B, H, W, Cin, in_cs, in_co, C.c_void_p(wt.ctypes.data) if w else NULL, NULL, NULL, Cout, ks, stride,
                               d_res, res_cs, res_co, act, relu_from, res_after, d_out, out_cs, out_co, arr, NULL)


def test_conv2d_ex_argument_errors(L):
    for kw, word in [(dict(d_in=NULL), "null"), (dict(d_out=NULL), "null"), (dict(w=False), "null"),
                     (dict(in_cs=32), "in_cs"),                         # stride smaller than offset + width
                     (dict(out_cs=48), "out_cs"), (dict(res_cs=32), "res_cs"),
                     (dict(in_co=4), "multiples of 16"),                # a plane admits whole 16-channel slices only
                     (dict(out_co=8, out_cs=48), "multiples of 16"), (dict(res_cs=72), "multiples of 16"), (dict(in_co=-16), "multiples"),
                     (dict(H=1, W=1, in_co=2), "multiples of 4"),       # rows: multiples of 4 ...
                     (dict(H=1, W=1, ks=3, in_co=4, cfg=(4, 4, 1, 1, 2, 1, 11)), "multiples of 16"),    # ... except for ALG 11
                     (dict(act=3, relu_from=8), "relu_from"), (dict(act=3, relu_from=48), "relu_from"), (dict(relu_from=-16), "relu_from"),
                     (dict(act=4), "act"), (dict(act=-1), "act"), (dict(res_after=2), "res_after_act"),
                     (dict(Cout=24), "Cout"), (dict(ks=5), "ks"), (dict(stride=3), "stride"), (dict(B=0), "B")]:
        assert _conv_ex(L, **kw) == ERR_ARG, kw
        assert "conv2d_ex" in _msg(L) and word in _msg(L), (kw, _msg(L))
    # without a residual its stride and offset are not looked at
    assert _conv_ex(L, d_res=NULL, res_cs=0, res_co=3, d_in=NULL) == ERR_ARG and "null" in _msg(L)


def test_side_kernel_argument_errors(L):
    w3, w1 = np.zeros(256 * 64, np.float32), np.zeros(64 * 256, np.float32)
    p3, p1 = C.c_void_p(w3.ctypes.data), C.c_void_p(w1.ctypes.data)

    def chain(t=FAKE, t_cs=64, res=FAKE, res_cs=256, y=FAKE, y_cs=256, u=FAKE, u_cs=64, a=p3, b=p1, B=1, H=4, W=4):
        return L.poco_op_bneck_chain(t, t_cs, res, res_cs, y, y_cs, u, u_cs, a, NULL, NULL, b, NULL, NULL, B, H, W, NULL)
    for kw in (dict(t=NULL), dict(res=NULL), dict(y=NULL), dict(u=NULL), dict(a=NULL), dict(b=NULL), dict(t_cs=48), dict(res_cs=240),
               dict(y_cs=264), dict(u_cs=32), dict(B=0), dict(W=0)):
        assert chain(**kw) == ERR_ARG and "bneck_chain" in _msg(L), kw
    assert L.poco_op_bneck_chain_resident_tiles() >= 16

    wa = np.zeros(64 * 32, np.float32)
    pa = C.c_void_p(wa.ctypes.data)

    def dual(a=FAKE, a_cs=32, Ca=32, b=FAKE, b_cs=32, Cb=32, H2=14, W2=14, s2=2, x=pa, y=pa, out=FAKE, out_cs=64, Cout=64, B=1, Ho=7, Wo=7,
             act=1, layout=0):
        return L.poco_op_conv1x1_dual(a, a_cs, Ca, b, b_cs, Cb, H2, W2, s2, x, NULL, NULL, y, NULL, NULL, out, out_cs, Cout, B, Ho, Wo, act,
                                      layout, NULL)
    for kw in (dict(a=NULL), dict(b=NULL), dict(out=NULL), dict(x=NULL), dict(y=NULL), dict(a_cs=16), dict(b_cs=24), dict(out_cs=48),
               dict(Cout=32, out_cs=32), dict(Ca=24), dict(s2=3), dict(H2=15), dict(W2=12), dict(act=2), dict(layout=99), dict(layout=242),
               dict(layout=-1), dict(layout=7), dict(layout=70), dict(B=0)):
        assert dual(**kw) == ERR_ARG and "conv1x1_dual" in _msg(L), kw

    def fuse(n=2, src=(4096, 8192), cs=(32, 48), sh=(0, 1), out=FAKE, out_cs=32, B=1, H=8, W=8, Cc=32, arrays=True):
        k = max(len(src), 1)
        ps = (C.c_void_p * k)(*src)
        return L.poco_op_fuse_sum(n, ps if arrays else NULL, (C.c_int * k)(*cs), (C.c_int * k)(*sh), out, out_cs, B, H, W, Cc, 1, NULL)
    for kw in (dict(arrays=False), dict(out=NULL), dict(src=(4096, 0)), dict(n=0), dict(n=5), dict(cs=(32, 16)), dict(cs=(32, 40)),
               dict(out_cs=16), dict(sh=(0, 4)), dict(sh=(0, -1)), dict(H=7, sh=(0, 1)), dict(Cc=24, out_cs=48), dict(B=0)):
        assert fuse(**kw) == ERR_ARG and "fuse_sum" in _msg(L), kw

    assert L.poco_op_bilinear_up2x(NULL, FAKE, 1, 4, 4, 16, NULL) == ERR_ARG and "bilinear" in _msg(L)
    assert L.poco_op_bilinear_up2x(FAKE, NULL, 1, 4, 4, 16, NULL) == ERR_ARG
    assert L.poco_op_bilinear_up2x(FAKE, FAKE, 1, 4, 4, 24, NULL) == ERR_ARG and L.poco_op_bilinear_up2x(FAKE, FAKE, 1, 0, 4, 16, NULL) == ERR_ARG

    assert L.poco_op_maxpool3x3s2(NULL, FAKE, 1, 4, 4, 16, 16, NULL) == ERR_ARG and "maxpool" in _msg(L)
    assert L.poco_op_maxpool3x3s2(FAKE, NULL, 1, 4, 4, 16, 16, NULL) == ERR_ARG
    assert L.poco_op_maxpool3x3s2(FAKE, FAKE, 1, 4, 4, 32, 16, NULL) == ERR_ARG          # out_cs < C
    assert L.poco_op_maxpool3x3s2(FAKE, FAKE, 1, 4, 4, 16, 24, NULL) == ERR_ARG and L.poco_op_maxpool3x3s2(FAKE, FAKE, 1, 4, 0, 16, 16, NULL) == ERR_ARG

    assert L.poco_op_avgpool(NULL, FAKE, 1, 4, 4, 16, 16, NULL) == ERR_ARG and "avgpool" in _msg(L)
    assert L.poco_op_avgpool(FAKE, NULL, 1, 4, 4, 16, 16, NULL) == ERR_ARG
    assert L.poco_op_avgpool(FAKE, FAKE, 1, 4, 4, 32, 16, NULL) == ERR_ARG               # dst_stride < C
    assert L.poco_op_avgpool(FAKE, C.c_void_p(4100), 1, 4, 4, 16, 16, NULL) == ERR_ARG and "16-byte" in _msg(L)     # float4 stores
    assert L.poco_op_avgpool(FAKE, FAKE, 1, 4, 4, 16, 18, NULL) == ERR_ARG and L.poco_op_avgpool(FAKE, FAKE, 1, 4, 4, 8, 16, NULL) == ERR_ARG

    ws = np.zeros(64 * 3 * 49, np.float32)
    pw = C.c_void_p(ws.ctypes.data)
    assert L.poco_op_stem_conv(NULL, pw, NULL, NULL, FAKE, 1, 224, 224, 7, 1, NULL) == ERR_ARG and "stem_conv" in _msg(L)
    assert L.poco_op_stem_conv(FAKE, NULL, NULL, NULL, FAKE, 1, 224, 224, 7, 1, NULL) == ERR_ARG
    assert L.poco_op_stem_conv(FAKE, pw, NULL, NULL, NULL, 1, 224, 224, 7, 1, NULL) == ERR_ARG
    assert L.poco_op_stem_conv(FAKE, pw, NULL, NULL, FAKE, 1, 224, 224, 5, 1, NULL) == ERR_ARG
    assert L.poco_op_stem_conv(FAKE, pw, NULL, NULL, FAKE, 1, 224, 224, 7, 2, NULL) == ERR_ARG
    assert L.poco_op_stem_conv(FAKE, pw, NULL, NULL, FAKE, 0, 224, 224, 7, 1, NULL) == ERR_ARG


def test_head_kernel_argument_errors(L):
    """The list tests/test_head_kernels_gpu.py runs on device buffers, here with fake pointers: each call is refused with
    POCO_ERR_ARG and a message that names the entry before anything is dereferenced or launched."""
    from tests.test_head_kernels_gpu import bad_calls
    calls = bad_calls(L, FAKE, FAKE)
    assert len(calls) > 40 and {w for w, _ in calls} == {"rot6d_ex", "lc2d_pose_ex", "copy_rows", "broadcast_rows", "nhwc_to_nchw",
                                                         "pack_record", "camera", "mlp_chain"}
    for who, rc in calls:
        assert rc == ERR_ARG, who
    # the message names the entry and what is wrong
    assert L.poco_op_camera(FAKE, 3, FAKE, 1, FAKE, FAKE, NULL, FAKE, FAKE, NULL, FAKE, 1, NULL) == ERR_ARG
    assert "camera" in _msg(L) and "d_center" in _msg(L)
    assert L.poco_op_rot6d_ex(FAKE, 100, FAKE, 216, NULL, 0, 1, NULL) == ERR_ARG and "rot6d_ex" in _msg(L) and "144" in _msg(L)
    layer = (C.c_int * 12)(16, 16, 0, 0, 2, 16, -1, 0, 0, 0, 16, 32)           # input offset 2: no multiple of 4
    w = np.zeros(256, np.float32)
    ptr = (C.c_void_p * 1)(w.ctypes.data)
    assert L.poco_op_mlp_chain(layer, 1, ptr, ptr, None, 0, (C.c_int * 4)(0, 1, 0, 0), 1, (C.c_void_p * 1)(4096), (C.c_longlong * 1)(64), 1,
                               1, 4, NULL) == ERR_ARG
    assert "mlp_chain" in _msg(L) and "layer 0" in _msg(L) and "multiple of 4" in _msg(L)
    rowj = (C.c_int * 11)(3, 0, 0, 16, 0, 16, 16, -1, 0, 0, 8)                 # kind 3
    assert L.poco_op_mlp_chain(None, 0, None, None, rowj, 1, (C.c_int * 4)(0, 0, 0, 1), 1, (C.c_void_p * 1)(4096), (C.c_longlong * 1)(64), 1,
                               1, 4, NULL) == ERR_ARG and "row job 0" in _msg(L)
    assert L.poco_op_mlp_chain(None, 0, None, None, None, 0, (C.c_int * 4)(0, 1, 0, 0), 1, (C.c_void_p * 1)(4096), (C.c_longlong * 1)(64), 1,
                               1, 4, NULL) == ERR_ARG and "stage 0" in _msg(L)


def test_rows_buffer_poisoning_helper():
    """ops.Rows on the CPU: slices round-trip at an odd stride; a write to a guard, another column or a row >= B is noticed."""
    import torch
    from poco_amd import ops
    x = torch.randn(3, 5)
    for fill in ("nan", "poison"):
        w = ops.Rows(3, 7, "cpu", fill, extra_rows=2).put(1, x)
        assert torch.equal(w.get(1, 5), x) and w.untouched([(1, 5)]) and not w.untouched([(1, 4)])
        assert w.guard % 4 == 0 and w.guard >= 64 and w.flat.numel() == 5 * 7 + 2 * w.guard
        assert w.ptr(3).value - w.ptr().value == 12 and w.ptr().value == w.flat.data_ptr() + 4 * w.guard
        for idx in (0, w.flat.numel() - 1, w.guard, w.guard + 3 * 7 + 2):      # guards, column 0 of row 0, a row >= B
            v = ops.Rows(3, 7, "cpu", fill, extra_rows=2).put(1, x)
            v.flat[idx] = 1.0
            assert not v.untouched([(1, 5)])
    assert bool(torch.isnan(ops.Rows(2, 4, "cpu", "poison").mark(0, 4).get(0, 4)).all())


def test_wide_buffer_poisoning_helper():
    """ops.Wide on the CPU: the slice round-trips, a write outside it (a neighbouring channel, either guard band) is noticed."""
    import torch
    from poco_amd import ops
    w = ops.Wide(2, 3, 5, 48, "cpu", "poison")
    x = torch.randn(2, 3, 5, 16)
    w.put(16, x)
    assert torch.equal(w.get(16, 16), x) and w.untouched(16, 16) and not w.untouched(0, 16)
    assert w.guard == 48 * 5 and w.flat.numel() == 2 * 3 * 5 * 48 + 2 * w.guard
    for idx in (0, w.flat.numel() - 1, w.guard):          # front guard, back guard, channel 0 of the body
        v = ops.Wide(2, 3, 5, 48, "cpu", "poison")
        v.flat[idx] = 1.0
        assert not v.untouched(16, 16)
    r = ops.Wide(3, 1, 1, 24, "cpu", "nan")               # rows: offsets in multiples of 4
    y = torch.randn(3, 1, 1, 16)
    r.put(4, y)
    assert torch.equal(r.get(4, 16), y) and bool(torch.isnan(r.flat).sum() == r.flat.numel() - 48)
    assert r.ptr(4).value - r.base().value == 16 and w.ptr(32).value - w.base().value == 4 * 2 * 5 * 16
