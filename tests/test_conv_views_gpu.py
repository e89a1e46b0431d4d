"""Every conv ALG on the operand form the engine uses - channel slices of wider L16 buffers - and with every epilogue form, through
poco_op_conv2d_ex (ops.conv2d_view), against torch CPU conv2d in fp64.

The dense operator test (test_conv_gpu.py) fixes in_cs = Cin, res_cs = out_cs = Cout, offsets 0, act 0 | 1.  The engine calls the
same kernels with strides wider than the conv, non-zero slice offsets, act 2 (sigmoid), act 3 (ReLU from relu_from) and
res_after_act; a wrong slice-row stride or a ReLU on the wrong channels in ONE kernel's epilogue was visible only through a whole
model.  Poisoning (ops.Wide): inputs and residuals sit in NaN-filled buffers (foreign memory that enters the arithmetic turns the
result NaN, even times a zero weight), the output slice starts as NaN (an unwritten element stays NaN) inside a buffer of a bit
pattern that must be bitwise unchanged afterwards (neighbouring channels, one image row of guard band on either side).

Tolerances are the project's, relative to max(1, |ref|max): 2e-5 direct / GEMM kernels (exact fp32 fma chains, only the summation
order differs) and sigmoid outputs, 1e-4 Winograd F(2x2), 2e-4 F(4x4) (test_conv_gpu.py ALG_TOL).
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

TOL = {3: 1e-4, 4: 1e-4, 7: 2e-4, 8: 2e-4, 11: 2e-4, 13: 2e-4}
WINOGRAD = (3, 4, 7, 8, 11, 13)          # refuse act 2 / 3 (conv_launch, conv_wino4*_launch, conv_wino4g_cfg_valid)


def _ref(x, w, scale, shift, stride, res, act, relu_from=0, res_after=0):
    """fp64: conv * scale + shift, residual before or after the activation, act 0 none | 1 ReLU | 2 sigmoid | 3 ReLU from relu_from."""
    y = F.conv2d(torch.from_numpy(x).permute(0, 3, 1, 2).double(), torch.from_numpy(w).double(), stride=stride,
                 padding=(w.shape[2] - 1) // 2)
    y = y * torch.from_numpy(scale).double().view(1, -1, 1, 1) + torch.from_numpy(shift).double().view(1, -1, 1, 1)
    y = y.permute(0, 2, 3, 1)
    r = None if res is None else torch.from_numpy(res).double()
    if r is not None and not res_after:
        y = y + r
    if act == 1:
        y = y.clamp_min(0)
    elif act == 2:
        y = torch.sigmoid(y)
    elif act == 3:
        y = torch.cat([y[..., :relu_from], y[..., relu_from:].clamp_min(0)], -1)
    if r is not None and res_after:
        y = y + r
    return y.numpy()


def _direct_cfg(alg, B, Ho, Wo):
    """ALG 0 / 1 / 2: the small generic tile of test_conv_parity_lds_dma (4 sub-tiles x 1 n-tile per wave, 2 x 2 waves)."""
    R = max(1, min(Ho, 128 // Wo))
    NI = max(1, 128 // (R * Wo)) if R == Ho else 1
    return (4, 1, 2, 2, R, min(NI, B), alg)


def _wino2_cfg(alg, nt, B, H, W):
    """ALG 3 / 4: as test_conv_parity_winograd."""
    cap = 128 if alg == 3 else 64
    TX, Hc = (W + 1) // 2, (H + 1) // 2 * 2
    R = 2
    while R + 2 <= Hc and ((R + 2) // 2) * TX <= cap:
        R += 2
    tiles = (R // 2) * TX
    WM = -(-tiles // 16)
    NI = min(B, max(1, (WM * 16) // tiles)) if R >= H else 1
    return (1, nt, WM, 1 if alg == 3 else 2, R, NI, alg)


def _wino4_cfg(H, W, nt, alg):
    """ALG 7 / 8 (13: the same rectangle with WN = 1): as test_conv_gpu._wino4_cfg."""
    TX, Hc = (W + 3) // 4, (H + 3) // 4 * 4
    R = Hc if (Hc // 4) * TX <= 32 else max(4, 32 // TX * 4)
    NI = max(1, min(32 // ((R // 4) * TX), 1024 // ((R + 2) * (4 * TX + 2)))) if R == Hc else 1
    npos = lambda ni: ni * (R + 2) * (4 * TX + 2)
    lds = lambda ni: 4 * ((npos(ni) + npos(ni) // 8 + 1 + 63) // 64 * 64 + 9 * nt * 64) * 16
    while NI > 1 and (lds(NI) > 160 * 1024 or (npos(NI) + npos(NI) // 8 + 1 + 63) // 64 * 64 > 1024):
        NI -= 1
    if alg == 13:
        return (1, nt, 2, 1, R, NI, 13)
    return (1, nt, 2, 4, R, NI, alg)


def _setups():
    """(id, alg, B, H, W, Cin, Cout, ks, stride, cfg): per ALG two or three of the configurations its dense test uses, on the
    smallest planes at which it still has ragged tiles; Cout = 48 / 112 leave the last n-tile group partly empty; for each
    persistent ALG (2, 4, 7, 8, 13, 14) one B at which its blocks walk more than one item."""
    out = []

    def add(alg, B, H, W, Cin, Cout, ks, stride, cfg):
        out.append(pytest.param((alg, B, H, W, Cin, Cout, ks, stride, cfg), id=f"alg{alg}-{B}x{H}x{W}x{Cin}x{Cout}k{ks}s{stride}-" +
                                "-".join(map(str, cfg[:6]))))

    for alg in (0, 1, 2):
        add(alg, 2, 13, 9, 32, 48, 3, 1, _direct_cfg(alg, 2, 13, 9))
        add(alg, 3, 15, 11, 16, 32, 3, 2, _direct_cfg(alg, 3, 8, 6))
        add(alg, 2, 13, 9, 48, 32, 1, 1, _direct_cfg(alg, 2, 13, 9))
    add(2, 270, 13, 9, 16, 48, 3, 1, _direct_cfg(2, 270, 13, 9))       # 540 tiles > 2 x 256 resident blocks: persistent blocks walk several
    for H, W in ((13, 9), (14, 14)):
        add(3, 2, H, W, 32, 48, 3, 1, _wino2_cfg(3, 1, 2, H, W))
        add(3, 3, H, W, 16, 64, 3, 1, _wino2_cfg(3, 2, 3, H, W))
        add(4, 2, H, W, 32, 48, 3, 1, _wino2_cfg(4, 2, 2, H, W))
        add(4, 3, H, W, 16, 96, 3, 1, _wino2_cfg(4, 3, 3, H, W))
        for alg in (7, 8, 13):
            add(alg, 2, H, W, 32, 48, 3, 1, _wino4_cfg(H, W, 2, alg))
            add(alg, 3, H, W, 16, 96, 3, 1, _wino4_cfg(H, W, 3, alg))
        add(13, 3, H, W, 32, 112, 3, 1, (1, 2, 2, 1, 4, 0, 13))       # flat items, 7 n-tiles
    for alg in (7, 8, 13):
        add(alg, 200, 14, 14, 16, 48, 3, 1, _wino4_cfg(14, 14, 1, alg))   # 100 two-image items x 3 n-groups > 256 blocks
    # ALG 4 is persistent too (conv_wino_launch: at most 256 x per_cu <= 512 blocks, each walks tiles t, t + grid, ...): one image per
    # block x 3 n-groups = 600 tiles -> 2 rounds of 304 blocks, every block's second tile in another image / n-group
    add(4, 200, 14, 14, 16, 48, 3, 1, _wino2_cfg(4, 1, 200, 14, 14))
    for cfg in ((4, 4, 1, 1, 2, 1, 11), (8, 2, 2, 4, 2, 1, 11)):
        add(11, 3, 5, 3, 16, 32, 3, 1, cfg)
        add(11, 2, 7, 7, 32, 48, 3, 1, cfg)
    add(11, 33, 7, 7, 16, 112, 3, 1, (4, 2, 2, 2, 3, 1, 11))             # T = 132 tiles > one 128-tile group
    for cfg in ((7, 2, 2, 4, 3, 1, 6), (4, 4, 1, 4, 2, 1, 6), (7, 4, 2, 2, 1, 1, 9), (8, 2, 1, 1, 1, 1, 9)):
        add(cfg[6], 2, 13, 9, 32, 48, 1, 1, cfg)
        add(cfg[6], 3, 15, 11, 48, 112, 1, 2, cfg)
    for cfg in ((4, 3, 2, 3, 3, 3, 10), (7, 2, 2, 4, 3, 1, 10)):
        add(10, 2, 13, 9, 32, 48, 3, 1, cfg)
        add(10, 3, 15, 11, 16, 112, 3, 2, cfg)
    for cfg in ((7, 4, 2, 1, 2, 1, 14), (4, 2, 8, 1, 3, 3, 14)):
        add(14, 2, 13, 9, 32, 48, 1, 1, cfg)
        add(14, 37, 13, 9, 96, 112, 1, 1, cfg)                            # stream-K: every wave several (tile, K slice) units
    return out


def _run(setup, cuda, *, in_w=False, out_w=None, res="none", act=1, relu_from=0, res_after=0, neg_res=False, vec4=False):
    """One launch of a setup in an operand form; returns nothing, asserts everything.  in_w: input at offset 16 of a buffer 3 x as wide
    (+ 16); out_w: "mid" | "last" = output slice in the middle / at the end of a wider buffer; res: "none" | "dense" | "wide" (a
    slice of a buffer whose stride differs from the output's) | "input" (the input buffer doubles as the residual)."""
    from poco_amd import ops
    alg, B, H, W, Cin, Cout, ks, stride, cfg = setup
    if res == "input":
        Cin = Cout                                        # BasicBlock conv2 form: out += x
        assert stride == 1
    rng = np.random.default_rng(1000 * alg + 31 * B + H + Cin + Cout + stride)
    pad = (ks - 1) // 2
    Ho, Wo = (H + 2 * pad - ks) // stride + 1, (W + 2 * pad - ks) // stride + 1
    x = rng.standard_normal((B, H, W, Cin)).astype(np.float32)
    w = (rng.standard_normal((Cout, Cin, ks, ks)) / np.sqrt(Cin * ks * ks)).astype(np.float32)
    scale = rng.uniform(0.5, 1.5, Cout).astype(np.float32)
    shift = rng.uniform(-0.3, 0.3, Cout).astype(np.float32)   # pre-activation ~ N(0, 1) + shift: about half of it negative
    unit = 4 if vec4 else 16
    kw = dict(act=act, relu_from=relu_from, res_after_act=res_after, cfg=cfg)
    if in_w:
        kw.update(in_cs=3 * Cin + 16, in_co=32 if alg == 12 else unit)     # (ALG 12 takes input offsets in multiples of 32)
    if out_w == "mid":
        kw.update(out_cs=Cout + 48, out_co=unit + (16 if not vec4 else 4))
    elif out_w == "last":
        kw.update(out_cs=Cout + 32, out_co=32)
    r = None
    if res == "input":
        r, rarg = x, "input"
    elif res != "none":
        r = rng.standard_normal((B, Ho, Wo, Cout)).astype(np.float32)
        if neg_res:
            r = -np.abs(r) - 0.25                          # negative-going: ReLU-then-add differs from add-then-ReLU everywhere
        rarg = torch.from_numpy(r).to(cuda)
        if res == "wide":
            kw.update(res_cs=kw.get("out_cs", Cout) + 64, res_co=2 * unit)
    else:
        rarg = None
    xd = torch.from_numpy(x).to(cuda)
    if alg in WINOGRAD and act in (2, 3):
        # refused for THIS reason (the launchers' own messages), never something else computed silently
        with pytest.raises(RuntimeError, match=r"activation must be none or ReLU|no activation or ReLU only|activation none\|ReLU"):
            ops.conv2d_view(xd, w, scale, shift, stride, rarg, **kw)
        return
    out, wide = ops.conv2d_view(xd, w, scale, shift, stride, rarg, **kw)
    ref = _ref(x, w, scale, shift, stride, r, act, relu_from, res_after)
    out = out.cpu().numpy()
    assert out.shape == ref.shape
    nan = int(np.isnan(out).sum())
    assert nan == 0, f"{nan} NaN of {out.size}: unwritten elements, or foreign (NaN-poisoned) memory in the arithmetic"
    assert wide.untouched(kw.get("out_co", 0), Cout), "the kernel wrote outside its output slice (neighbour channels / guard band)"
    err = np.abs(out - ref).max() / max(1.0, np.abs(ref).max())
    print(f"alg {alg} rel err {err:.2e}")
    assert err <= (2e-5 if act == 2 else TOL.get(alg, 2e-5)), err


FORMS = {
    "in-slice": dict(in_w=True),                                              # 1
    "out-slice-mid": dict(out_w="mid"),                                       # 2
    "out-slice-last": dict(out_w="last"),                                     # 2, as the last slice of the buffer
    "res-slice": dict(res="wide"),                                            # 3: res_cs != out_cs
    "input-is-residual": dict(res="input"),                                   # 4
    "all-slices": dict(in_w=True, out_w="mid", res="wide"),                   # 5
    "sigmoid": dict(in_w=True, out_w="mid", act=2),
    "relu-from-16": dict(in_w=True, out_w="mid", res="wide", act=3, relu_from=16),
    "relu-from-last": dict(in_w=True, out_w="mid", act=3, relu_from=-16),    # Cout - 16
    "res-after-relu": dict(in_w=True, out_w="mid", res="wide", act=1, res_after=1, neg_res=True),
}


@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("setup", _setups())
def test_conv_view(setup, form, cuda):
    kw = dict(FORMS[form])
    if form == "input-is-residual" and setup[7] != 1:
        # no such operand exists at stride 2 (the residual has the output's plane): the form is run on this setup's stride-1 twin
        setup = setup[:7] + (1,) + setup[8:]
        if setup[0] in (0, 1, 2):
            setup = setup[:8] + (_direct_cfg(setup[0], setup[1], setup[2], setup[3]),)
    if kw.get("relu_from", 0) < 0:
        kw["relu_from"] = setup[5] - 16
    _run(setup, cuda, **kw)


# ---- ALG 5 on rows (H = W = 1): the CLIFF regressor's state vector uses offsets that are multiples of 4, not of 16 ---------------
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("unit", [4, 16])
@pytest.mark.parametrize("wm", [1, 4])
@pytest.mark.parametrize("B", [1, 37])
def test_linear_rows_view(B, wm, unit, form, cuda):
    kw = dict(FORMS[form])
    setup = (5, B, 1, 1, 48, 32 if form == "input-is-residual" else 64, 1, 1, (1, 1, wm, 1, 1, 1, 5))
    if kw.get("relu_from", 0) < 0:
        kw["relu_from"] = setup[5] - 16
    _run(setup, cuda, vec4=(unit == 4), **kw)


def test_conv_view_split_f16_experiment(cuda):
    from tests import util as _u
    if not _u.has_experiments():
        pytest.skip("experiment build only (python -m poco_amd.build --experiments)")
    for form in FORMS:
        kw = dict(FORMS[form])
        setup = (12, 2, 13, 9, 32, 48, 1, 1, (4, 2, 1, 4, 2, 1, 12))
        if kw.get("relu_from", 0) < 0:
            kw["relu_from"] = 32
        _run(setup, cuda, **kw)


def test_view_equals_dense_acceptance(cuda):
    """A view form whose dense counterpart the library accepts with the same configuration is accepted too: the heuristic
    configuration (cfg = None) on slices of every kind."""
    _run((0, 2, 13, 9, 32, 48, 3, 1, None), cuda, in_w=True, out_w="mid", res="wide")
    _run((5, 3, 1, 1, 48, 64, 1, 1, None), cuda, in_w=True, out_w="last", res="wide", vec4=True)


@pytest.mark.parametrize("bad", ["stride-too-small", "relu-from-odd", "relu-from-large", "act-4", "vec-offset-2"])
def test_conv_view_argument_errors(bad, cuda):
    from poco_amd import ops
    x = torch.zeros(1, 4, 4, 16, device=cuda)
    w = np.zeros((32, 16, 1, 1), np.float32)
    kw = {"stride-too-small": dict(out_cs=32, out_co=16),
          "relu-from-odd": dict(act=3, relu_from=8), "relu-from-large": dict(act=3, relu_from=48), "act-4": dict(act=4)}.get(bad)
    if bad == "vec-offset-2":
        x, kw = torch.zeros(2, 1, 1, 16, device=cuda), dict(in_cs=32, in_co=2)
    with pytest.raises(RuntimeError):
        ops.conv2d_view(x, w, **kw)
