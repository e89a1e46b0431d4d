"""GPU: ops.select_regressor (poco_op_select_regressor, csrc/select_regressor.hip) against its float64 restatement
tests/select_np.py.  Every output is compared bit for bit: the operator is a decision plus copies.

Rows 1, 2, 3, 64, 65 and 130: one block, more rows than a wave's ballot, and at 130 rows a second pass of the 128-thread
compaction block with a carried base; the grid cap (1024 blocks) is above 130, so one call per mode forces it to 3 blocks.  Payload widths 1, 3, 15, 98
and 20670: widths 1, 3 and 15 put rows off 8- and 16-byte alignment, and the destination of payload p in case c starts
(c + p) % 4 floats into its buffer, so that each width is copied on the 16-byte path (source and destination at the same offset
in a 16-byte line), the 8-byte path and the 4-byte path.  The sweep: both modes, the four kind pairs, kinematic on and off, scale 1
and 0.5.  Row t has pattern (t + 2) % 8 of PATTERNS (rows 128 and 129 are mixed and tied); the two models' pose and payload words differ in every word (model 0 in
[0, 0.9), model 1 in [1, 1.9)); the var words differ except where a tie at scale 1 needs equal values.  Inputs lie in NaN-filled
ops.Rows buffers, outputs between poisoned guard bands with NaN where the kernel must write."""
import itertools

import numpy as np
import pytest
import torch

from poco_amd import ops
from tests import select_np as snp

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 3, 64, 65, 130)
BMAX = max(SIZES)
WIDTHS = (1, 3, 15, 98, 20670)
THR = 0.40
CASES = list(itertools.product(((0, 0), (0, 1), (1, 0), (1, 1)), (False, True), (1.0, 0.5)))       # (kinds, kinematic, scale)
PATTERNS = {0: "model 1 three times as uncertain: model 0 at both scales", 1: "model 1 a quarter as uncertain: model 1",
            2: "the root from model 0, its three children from model 1, whatever the scale and the accumulation: mixed in joint mode", 3: "equal values: ties at scale 1", 4: "model 1 exactly twice: ties at scale 0.5",
            5: "NaN at joint 12 of model 0 / at the root of model 1, in turn", 6: "model 0's root over both thresholds: its score is 1",
            7: "independent draws, model 1's root over 2 thr"}
NAN_BITS = 0x7FC00000


def _material():
    r = np.random.default_rng(25)
    B = BMAX
    v0 = r.uniform(0.01, 0.04, (B, 24)).astype(np.float32)                       # nine accumulated joints stay below thr
    v1 = r.uniform(0.01, 0.04, (B, 24)).astype(np.float32)
    pat = (np.arange(B) + 2) % 8
    v1[pat == 0] = 3 * v0[pat == 0]
    v1[pat == 1] = v0[pat == 1] / 4
    two = pat == 2
    v0[two, 0], v1[two, 0], v1[two, 1:4] = 0.005, 0.02, 0.001                    # 0.5 * 0.02 > 0.005; 0.02 + 0.001 < 0.005 + v0[1..3]
    v0[two, 1:4] = r.uniform(0.03, 0.04, (int(two.sum()), 3)).astype(np.float32)
    v1[pat == 3] = v0[pat == 3]
    v1[pat == 4] = 2 * v0[pat == 4]
    five = np.nonzero(pat == 5)[0]
    v0[five[0::2], 12] = np.nan
    v1[five[1::2], 0] = np.nan
    v0[pat == 6, 0] = 0.9
    v1[pat == 7, 0] = 0.85
    pose0, pose1 = r.uniform(0, 0.9, (B, 24, 3, 3)).astype(np.float32), r.uniform(1, 1.9, (B, 24, 3, 3)).astype(np.float32)
    pay = [(r.uniform(0, 0.9, (B, w)).astype(np.float32), r.uniform(1, 1.9, (B, w)).astype(np.float32)) for w in WIDTHS]
    return dict(pose0=pose0, var0=v0, pose1=pose1, var1=v1, pay=pay)


@pytest.fixture(scope="module")
def data():
    return _material()


_REF, _DEV = {}, {}


def _ref(data, mode, case):
    """The restatement on all BMAX rows, once per case: rows are independent, so the first B rows are the reference of a B-row call."""
    key = (mode, case)
    if key not in _REF:
        (k0, k1), kin, scale = case
        _REF[key] = snp.select(data["pose0"], data["var0"], k0, data["pose1"], data["var1"], k1, kin, THR, scale, mode, data["pay"])
    return _REF[key]


def _inputs(data, B, dev):
    """The first B rows in NaN-filled Rows buffers of exactly B rows, once per B."""
    if B not in _DEV:
        up = lambda a, w: ops.Rows(B, w, dev, "nan").put(0, torch.from_numpy(np.ascontiguousarray(a[:B])).to(dev))   # noqa: E731
        _DEV[B] = dict(pose0=up(data["pose0"], 216), pose1=up(data["pose1"], 216), var0=up(data["var0"], 24), var1=up(data["var1"], 24),
                       pay=[(up(a, w), up(b, w)) for (a, b), w in zip(data["pay"], WIDTHS)])
    return _DEV[B]


class _Out:
    """`words` 32-bit words the kernel must write (NaN on entry) starting `shift` floats into a poisoned Rows buffer; viewed as
    `dtype` [shape].  nbytes < 4 * words: the bytes behind the view must keep their NaN pattern too."""

    def __init__(self, shape, dtype, dev, shift=0):
        self.nbytes = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
        self.words, self.shift = (self.nbytes + 3) // 4, shift
        self.rows = ops.Rows(1, self.words + shift + 3, dev, "poison").mark(shift, self.words)
        self.flat = self.rows.body.view(-1)[shift:shift + self.words]
        self.t = self.flat.view(torch.uint8)[:self.nbytes].view(dtype).view(shape)

    def intact(self):
        tail = self.flat.view(torch.uint8)[self.nbytes:].cpu().numpy()
        want = np.frombuffer(np.uint32(NAN_BITS).tobytes(), np.uint8)[self.nbytes % 4:] if self.nbytes % 4 else tail
        return self.rows.untouched([(self.shift, self.words)]) and np.array_equal(tail, want)


def _call(dv, B, mode, case, ci, dev, max_blocks=0):
    (k0, k1), kin, scale = case
    o = {"pose": _Out((B, 24, 3, 3), torch.float32, dev), "var": _Out((B, 24), torch.float32, dev), "choice": _Out((B, 24), torch.uint8, dev),
         "score": _Out((B, 2), torch.float32, dev), "mixed": _Out((B,), torch.uint8, dev), "rows": _Out((B,), torch.int32, dev),
         "count": _Out((1,), torch.int32, dev)}
    po = [_Out((B, w), torch.float32, dev, shift=(ci + p) % 4) for p, w in enumerate(WIDTHS)]
    out = {k: v.t for k, v in o.items()}
    out["payloads"] = [v.t for v in po]
    ops.select_regressor(dv["pose0"].body[:B].view(B, 24, 3, 3), dv["var0"].body[:B], k0, dv["pose1"].body[:B].view(B, 24, 3, 3),
                         dv["var1"].body[:B], k1, [(a.body[:B], b.body[:B]) for a, b in dv["pay"]], kinematic=kin, thr=THR, scale=scale,
                         mode=mode, rows=True, out=out, max_blocks=max_blocks)
    torch.cuda.synchronize()
    for name, v in list(o.items()) + [(f"payload {w}", v) for w, v in zip(WIDTHS, po)]:
        assert v.intact(), (name, B, mode, case)
    got = {k: v.cpu().numpy() for k, v in out.items() if k != "payloads"}
    got["payloads"] = [v.cpu().numpy() for v in out["payloads"]]
    return got


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _compare(got, ref, B, what):
    for k in ("pose", "var", "choice", "score", "mixed"):
        assert np.array_equal(_bits(got[k]), _bits(ref[k][:B])), (k, what)
    for w, g, r in zip(WIDTHS, got["payloads"], ref["payloads"]):
        assert np.array_equal(_bits(g), _bits(r[:B])), (f"payload of width {w}", what)
    rows = ref["rows"][ref["rows"] < B]
    n = int(got["count"][0])
    assert n == len(rows) == int(ref["mixed"][:B].sum()) and np.array_equal(got["rows"][:n], rows), what
    assert (got["rows"][n:].view(np.uint32) == NAN_BITS).all(), what               # the rest of the list is left alone


def test_the_material_holds_every_decision_pattern(data):
    """Without these the comparisons below show nothing."""
    assert np.isnan(data["var0"]).any() and np.isnan(data["var1"]).any()
    assert not (_bits(data["pose0"]) == _bits(data["pose1"])).any()
    assert not any((_bits(a) == _bits(b)).any() for a, b in data["pay"])
    assert ((_bits(data["var0"]) == _bits(data["var1"])) == ((np.arange(BMAX) + 2) % 8 == 3)[:, None]).all()
    for mode, case in itertools.product((0, 1), CASES):
        (k0, k1), kin, scale = case
        ref = _ref(data, mode, case)
        c = ref["choice"]
        assert (c == 0).all(1).any() and (c == 1).all(1).any(), (mode, case)          # rows all from model 0, rows all from model 1
        assert ref["mixed"].any() == (mode == 1), (mode, case)                        # mixed rows: in joint mode, never in crop mode
        rows = ref["rows"]
        assert len(rows) == ref["mixed"].sum()
        if mode == 1:                                                                 # in every wave and in the second pass of the compaction
            assert (rows < 64).any() and ((rows >= 64) & (rows < 128)).any() and (rows >= 128).any(), (mode, case)
        u0, u1 = ref["u"][0].astype(np.float64), ref["u"][1].astype(np.float64)
        assert (scale * u1 == u0).any(), (mode, case)                                 # exact ties between the joints
        s = ref["score"]
        if k0 == k1:
            assert (s[:, 0] == s[:, 1]).any(), (mode, case)                           # ... and between the crop scores
        assert (s.view(np.uint32) == NAN_BITS).any() and (s == 1.0).any(), (mode, case)
        if mode == 1:
            assert not c[np.isnan(u0) | np.isnan(u1)].any()                           # a NaN entry stays with model 0
        else:
            assert not c[np.isnan(s).any(1)].any()


@pytest.mark.parametrize("mode", [0, 1], ids=["crop", "joint"])
@pytest.mark.parametrize("B", SIZES)
def test_operator_matches_the_restatement_bit_for_bit(data, B, mode, cuda):
    dv = _inputs(data, B, cuda)
    for ci, case in enumerate(CASES):
        _compare(_call(dv, B, mode, case, ci, cuda), _ref(data, mode, case), B, (B, mode, case))


@pytest.mark.parametrize("mode", [0, 1], ids=["crop", "joint"])
def test_the_result_does_not_depend_on_the_grid(data, mode, cuda):
    """130 rows on 3 blocks (the grid-stride loop takes 44 turns), and 65 rows submitted one at a time, against the same bits."""
    case = ((0, 1), True, 0.5)
    ci = CASES.index(case)
    ref = _ref(data, mode, case)
    _compare(_call(_inputs(data, BMAX, cuda), BMAX, mode, case, ci, cuda, max_blocks=3), ref, BMAX, "3 blocks")
    B = 65
    dv = _inputs(data, B, cuda)
    (k0, k1), kin, scale = case
    keys = ("pose", "var", "choice", "score", "mixed")
    parts = []
    for t in range(B):
        row = lambda w: w.body[t:t + 1]                                             # noqa: E731
        parts.append(ops.select_regressor(row(dv["pose0"]).view(1, 24, 3, 3), row(dv["var0"]), k0, row(dv["pose1"]).view(1, 24, 3, 3),
                                          row(dv["var1"]), k1, [(row(a), row(b)) for a, b in dv["pay"]], kinematic=kin, thr=THR,
                                          scale=scale, mode=mode, rows=True))
    got = {k: torch.cat([p[k] for p in parts]).cpu().numpy() for k in keys}
    got["payloads"] = [torch.cat([p["payloads"][i] for p in parts]).cpu().numpy() for i in range(len(WIDTHS))]
    counts = np.array([int(p["count"].item()) for p in parts])
    assert np.array_equal(counts, ref["mixed"][:B]) and all(int(p["rows"][0]) == 0 for p, c in zip(parts, counts) if c)
    for k in keys:
        assert np.array_equal(_bits(got[k]), _bits(ref[k][:B])), k
    for w, g, r in zip(WIDTHS, got["payloads"], ref["payloads"]):
        assert np.array_equal(_bits(g), _bits(r[:B])), w


def test_wrapper_refuses_other_shapes(cuda):
    z = lambda *s: torch.zeros(*s, device=cuda)                                     # noqa: E731
    good = dict(pose0=z(2, 24, 3, 3), var0=z(2, 24), kind0=1, pose1=z(2, 24, 3, 3), var1=z(2, 24), kind1=0)
    for kw in (dict(var0=z(2, 24, 3)), dict(var1=z(2, 24, 3, 3)), dict(var0=z(2, 23)), dict(pose1=z(3, 24, 3, 3)), dict(kind0=2),
               dict(mode="frame"), dict(scale=0.0), dict(scale=float("nan")), dict(payloads=[(z(2, 3), z(2, 4))]),
               dict(payloads=[(z(2, 3), z(2, 3))] * 9), dict(payloads=[(z(3, 3), z(3, 3))])):
        with pytest.raises(ops.PocoHipError, match="select_regressor"):
            ops.select_regressor(**{**good, **kw})
