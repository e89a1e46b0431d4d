"""GPU: ops.track_stitch (poco_op_track_stitch, csrc/track_stitch.hip) against its float64 numpy restatement tests/stitch_np.py on the
seeded scenes of tests/stitch_scenes.py.  tests/test_stitch_cpu.py checks on the CPU that every scene has decision margins > 1e-9, the
condition under which two fp64 implementations must take the same discrete decisions: here succ, pred, chain and status are EQUAL to
the restatement's.  desc and gain agree within stitch_scenes.TOL = 16 x the rounding floor measured there (float64 against long
double, |difference| / (1 + |value|), NOTEBOOK.md "Track stitching").  Every output lies between guard words that must come back
intact."""
import numpy as np
import pytest
import torch

from poco_amd import ops
from tests import stitch_np, stitch_scenes

pytestmark = pytest.mark.gpu
GUARD = 64
INT_GUARD, INT_UNSET = 0x5A5AA5A5, -77
DISCRETE = ("succ", "pred", "chain", "status")


class Guarded:
    """The six outputs inside allocations with GUARD words before and after each; the body starts as a value the operator never
    writes (every element must be written), the guards as a bit pattern that must survive."""

    def __init__(self, P, Cn, dev):
        self.flat, self.out = {}, {}
        for k, n, shape, dt in (("succ", P, (P,), torch.int32), ("pred", P, (P,), torch.int32), ("chain", P, (P,), torch.int32),
                                ("gain", P, (P,), torch.float64), ("desc", ops.STITCH_DESC * P, (P, ops.STITCH_DESC), torch.float64),
                                ("status", Cn, (Cn,), torch.int32)):
            if dt == torch.int32:
                f = torch.full((n + 2 * GUARD,), INT_GUARD, dtype=dt, device=dev)
                f[GUARD:GUARD + n] = INT_UNSET
            else:
                f = torch.full((n + 2 * GUARD,), 1.5e300, dtype=dt, device=dev)
                f[GUARD:GUARD + n] = -float("inf")
            self.flat[k], self.out[k] = f, f[GUARD:GUARD + n].view(shape)

    def check(self):
        for k, f in self.flat.items():
            n = f.numel() - 2 * GUARD
            edge = torch.cat([f[:GUARD], f[GUARD + n:]]).cpu()
            assert bool((edge == (INT_GUARD if f.dtype == torch.int32 else 1.5e300)).all()), f"{k}: a guard word was written"
            body = f[GUARD:GUARD + n].cpu()
            assert not bool((body == (INT_UNSET if f.dtype == torch.int32 else -float("inf"))).any()), f"{k}: an element was not written"


def run(sc, dev, **over):
    P, Cn = len(sc["frag_offsets"]) - 1, len(sc["clip_offsets"]) - 1
    g = Guarded(P, Cn, dev)
    res = ops.track_stitch(sc["clip_offsets"], sc["frag_offsets"], *(torch.from_numpy(sc[k]).to(dev) for k in ("frames", "boxes", "betas", "var")),
                           **{**sc["params"], **over}, out=g.out)
    torch.cuda.synchronize()
    g.check()
    return {k: v.cpu().numpy() for k, v in res.items()}


def restate(sc, **over):
    return stitch_np.track_stitch(sc["clip_offsets"], sc["frag_offsets"], sc["frames"], sc["boxes"], sc["betas"], sc["var"],
                                  **{**sc["params"], **over})


def worst(got, want):
    return max((float(np.abs((got[k] - want[k]) / (1 + np.abs(want[k]))).max()) if want[k].size else 0.0) for k in ("desc", "gain"))


@pytest.fixture(scope="module")
def want():
    """The restatement on every scene, once."""
    return {name: restate(sc) for name, sc in stitch_scenes.scenes().items()}


@pytest.mark.parametrize("name", list(stitch_scenes.scenes()))
def test_scene_equals_the_restatement(name, want, cuda):
    sc, w = stitch_scenes.scenes()[name], want[name]
    got = run(sc, cuda)
    for k in DISCRETE:
        assert got[k].dtype == np.int32 and np.array_equal(got[k], w[k]), (name, k, got[k].tolist(), w[k].tolist())
    assert got["desc"].shape == w["desc"].shape and got["gain"].dtype == np.float64
    err = worst(got, w)
    print(f"track_stitch {name}: P = {len(got['succ'])}, N = {len(sc['frames'])}, desc and gain within {err:.2e} "
          f"({err / stitch_scenes.FLOOR:.2f} x the floor, 16 allowed)")
    assert err <= stitch_scenes.TOL
    assert np.array_equal(got["gain"] > 0, got["succ"] >= 0)


def test_the_shape_term_changes_the_links(want, cuda):
    """The same boxes and shapes: with the shape term each person continues herself, on motion alone the 3-pixel offsets swap them."""
    on, off = run(stitch_scenes.scenes()["shape_on"], cuda), run(stitch_scenes.scenes()["shape_off"], cuda)
    assert on["succ"].tolist() == [3, 2, -1, -1] and off["succ"].tolist() == [2, 3, -1, -1]
    assert np.array_equal(on["desc"], off["desc"])                               # the descriptors do not depend on the weight


def test_default_scenes_as_clips_of_one_call(want, cuda):
    """Every scene with default parameters becomes a clip of ONE call: a clip's outputs do not depend on its neighbours."""
    sc = stitch_scenes.default_clips()
    got = run(sc, cuda)
    base, succ, pred = 0, [], []
    for n in sc["names"]:
        w = want[n]
        succ.append(np.where(w["succ"] >= 0, w["succ"] + base, -1))
        pred.append(np.where(w["pred"] >= 0, w["pred"] + base, -1))
        base += len(w["succ"])
    assert np.array_equal(got["succ"], np.concatenate(succ)) and np.array_equal(got["pred"], np.concatenate(pred))
    assert np.array_equal(got["chain"], np.concatenate([want[n]["chain"] for n in sc["names"]]))
    assert np.array_equal(got["status"], np.concatenate([want[n]["status"] for n in sc["names"]]))
    joined = {k: np.concatenate([want[n][k] for n in sc["names"]]) for k in ("desc", "gain")}
    assert worst(got, joined) <= stitch_scenes.TOL
    again = run(sc, cuda)
    assert all(np.array_equal(got[k], again[k]) for k in got)                    # bit for bit from run to run


def test_tie_gives_a_valid_optimum(cuda):
    """One tail, two bit-identical heads: either may continue it.  Checked: one link, of the restatement's optimal total."""
    sc = stitch_scenes.tie_scene()
    w, got = restate(sc), run(sc, cuda)
    assert got["status"].tolist() == [0] and got["succ"][0] in (1, 2) and got["succ"][1:].tolist() == [-1, -1]
    head = int(got["succ"][0])
    assert got["pred"].tolist() == [-1] + [0 if i == head else -1 for i in (1, 2)]
    assert sorted(got["chain"].tolist()) == [0, 0, 1] and got["chain"][0] == got["chain"][head] == 0
    assert float(got["gain"].sum()) == pytest.approx(float(w["total"][0]), abs=stitch_scenes.TOL)


def test_a_table_the_kernel_cannot_read_ends_its_clip_with_status_2(cuda):
    """Past ops.track_stitch's checks, through the C ABI: the first clip of `empty_clip` with an EMPTY second fragment.  Its fragments
    get -1, -1, their own chain and gain 0, the unreadable fragment a descriptor of zeros; the other clips are untouched."""
    import ctypes as C
    from poco_amd._lib import check, current_stream, lib
    sc = stitch_scenes.scenes()["empty_clip"]
    w = restate(sc)
    fo = sc["frag_offsets"].copy()
    fo[1] = fo[2]                                                                # fragment 0 takes the rows of both, fragment 1 none
    g = Guarded(3, 3, cuda)
    dev = [torch.from_numpy(a).to(cuda) for a in (sc["clip_offsets"], fo, sc["frames"], sc["boxes"], sc["betas"], sc["var"])]
    scratch = torch.empty(3 * ops.STITCH_MAX_FRAGS, dtype=torch.float64, device=cuda)
    p = lambda t: C.c_void_p(t.data_ptr())                                      # noqa: E731
    check(lib().poco_op_track_stitch(*(p(t) for t in dev), C.c_int64(3), C.c_int64(3), C.c_int64(len(sc["frames"])), 30, 8, C.c_double(0.3),
                                     C.c_double(0.5), C.c_double(1.0), C.c_double(0.05), C.c_double(1.0), p(scratch),
                                     *(p(g.out[k]) for k in ("succ", "pred", "chain", "gain", "desc", "status")), current_stream()),
          "poco_op_track_stitch")
    torch.cuda.synchronize()
    g.check()
    got = {k: v.cpu().numpy() for k, v in g.out.items()}
    assert got["status"].tolist() == [2, 0, 0] and got["succ"].tolist() == [-1, -1, -1] and got["pred"].tolist() == [-1, -1, -1]
    assert got["chain"].tolist() == [0, 1, 0] and got["gain"].tolist() == [0.0, 0.0, 0.0]
    assert (got["desc"][1] == 0).all() and got["desc"][0, 13] == 56
    assert float(np.abs((got["desc"][2] - w["desc"][2]) / (1 + np.abs(w["desc"][2]))).max()) <= stitch_scenes.TOL


def test_device_tables_refusals_and_no_fragments(cuda):
    sc = stitch_scenes.scenes()["empty_clip"]
    rows = [torch.from_numpy(sc[k]).to(cuda) for k in ("frames", "boxes", "betas", "var")]
    a = ops.track_stitch(torch.from_numpy(sc["clip_offsets"]).to(cuda), torch.from_numpy(sc["frag_offsets"]).to(cuda), *rows)
    b = ops.track_stitch(sc["clip_offsets"].tolist(), sc["frag_offsets"].tolist(), *rows)
    assert all(torch.equal(a[k], b[k]) for k in a) and a["succ"].is_cuda and a["status"].tolist() == [0, 0, 0]
    from poco_amd._lib import PocoHipError
    with pytest.raises(PocoHipError, match="fragment 1"):
        ops.track_stitch(None, [0, 30, 30, 76], *rows)
    with pytest.raises(PocoHipError, match="out"):
        ops.track_stitch(sc["clip_offsets"], sc["frag_offsets"], *rows, out={"succ": a["succ"]})
    none = ops.track_stitch([0, 0, 0], [0], *(r[:0] for r in rows))             # two clips without a fragment
    assert none["status"].tolist() == [0, 0] and none["succ"].numel() == 0 and none["desc"].shape == (0, 28)
