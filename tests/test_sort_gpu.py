"""GPU: ops.sort_tracks (poco_op_sort_tracks, csrc/sort_tracks.hip) against its float64 numpy restatement tests/sort_np.py on the
seeded scenes of tests/sort_scenes.py.  tests/test_sort_cpu.py checks on the CPU that every scene has decision margins > 1e-9, the
condition under which two fp64 implementations must take the same discrete decisions: here tracker, id, count and status are EQUAL to
the restatement's.  The filtered boxes agree within sort_scenes.BOX_TOL = 16 x the rounding floor measured there (float64 against
long double, NOTEBOOK.md "SORT on the device").  Every output lies between guard words that must come back intact."""
import numpy as np
import pytest
import torch

from poco_amd import ops
from tests import sort_np, sort_scenes

pytestmark = pytest.mark.gpu
GUARD = 64
INT_GUARD, INT_UNSET = 0x5A5AA5A5, -77


class Guarded:
    """The five outputs inside allocations with GUARD words before and after each; the body starts as a value the operator never
    writes (every element must be written), the guards as a bit pattern that must survive."""

    def __init__(self, N, Cn, dev):
        self.flat, self.out = {}, {}
        for k, n, shape, dt in (("tracker", N, (N,), torch.int32), ("id", N, (N,), torch.int32), ("box", 4 * N, (N, 4), torch.float64),
                                ("count", Cn, (Cn,), torch.int32), ("status", Cn, (Cn,), torch.int32)):
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
    N, Cn = len(sc["dets"]), len(sc["clip_offsets"]) - 1
    g = Guarded(N, Cn, dev)
    res = ops.sort_tracks(torch.from_numpy(sc["dets"]).to(dev), sc["frame_offsets"], sc["clip_offsets"], **{**sc["params"], **over}, out=g.out)
    torch.cuda.synchronize()
    g.check()
    return {k: v.cpu().numpy() for k, v in res.items()}


@pytest.fixture(scope="module")
def want():
    """The restatement on every scene, once."""
    return {name: sort_np.sort_tracks(sc["dets"], sc["frame_offsets"], sc["clip_offsets"], **sc["params"])
            for name, sc in sort_scenes.scenes().items()}


@pytest.mark.parametrize("name", list(sort_scenes.scenes()))
def test_scene_equals_the_restatement(name, want, cuda):
    sc, w = sort_scenes.scenes()[name], want[name]
    got = run(sc, cuda)
    for k in ("status", "count", "tracker", "id"):
        assert got[k].dtype == np.int32 and np.array_equal(got[k], w[k]), (name, k, got[k].tolist(), w[k].tolist())
    ok = np.isfinite(w["box"]).all(1)
    assert np.array_equal(np.isnan(got["box"]).all(1), ~ok) and np.array_equal(np.isfinite(got["box"]).all(1), ok)
    rel = float(np.abs((got["box"][ok] - w["box"][ok]) / w["box"][ok]).max()) if ok.any() else 0.0
    print(f"sort_tracks {name}: N = {len(sc['dets'])}, boxes within {rel:.2e} relative ({rel / sort_scenes.BOX_FLOOR:.2f} x the floor, "
          f"16 allowed)")
    assert rel <= sort_scenes.BOX_TOL
    if name == "overflow":                      # max_trackers = 2 with three people: status 1, -1 from that frame on, the next clip untouched
        assert got["status"].tolist() == [1, 0] and (got["tracker"][4:16] == -1).all() and (got["id"][4:16] == -1).all()
        assert (got["tracker"][:4] >= 0).all() and (got["tracker"][16:] == 0).all()


def test_all_scenes_as_clips_of_one_call(want, cuda):
    """Every scene with SORT's default parameters becomes a clip of ONE call: a clip's outputs do not depend on its neighbours."""
    names = [n for n, sc in sort_scenes.scenes().items() if not sc["params"]]
    dets, fo, co = [], [0], [0]
    for n in names:
        sc = sort_scenes.scenes()[n]
        base_f = len(fo) - 1
        fo.extend((sc["frame_offsets"][1:] + sum(len(d) for d in dets)).tolist())
        co.extend((sc["clip_offsets"][1:] + base_f).tolist())
        dets.append(sc["dets"])
    got = run({"dets": np.concatenate(dets), "frame_offsets": np.asarray(fo, np.int32), "clip_offsets": np.asarray(co, np.int32), "params": {}}, cuda)
    for k in ("tracker", "id"):
        assert np.array_equal(got[k], np.concatenate([want[n][k] for n in names])), k
    for k in ("count", "status"):
        assert np.array_equal(got[k], np.concatenate([want[n][k] for n in names])), k
    w = np.concatenate([want[n]["box"] for n in names])
    assert float(np.abs((got["box"] - w) / w).max()) <= sort_scenes.BOX_TOL
    again = run({"dets": np.concatenate(dets), "frame_offsets": np.asarray(fo, np.int32), "clip_offsets": np.asarray(co, np.int32), "params": {}}, cuda)
    assert all(np.array_equal(got[k], again[k]) for k in got)                  # bit for bit from run to run


def test_tie_gives_a_valid_optimum(cuda):
    """Two bit-identical detections over one tracker: either may take it.  Checked: each frame's matching is one-to-one, reaches the
    restatement's optimal total, and the ids are a valid outcome (one of the twins continues tracker 0, the other is born as 1)."""
    sc = sort_scenes.tie_scene()
    w = sort_np.sort_tracks(sc["dets"], sc["frame_offsets"], sc["clip_offsets"], **sc["params"])
    got = run(sc, cuda)
    assert got["status"].tolist() == [0] and got["count"].tolist() == [2]
    assert got["tracker"][:2].tolist() == [0, 0] and sorted(got["tracker"][2:4].tolist()) == [0, 1]
    assert np.array_equal(got["id"], got["tracker"])                             # min_hits = 0: everything is emitted
    # the total of frame 2: one pair of IoU 1 (the boxes are the tracker's own), as the restatement's
    assert w["total"][2] == pytest.approx(1.0, abs=1e-9) and (got["tracker"][2:4] == 0).sum() == 1
    assert got["tracker"][4] in (0, 1)                                           # frame 3: both trackers sit on the box


def test_device_offsets_and_refusals(cuda):
    sc = sort_scenes.scenes()["ragged"]
    dev_dets = torch.from_numpy(sc["dets"]).to(cuda)
    a = ops.sort_tracks(dev_dets, torch.from_numpy(sc["frame_offsets"]).to(cuda), torch.from_numpy(sc["clip_offsets"]).to(cuda))
    b = ops.sort_tracks(dev_dets, sc["frame_offsets"].tolist(), sc["clip_offsets"].tolist())
    assert all(torch.equal(a[k], b[k]) for k in a) and a["tracker"].is_cuda
    from poco_amd._lib import PocoHipError
    with pytest.raises(PocoHipError, match="frame 2"):
        ops.sort_tracks(dev_dets, [0, 1, 6, 3, 12])
    with pytest.raises(PocoHipError, match="out"):
        ops.sort_tracks(dev_dets, sc["frame_offsets"], sc["clip_offsets"], out={"tracker": a["tracker"]})
    empty = ops.sort_tracks(torch.zeros((0, 4), dtype=torch.float64, device=cuda), [0, 0, 0], [0, 2, 2])   # frames without people, a clip without frames
    assert empty["count"].tolist() == [0, 0] and empty["status"].tolist() == [0, 0] and empty["tracker"].numel() == 0
