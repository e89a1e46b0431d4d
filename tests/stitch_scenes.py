"""Seeded scenes for the track stitcher (tests/test_stitch_cpu.py checks their decision margins, tests/test_stitch_gpu.py runs the
operator on them): the smallest shapes at which csrc/track_stitch.hip can still go wrong.  A scene is dict(clip_offsets int32 [C+1],
frag_offsets int32 [P+1], frames int32 [N], boxes float64 [N,4], betas float32 [N,10], var float32 [N,24], params).  scenes() is
computed once and must be left unchanged by its readers.

FLOOR is the rounding floor of `desc` and `gain`: the largest |float64 - long double| / (1 + |long double|) of tests/stitch_np.py
over all scenes, measured by tests/test_stitch_cpu.py (NOTEBOOK.md "Track stitching"); TOL = 16 x FLOOR is what the GPU test allows,
the project's rule from DESIGN.md section 32."""
import functools

import numpy as np

FLOOR = 8.83e-16
TOL = 16 * FLOOR


class Person:
    """A straight walk: centre (x0 + vx f, y0 + vy f), height h0 + vh f, width half of it; a body shape of her own; boxes with
    `jitter` pixels of noise."""

    def __init__(self, rng, x0, y0, vx=0.0, vy=0.0, h0=80.0, vh=0.0, jitter=0.1, betas=None):
        self.rng, self.p, self.jitter = rng, (x0, y0, vx, vy, h0, vh), jitter
        self.betas = rng.normal(0.0, 1.0, 10) if betas is None else np.asarray(betas, np.float64)

    def rows(self, frames, dx=0.0):
        x0, y0, vx, vy, h0, vh = self.p
        f = np.asarray(frames, np.float64)
        h = h0 + vh * f
        box = np.stack([x0 + vx * f + dx, y0 + vy * f, 0.5 * h, h], 1) + self.jitter * self.rng.normal(0.0, 1.0, (len(f), 4))
        betas = (self.betas[None] + 0.02 * self.rng.normal(0.0, 1.0, (len(f), 10))).astype(np.float32)
        var = (0.1 + 0.05 * self.rng.random((len(f), 24))).astype(np.float32)
        return np.asarray(frames, np.int32), box, betas, var


def pack(clips, **params):
    """clips: a list of lists of fragments (frames, boxes, betas, var)."""
    co, fo, parts = [0], [0], []
    for frags in clips:
        for fr in frags:
            parts.append(fr)
            fo.append(fo[-1] + len(fr[0]))
        co.append(co[-1] + len(frags))
    cat = lambda i, dt, w: (np.concatenate([p[i] for p in parts]).astype(dt) if parts else np.zeros((0,) + w, dt))   # noqa: E731
    return {"clip_offsets": np.asarray(co, np.int32), "frag_offsets": np.asarray(fo, np.int32), "frames": cat(0, np.int32, ()),
            "boxes": np.ascontiguousarray(cat(1, np.float64, (4,))), "betas": np.ascontiguousarray(cat(2, np.float32, (10,))),
            "var": np.ascontiguousarray(cat(3, np.float32, (24,))), "params": params}


def _two(rng, T, gap, **params):
    """One walker seen for T frames, hidden for `gap` frames (D = gap + 1), seen for T frames again."""
    a = Person(rng, 100.0, 120.0, 2.0, 0.5, 80.0, 0.1)
    return pack([[a.rows(range(T)), a.rows(range(T + gap, 2 * T + gap))]], **params)


@functools.lru_cache(maxsize=None)
def scenes() -> dict:
    r = np.random.default_rng(36)
    out = {}
    out["single"] = pack([[Person(r, 50.0, 60.0, 1.0).rows(range(12))]])
    a, b = Person(r, 100.0, 100.0, 3.0, 0.0), Person(r, 400.0, 200.0, -1.0, 1.0)
    out["empty_clip"] = pack([[a.rows(range(30)), a.rows(range(34, 60))], [], [b.rows(range(20))]])
    out["gap_1"] = _two(r, 20, 0)
    out["gap_edge"] = _two(r, 20, 4, max_gap=4)                                  # D = 5 = max_gap + 1: linked
    out["gap_over"] = _two(r, 20, 5, max_gap=4)                                  # D = 6 = max_gap + 2: not linked
    still = Person(r, 300.0, 150.0)
    out["short"] = pack([[still.rows([7]), still.rows([10, 12]), still.rows([3])]])          # T = 1, 2, 1: the degenerate fits
    out["fit_1"] = _two(r, 40, 3, fit_len=1, motion_tol=2.0)                     # no velocity: the walk itself is the mismatch
    out["fit_32"] = _two(r, 40, 3, fit_len=32)
    for T in (63, 64, 65, 1000):
        out[f"rows_{T}"] = _two(r, T, 6)
    # two people cross while both are hidden: the last seen positions would swap them, the extrapolated motion does not
    shape = r.normal(0.0, 1.0, 10)
    a, b = Person(r, 100.0, 100.0, 4.0, 0.0, betas=shape), Person(r, 300.0, 130.0, -4.0, 0.0, betas=shape)
    out["crossing"] = pack([[a.rows(range(20)), b.rows(range(20)), b.rows(range(26, 46)), a.rows(range(26, 46))]])
    # nearly the same boxes for both people: the motion (a 3-pixel offset that swaps sides) prefers the wrong pairing, the shape decides
    a, b = Person(r, 200.0, 150.0, 1.0, 0.0, jitter=0.0), Person(r, 200.0, 150.0, 1.0, 0.0, jitter=0.0)
    frs = [a.rows(range(20), dx=3.0), b.rows(range(20)), b.rows(range(24, 44)), a.rows(range(24, 44), dx=-3.0)]
    out["shape_on"] = pack([frs], motion_tol=0.2)
    out["shape_off"] = pack([frs], motion_tol=0.2, shape_w=0.0)
    a = Person(r, 80.0, 90.0, 1.5, 0.25)
    out["chain3"] = pack([[a.rows(range(40, 60)), a.rows(range(0, 15)), a.rows(range(18, 37))]])   # listed out of time order
    a, b = Person(r, 100.0, 100.0, 1.0), Person(r, 110.0, 100.0, 1.0)
    out["overlap"] = pack([[a.rows(range(0, 30)), b.rows(range(20, 50))]])                        # D < 1 both ways: never linked
    # two tails, two heads, motion alone (c = distance / 16): taking the best pair first (0 -> 2) leaves 1 -> 3 gated out; the optimum
    # is 0 -> 3 with 1 -> 2
    mk = lambda y, fr: Person(r, 100.0, y, jitter=0.0, betas=shape).rows(fr)                      # noqa: E731
    out["greedy"] = pack([[mk(100.0, range(10)), mk(120.0, range(10)), mk(108.0, range(13, 23)), mk(90.0, range(13, 23))]],
                         motion_tol=0.1, shape_w=0.0)
    # one row the model does not believe at all (var = 1e6) with a wild shape: it must not move the mean shape
    a = Person(r, 150.0, 150.0, 1.0)
    f0, f1 = a.rows(range(20)), a.rows(range(25, 45))
    f0[2][7] = 5.0
    f0[3][7] = 1e6
    out["outlier_var"] = pack([[f0, f1]])
    # 128 people on a grid, each seen for 2 frames, hidden for 2, seen for 2: 256 fragments of 2 rows in one clip
    grid = [Person(r, 100.0 + 150.0 * (i % 16), 100.0 + 150.0 * (i // 16), 1.0, 0.0, 60.0) for i in range(128)]
    out["crowd256"] = pack([[g.rows([0, 1]) for g in grid] + [g.rows([4, 5]) for g in reversed(grid)]])
    return out


def tie_scene() -> dict:
    """One tail and two bit-identical heads: either may continue it.  Checked for validity and the optimal total only."""
    r = np.random.default_rng(37)
    a = Person(r, 100.0, 100.0, jitter=0.0)
    head = a.rows(range(13, 23))
    return pack([[a.rows(range(10)), head, tuple(np.array(x) for x in head)]])


def default_clips() -> dict:
    """Every scene with default parameters as a clip of ONE call, and the names in order."""
    names = [n for n, sc in scenes().items() if not sc["params"]]
    co, fo, rows = [0], [0], {k: [] for k in ("frames", "boxes", "betas", "var")}
    for n in names:
        sc = scenes()[n]
        co.extend((sc["clip_offsets"][1:] + (len(fo) - 1)).tolist())
        fo.extend((sc["frag_offsets"][1:] + fo[-1]).tolist())
        for k in rows:
            rows[k].append(sc[k])
    return {"names": names, "clip_offsets": np.asarray(co, np.int32), "frag_offsets": np.asarray(fo, np.int32),
            **{k: np.concatenate(v) for k, v in rows.items()}, "params": {}}
