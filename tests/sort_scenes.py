"""The seeded scenes of the SORT tests (tests/test_sort_cpu.py checks their decision margins on the CPU, tests/test_sort_gpu.py runs
the operator on them): the smallest shapes at which csrc/sort_tracks.hip can still go wrong.  A scene is dict(dets float64 [N,4],
frame_offsets int32 [F+1], clip_offsets int32 [C+1], params = the operator's keyword arguments).  Not a test module."""
import functools

import numpy as np


# NOTEBOOK.md, "SORT on the device": the largest relative difference of the filtered boxes between tests/sort_np.py run in float64 and
# in numpy.longdouble (x87 extended, eps 1.08e-19) over scenes() is 8.16e-16 (scene `shrinking`; 3.0e-16 on the 300-frame `walkers`):
# the rounding floor of the contract's arithmetic in fp64.  The operator is allowed 16 x that, because a compiler may order the sums
# inside the 7 x 7 products differently: 1.31e-14.
BOX_FLOOR = 8.16e-16
BOX_TOL = 16 * BOX_FLOOR


def pack(clips, **params):
    """clips: list of clips, a clip a list of frames, a frame a list of (cx, cy, w, h)."""
    dets, fo, co = [], [0], [0]
    for clip in clips:
        for frame in clip:
            dets.extend(frame)
            fo.append(len(dets))
        co.append(len(fo) - 1)
    return {"dets": np.asarray(dets, np.float64).reshape(-1, 4), "frame_offsets": np.asarray(fo, np.int32),
            "clip_offsets": np.asarray(co, np.int32), "params": params}


def walk(r, T, x0, y0, vx=0.0, vy=0.0, w=40.0, h=90.0, jitter=0.7, grow=0.0):
    """T boxes of a person moving at (vx, vy) from (x0, y0), every number jittered: no two scenes' IoUs sit on a tie."""
    t = np.arange(T)
    return np.stack([x0 + vx * t + r.uniform(-jitter, jitter, T), y0 + vy * t + r.uniform(-jitter, jitter, T),
                     w + grow * t + r.uniform(-jitter, jitter, T), h + grow * t + r.uniform(-jitter, jitter, T)], 1)


def frames_of(T, people):
    """people: list of (first frame, boxes [n,4], set of frames in which the person is NOT detected)."""
    out = [[] for _ in range(T)]
    for start, boxes, missing in people:
        for i, b in enumerate(boxes):
            if start + i < T and (start + i) not in missing:
                out[start + i].append(tuple(b))
    return out


def lost_scene(r, max_age):
    """Person 0 is always seen.  Person 1 is lost for max_age frames (kept: same id afterwards), seen for six frames, then lost for
    max_age + 1 frames (reborn under a new id).  She stands still, so the predicted box stays on her while she is lost."""
    a, b = 6, 6 + max_age + 6
    T = b + max_age + 1 + 6
    gone = set(range(a, a + max_age)) | set(range(b, b + max_age + 1))
    return pack([frames_of(T, [(0, walk(r, T, 100, 200, vx=2.0), set()), (0, walk(r, T, 400, 220, jitter=0.3), gone)])], max_age=max_age)


@functools.lru_cache(maxsize=None)
def scenes():
    r = np.random.default_rng(32)
    S = {}
    S["t1"] = pack([frames_of(1, [(0, walk(r, 1, 100, 100), set()), (0, walk(r, 1, 300, 120), set())])])
    S["ragged"] = pack([frames_of(5, [(0, walk(r, 5, 100, 100, vx=3), set()), (1, walk(r, 4, 300, 100), set())]), [],
                        frames_of(3, [(0, walk(r, 3, 50, 60), set())])])
    S["empty_frames"] = pack([frames_of(14, [(2, walk(r, 10, 200, 200, vx=1.5, vy=-1), {6, 7})])])      # none at 0, 1, 6, 7, 12, 13
    S["one_person"] = pack([frames_of(10, [(0, walk(r, 10, 150, 150, vx=4, vy=1), set())])])
    S["crossing"] = pack([frames_of(24, [(0, walk(r, 24, 100, 200, vx=8), set()), (0, walk(r, 24, 290, 212, vx=-8), set())])])
    for age in (0, 1, 5):
        S[f"lost_age{age}"] = lost_scene(r, age)
    for hits in (0, 3):
        S[f"late_hits{hits}"] = pack([frames_of(12, [(0, walk(r, 12, 100, 100, vx=2), set()), (5, walk(r, 7, 400, 300, vy=-3), set())])],
                                     min_hits=hits)
    S["more_dets_then_fewer"] = pack([frames_of(12, [(0, walk(r, 12, 60 + 110 * i, 100 + 7 * i, vx=1.0 + i), set()) for i in range(3)] +
                                                [(4, walk(r, 4, 500 + 120 * i, 300, vy=2), set()) for i in range(2)] +
                                                [(0, walk(r, 12, 60 + 110 * i, 400), set(range(9, 12))) for i in range(2)])])
    t = np.arange(9)
    side = np.array([60, 52, 44, 36, 28, 20, 12, 6, 3], np.float64) + r.uniform(-0.2, 0.2, 9)
    shrink = np.stack([200 + 0.3 * t + r.uniform(-0.2, 0.2, 9), 200 + r.uniform(-0.2, 0.2, 9), side, side * 1.5], 1)
    S["shrinking"] = pack([frames_of(9, [(0, shrink, set()), (0, walk(r, 9, 500, 100), set())])])
    S["cap64"] = pack([frames_of(4, [(0, walk(r, 4, 40 + 70 * (i % 8), 60 + 120 * (i // 8), vx=1.5, vy=0.5, jitter=0.5), set())
                                     for i in range(64)])])
    S["overflow"] = pack([frames_of(6, [(0, walk(r, 6, 100, 100), set()), (0, walk(r, 6, 300, 100), set()), (2, walk(r, 4, 500, 100), set())]),
                          frames_of(3, [(0, walk(r, 3, 100, 100), set())])], max_trackers=2)
    T = 300
    people = []
    for i in range(5):
        steps = np.cumsum(r.normal(0, 2.0, (T, 2)), 0)
        size = 60 + np.cumsum(r.normal(0, 0.4, T))
        people.append((0, np.stack([150 + 160 * i + steps[:, 0], 300 + steps[:, 1], size, 2.2 * size + r.uniform(-0.5, 0.5, T)], 1), set()))
    S["walkers"] = pack([frames_of(T, people)])
    return S


def tie_scene():
    """Two bit-identical detections over one tracker: two optima of the same total - validity and the total are checked, not equality."""
    b = (100.0, 100.0, 40.0, 80.0)
    return pack([[[b], [b], [b, b], [b]]], min_hits=0)
