"""Make tests/golden/tracks.npz: the REFERENCE's keypoint-to-box parameters on seeded keypoint tracks.  CPU only; needs the
reference checkout (oracle/ref_import.REFERENCE), numpy and scipy.

    python tools/gen_tracks_golden.py

pocolib/utils/smooth_bbox.py is imported by file path (the pocolib package does not import without its other dependencies) and
its get_all_bbox_params(., 0.3) and smooth_bbox_params run on each track; ONLY their outputs and the tracks go into the file.  The
reference's parameters take the keypoints' float type (float64 keypoints, what a tracker's pickle holds, give float64); the two
cases that interpolate with few frames in between are also stored for float32 keypoints (c3_params32, c7_params32).

Keypoints are stored as int16 (CASES_40 in one array, so that the shared coordinates compress): x, y in half pixels,
confidence in 1/16; a test decodes them with `decode` below (exact in either float type) and drops the frames of the `none`
mask.  Per case c1 .. c7: c<i>_params64, c<i>_smooth64 and c<i>_range = (start, end).

    c1  40 frames x 25 joints, clean                          c5  one frame whose visible joints coincide (diagonal 0)
    c2  frames 0-2 and 37-39 below the threshold (trim)       c6  5 frames: shorter than the median kernel
    c3  interior gaps of 1 (frame 10) and 7 (20-26) frames    c7  12 frames x 44 joints, one missing frame
    c4  None entries: 0, 1, 15, 16, 17, 39"""
import importlib.util
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import ref_import  # noqa: E402

OUT = ROOT / "tests" / "golden" / "tracks.npz"
VIS_THRESH = 0.3
CASES_40 = ("c1", "c2", "c3", "c4", "c5")


def decode(q, dtype=np.float64):
    """int16 [..., 3] -> keypoints (x, y, confidence) of `dtype`."""
    q = np.asarray(q)
    return np.concatenate([q[..., :2].astype(dtype) / dtype(2), q[..., 2:].astype(dtype) / dtype(16)], -1)


def person(rng, T, K):
    """int16 [T,K,3]: a skeleton of K joints inside about 60 x 160 px that drifts, sways and grows over T frames; confidences
    0.5 .. 1 except two joints per frame at 0.125."""
    skel = rng.uniform(-1, 1, (K, 2)) * np.array([30.0, 80.0])
    t = np.arange(T)[:, None, None]
    xy = np.array([300.0, 250.0]) + np.array([2.5, -0.75]) * t + skel * (1 + 0.01 * t) + rng.normal(0, 1.5, (T, K, 2))
    conf = rng.uniform(0.5, 1.0, (T, K))
    for f in range(T):
        conf[f, rng.choice(K, 2, replace=False)] = 0.125
    return np.concatenate([np.rint(xy * 2), np.rint(conf * 16)[..., None]], -1).astype(np.int16)


def main():
    assert ref_import.available(), "needs the reference checkout"
    path = Path(ref_import.REFERENCE) / "pocolib" / "utils" / "smooth_bbox.py"
    spec = importlib.util.spec_from_file_location("ref_smooth_bbox", path)
    ref = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(ref)

    rng = np.random.default_rng(28)
    low = np.int16(2)                           # 0.125
    base = person(rng, 40, 25)
    kp40 = np.stack([base] * len(CASES_40))
    none40 = np.zeros((len(CASES_40), 40), bool)
    kp40[1, [0, 1, 2, 37, 38, 39], :, 2] = low
    kp40[2, [10] + list(range(20, 27)), :, 2] = low
    none40[3, [0, 1, 15, 16, 17, 39]] = True
    vis = kp40[4, 12, :, 2] > VIS_THRESH * 16
    kp40[4, 12, vis, :2] = kp40[4, 12, 0, :2]
    kp5 = person(rng, 5, 25)
    kp44 = person(rng, 12, 44)
    none44 = np.zeros(12, bool)
    none44[6] = True

    o = {"kp40": kp40, "none40": none40, "kp5": kp5, "kp44": kp44, "none44": none44, "vis_thresh": np.float64(VIS_THRESH)}
    tracks = {name: (kp40[i], none40[i]) for i, name in enumerate(CASES_40)}
    tracks["c6"] = (kp5, np.zeros(5, bool))
    tracks["c7"] = (kp44, none44)
    for name, (q, none) in tracks.items():
        for bits, dt in ((64, np.float64), (32, np.float32)):
            kps = [None if n else k for k, n in zip(decode(q, dt), none)]
            params, start, end = ref.get_all_bbox_params(kps, VIS_THRESH)
            assert params.dtype == dt and len(params) == end - start, (name, params.dtype, start, end)
            if bits == 64:
                o[f"{name}_params64"], o[f"{name}_smooth64"] = params, ref.smooth_bbox_params(params)
                o[f"{name}_range"] = np.array([start, end], np.int64)
            elif name in ("c3", "c7"):
                o[f"{name}_params32"] = params
    # the cases are what their names say
    assert tuple(o["c1_range"]) == (0, 40) and tuple(o["c2_range"]) == (3, 37) and tuple(o["c3_range"]) == (0, 40)
    assert tuple(o["c4_range"]) == (2, 39) and tuple(o["c5_range"]) == (0, 40) and tuple(o["c6_range"]) == (0, 5)
    assert np.array_equal(o["c2_params64"], o["c1_params64"][3:37]) and not np.array_equal(o["c3_params64"], o["c1_params64"])
    assert not np.array_equal(o["c5_params64"][12], o["c1_params64"][12])
    np.savez_compressed(OUT, **o)
    print(f"{OUT}: {OUT.stat().st_size} bytes, {len(o)} arrays")


if __name__ == "__main__":
    main()
