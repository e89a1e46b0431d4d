"""Make tests/golden/occlude.npz: what the REFERENCE's own occlude_with_pascal_objects_kp (pocolib/dataset/occlusion.py:109-149) gives
on seeded inputs - its draw order, the centres and sizes it hands on, and paste_over's clipping and blend.  cv2 is absent here, so
cv2.resize is replaced by a recorder that logs (source shape, new_size, interpolation) and returns the RESTATED resize
(tests/occlude_np.py resize_area): the resize inside the fixture is ours, and the key `resize_is_restated` says so.

    python tools/gen_occlude_golden.py [--reference DIR] [--out tests/golden/occlude.npz]

The reference's module is imported from DIR with cv2, skimage, matplotlib and its package siblings stubbed; only data is written."""
import argparse
import importlib
import os
import random
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

INTER_LINEAR, INTER_AREA = 1, 3                       # cv2's values


def import_occlusion(ref):
    import types
    import gen_datacrop_golden as g
    for pkg in ("pocolib", "pocolib.core", "pocolib.utils", "pocolib.dataset"):
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(ref, *pkg.split("."))]
        sys.modules[pkg] = m
    for n in ("cv2", "skimage", "skimage.data", "matplotlib", "matplotlib.pyplot", "loguru", "pocolib.core.config", "pocolib.utils.kp_utils"):
        g._stub(n)
    sys.path.insert(0, ref)
    for _ in range(64):
        try:
            return importlib.import_module("pocolib.dataset.occlusion")
        except ModuleNotFoundError as e:
            if not e.name or e.name.startswith("pocolib"):
                raise
            g._stub(e.name)
            sys.modules.pop("pocolib.dataset.occlusion", None)
    raise RuntimeError("could not import the reference's occlusion module")


def cutouts(r):
    """Synthetic RGBA cut-outs: odd and even sides, alpha 0 / 192 / 255 as the reference's masks hold, one fully opaque."""
    out = []
    for h, w in ((37, 52), (64, 48), (90, 121), (40, 23)):
        a = r.integers(0, 256, (h, w, 4), dtype=np.uint8)
        a[..., 3] = r.choice(np.array([0, 192, 255], np.uint8), (h, w), p=[0.3, 0.2, 0.5])
        out.append(a)
    out[3][..., 3] = 255
    return out


def keypoint_sets(r):
    """[49, 3] keypoint sets in normalised crop coordinates, float32 (the reference slices [25:]): a spread one with a few invisible
    joints, one with a single visible keypoint, one with keypoints on and beyond the crop border."""
    kps = []
    k = np.zeros((49, 3), np.float32)
    k[:, :2] = r.uniform(-0.8, 0.8, (49, 2))
    k[:, 2] = r.choice([0.0, 0.25, 0.31, 1.0], 49)
    k[25, 2] = 1.0
    kps.append(k)
    k = np.zeros((49, 3), np.float32)
    k[:, :2] = r.uniform(-0.8, 0.8, (49, 2))
    k[:25, 2] = 1.0                                      # the OpenPose block is not read
    k[25 + 13] = (0.21, -0.43, 0.9)
    kps.append(k)
    k = np.zeros((49, 3), np.float32)
    k[:, 2] = 1.0
    edge = np.array([(-1, -1), (1, 1), (-1, 1), (1, -1), (-1, 0), (1, 0), (0, -1), (0, 1), (-1.2, 0.3), (1.3, 1.3), (0, 0), (0.99, -0.99)],
                    np.float32)
    k[25:, :2] = edge[np.arange(24) % len(edge)]
    kps.append(k)
    return kps


def main():
    ap = argparse.ArgumentParser()
    from oracle import ref_import
    ap.add_argument("--reference", default=ref_import.REFERENCE)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "occlude.npz"))
    a = ap.parse_args()
    occ = import_occlusion(a.reference)
    from tests import occlude_np
    calls = []

    def resize(im, new_size, fx=None, fy=None, interpolation=None):
        calls.append((im.shape[0], im.shape[1], int(new_size[0]), int(new_size[1]), int(interpolation)))
        return occlude_np.resize_area(im, new_size)

    occ.cv2.resize, occ.cv2.INTER_LINEAR, occ.cv2.INTER_AREA = resize, INTER_LINEAR, INTER_AREA
    centres, paste_over = [], occ.paste_over

    def paste_recorder(im_src, im_dst, center):
        centres.append((int(center[0]), int(center[1]), im_src.shape[1], im_src.shape[0]))
        return paste_over(im_src=im_src, im_dst=im_dst, center=center)

    occ.paste_over = paste_recorder                      # the reference's own paste_over runs; its arguments are logged
    r = np.random.default_rng(23)
    cuts, kps = cutouts(r), keypoint_sets(r)
    out = {"resize_is_restated": np.array(1, np.int32), "n_cutouts": np.array(len(cuts), np.int32), "n_kp_sets": np.array(len(kps), np.int32)}
    for i, c in enumerate(cuts):
        out[f"cutout_{i}"] = c
    for i, k in enumerate(kps):
        out[f"kp_{i}"] = k
    # (keypoint set, res, scale = sc * scale, seed): every keypoint set at res 224 and at res 32
    cases = [(0, 224, 1.1, 0), (1, 224, 2.3, 2), (2, 224, 1.0, 3), (2, 32, 1.7, 4), (0, 32, 0.9, 5), (1, 32, 1.0, 6), (0, 32, 1.37, 7),
             (2, 32, 3.0, 8)]
    out["cases"] = np.asarray(cases, np.float64)
    for ci, (ki, res, scale, seed) in enumerate(cases):
        crop = occlude_np.synthetic_crop(res, ci)
        np.random.seed(seed)
        random.seed(seed)
        calls.clear()
        centres.clear()
        got = occ.occlude_with_pascal_objects_kp(crop.copy(), kps[ki].copy(), np.float64(scale), cuts)
        assert got.dtype == np.float32 and all(c[4] == INTER_AREA for c in calls)
        out[f"crop_{ci}"], out[f"out_{ci}"] = crop, got
        out[f"calls_{ci}"] = np.asarray(calls, np.int64).reshape(-1, 5)        # source h, w, new w, new h, interpolation
        out[f"pastes_{ci}"] = np.asarray(centres, np.int64).reshape(-1, 4)     # centre x, y, pasted w, h
        out[f"next_{ci}"] = np.array([np.random.uniform(), random.random()])      # the generators' states after the sample
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out}: {os.path.getsize(a.out)} bytes, {len(out)} arrays, {sum(len(out[f'calls_{i}']) for i in range(len(cases)))} objects")


if __name__ == "__main__":
    main()
