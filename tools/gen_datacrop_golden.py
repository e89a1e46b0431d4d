"""Make tests/golden/datacrop.npz: what the REFERENCE's own dataset code gives on seeded inputs, for everything of the dataset crop
that does not go through cv2 (absent here): augm_params sequences, gen_trans_from_patch_cv's point triples (cv2.getAffineTransform
replaced by a recorder), flip_pose, flip_kp, j3d_processing, j2d_processing / transform with rot != 0 and calculate_bbox_info with
sc.  crop_cv2's warp and rot_aa (cv2.Rodrigues) cannot be run here; tools/validate_assets.py --dataset-crop covers them where
opencv-python is installed.

    python tools/gen_datacrop_golden.py [--reference DIR] [--out tests/golden/datacrop.npz]

The reference's modules are imported from DIR with their third-party imports stubbed; only data is written."""
import argparse
import importlib
import logging
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _Any(types.ModuleType):
    """A module whose every attribute is another such module / a no-op callable."""

    def __getattr__(self, k):
        if k.startswith("__"):
            raise AttributeError(k)
        m = _Any(self.__name__ + "." + k)
        sys.modules[m.__name__] = m
        setattr(self, k, m)
        return m

    def __call__(self, *a, **k):
        return None


def _stub(n):
    m = _Any(n)
    m.__path__ = []
    sys.modules[n] = m
    if "." in n and n.rsplit(".", 1)[0] in sys.modules:
        setattr(sys.modules[n.rsplit(".", 1)[0]], n.rsplit(".", 1)[1], m)


def import_reference(ref):
    """pocolib.utils.image_utils, pocolib.utils.vibe_image_utils, pocolib.dataset.base_dataset and pocolib.core.constants, without
    running the packages' __init__ files (they pull in the models and the trainer)."""
    for pkg in ("pocolib", "pocolib.core", "pocolib.utils", "pocolib.dataset"):
        m = types.ModuleType(pkg)
        m.__path__ = [os.path.join(ref, *pkg.split("."))]
        sys.modules[pkg] = m
    for n in ("cv2", "pocolib.models", "pocolib.dataset.occlusion", "pocolib.utils.train_utils", "pocolib.core.config"):
        _stub(n)
    lg = types.ModuleType("loguru")
    lg.logger = logging.getLogger("ref")
    sys.modules["loguru"] = lg
    import scipy  # noqa: F401
    _stub("scipy.misc")                              # removed from scipy long ago; the reference only names it
    sys.path.insert(0, ref)
    mods = {}
    for n in ("pocolib.core.constants", "pocolib.utils.vibe_image_utils", "pocolib.utils.image_utils", "pocolib.dataset.base_dataset"):
        for _ in range(64):                          # every third-party module this machine lacks becomes a stub, one per attempt
            try:
                mods[n.rsplit(".", 1)[1]] = importlib.import_module(n)
                break
            except ModuleNotFoundError as e:
                if not e.name or e.name.startswith("pocolib"):
                    raise
                _stub(e.name)
                sys.modules.pop(n, None)
    return mods


def main():
    ap = argparse.ArgumentParser()
    sys.path.insert(0, ROOT)
    from oracle import ref_import
    ap.add_argument("--reference", default=ref_import.REFERENCE)
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "datacrop.npz"))
    a = ap.parse_args()
    mods = import_reference(a.reference)
    iu, viu, bd, const = mods["image_utils"], mods["vibe_image_utils"], mods["base_dataset"], mods["constants"]
    out = {"smpl_pose_flip_perm": np.asarray(const.SMPL_POSE_FLIP_PERM, np.int32), "j24_flip_perm": np.asarray(const.J24_FLIP_PERM, np.int32)}

    # augm_params: 12 draws per seed, training and evaluation, FLIP on and off
    opts = types.SimpleNamespace(FLIP=1, NOISE_FACTOR=0.4, ROT_FACTOR=30, SCALE_FACTOR=0.25, IMG_RES=224)
    me = types.SimpleNamespace(options=opts, is_train=True, use_augmentation=True)
    seeds, seqs = [0, 7, 123], []
    for flip_on in (1, 0):
        opts.FLIP = flip_on
        for s in seeds:
            np.random.seed(s)
            seqs.append([np.concatenate([[f], pn, [r], [sc]]) for f, pn, r, sc in (bd.BaseDataset.augm_params(me) for _ in range(12))])
    out["augm_seeds"], out["augm_train"] = np.asarray(seeds, np.int32), np.asarray(seqs, np.float64).reshape(2, len(seeds), 12, 6)
    me.is_train = False
    np.random.seed(5)
    out["augm_eval"] = np.concatenate([np.concatenate([[f], pn, [r], [sc]]) for f, pn, r, sc in [bd.BaseDataset.augm_params(me)]]).astype(np.float64)
    opts.FLIP = 1

    # gen_trans_from_patch_cv as crop_cv2 calls it: the two float32 point triples handed to cv2.getAffineTransform
    rec = []
    viu.cv2.getAffineTransform = lambda s, d: rec.append((np.array(s), np.array(d))) or np.zeros((2, 3))
    r = np.random.default_rng(11)
    pts_in = []
    for rot in (0.0, 30.0, -47.5, 90.0, 180.0, 12.3456789, -171.25):
        for _ in range(3):
            c_x, c_y, bb, res = int(r.integers(-50, 2000)), int(r.integers(-50, 1200)), int(r.integers(1, 900)), int(r.choice([32, 224]))
            viu.gen_trans_from_patch_cv(c_x, c_y, bb, bb, res, res, scale=1.0, rot=rot, inv=False)
            pts_in.append((c_x, c_y, bb, res, rot))
    out["pts_in"] = np.asarray(pts_in, np.float64)
    out["pts_src"] = np.stack([s for s, _ in rec]).astype(np.float32)
    out["pts_dst"] = np.stack([d for _, d in rec]).astype(np.float32)
    assert all(s.dtype == np.float32 and d.dtype == np.float32 for s, d in rec)

    # ground-truth transforms
    pose = 0.5 * r.standard_normal((4, 72))
    out["pose"], out["flip_pose"] = pose, np.stack([iu.flip_pose(p.copy()) for p in pose])
    S = np.concatenate([r.standard_normal((4, 24, 3)), np.ones((4, 24, 1))], 2)
    out["S"], out["flip_kp"] = S, np.stack([iu.flip_kp(s.copy()) for s in S])
    gt = [(30.0, 0), (-47.5, 1), (0, 1), (180.0, 0)]
    out["gt_rot_flip"] = np.asarray(gt, np.float64)
    out["j3d"] = np.stack([bd.BaseDataset.j3d_processing(me, s.copy(), rr, int(f)) for s, (rr, f) in zip(S, gt)])
    kp = np.concatenate([r.uniform(0, 400, (4, 24, 2)), r.uniform(0, 1, (4, 24, 1))], 2)
    cen, scl = r.uniform(100, 300, (4, 2)), r.uniform(0.5, 1.5, 4) * np.array([0.75, 1.0, 1.25, 1.1])
    out["kp"], out["kp_center"], out["kp_scale"] = kp, cen, scl
    out["j2d"] = np.stack([bd.BaseDataset.j2d_processing(me, k.copy(), c, s, rr, int(f)) for k, c, s, (rr, f) in zip(kp, cen, scl, gt)])
    out["transform"] = np.stack([iu.transform(k[0, :2] + 1, c, s, [224, 224], rot=rr) for k, c, s, (rr, _) in zip(kp, cen, scl, gt)]).astype(np.int64)
    shp = np.array([[480, 640], [1080, 1920], [1920, 1080], [61, 83]], np.float64)
    out["bbox_shape"] = shp
    out["bbox_info"] = np.stack([iu.calculate_bbox_info(c, s, hw) for c, s, hw in zip(cen, scl, shp)])
    np.savez_compressed(a.out, **out)
    print(f"wrote {a.out}: {sorted(out)}")


if __name__ == "__main__":
    main()
