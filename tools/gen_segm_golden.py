"""Make tests/golden/segm.npz: the outputs of the REFERENCE's own functions on the seeded inputs of tests/segm_np.py.  CPU only;
needs the reference checkout (oracle/ref_import.py).

    python tools/gen_segm_golden.py

Runs CrossEntropy (pocolib/losses/segmentation.py) on the seeded logits [3,25,56,56] and labels [3,224,224], and
estimate_translation (pocolib/utils/geometry.py) on seeded joints whose last row is singular, and stores ONLY data: the inputs
(`S`, `joints2d`; of the seeded `logits` and `labels`, which tests/segm_np.py regenerates, their CRC-32) and the reference's outputs (`ce` = its mean loss, `cam_t` float32 [B,3]).  The reference
takes joints 25:49 of 49; the 24 seeded joints are placed there."""
import importlib
import importlib.util
import sys
from pathlib import Path

import numpy as np
import torch

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from oracle import ref_import  # noqa: E402
from poco_amd import synth  # noqa: E402
from tests import segm_np  # noqa: E402

OUT = ROOT / "tests" / "golden" / "segm.npz"


def main():
    assert ref_import.available(), "needs the reference checkout"
    torch.set_num_threads(8)
    mp = synth.synth_state_dict([("head.init_pose", (1, 144)), ("head.init_shape", (1, 10)), ("head.init_cam", (1, 3))], 0)
    ref_import.setup({"pose": mp["head.init_pose"][0], "shape": mp["head.init_shape"][0], "cam": mp["head.init_cam"][0]})
    ref_import.setup_host_utils()
    geo = importlib.import_module("pocolib.utils.geometry")
    spec = importlib.util.spec_from_file_location("ref_losses_segmentation",
                                                  Path(ref_import.REFERENCE) / "pocolib" / "losses" / "segmentation.py")
    seg = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(seg)
    assert geo.__file__.startswith(ref_import.REFERENCE)

    logits, labels = segm_np.golden_logits()
    with torch.no_grad():
        ce = float(seg.CrossEntropy()(torch.from_numpy(logits.copy()), torch.from_numpy(labels.astype(np.int64))))
    S, k2d = segm_np.translation_fixture()
    B = S.shape[0]
    S49, k49 = np.ones((B, 49, 3), np.float32), np.zeros((B, 49, 3), np.float32)
    S49[:, 25:], k49[:, 25:] = S, k2d
    cam_t = geo.estimate_translation(torch.from_numpy(S49), torch.from_numpy(k49), focal_length=5000.0, img_size=224.0).numpy()
    assert cam_t.dtype == np.float32 and np.array_equal(cam_t[-1], [1, 1, 1]) and not np.any(np.all(cam_t[:-1] == 1, axis=1))
    import zlib
    o = {"logits_crc": np.uint32(zlib.crc32(logits.tobytes())), "labels_crc": np.uint32(zlib.crc32(labels.tobytes())),
         "ce": np.float64(ce), "S": S, "joints2d": k2d, "cam_t": cam_t}
    OUT.parent.mkdir(parents=True, exist_ok=True)
    np.savez_compressed(OUT, **o)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes): CrossEntropy = {ce!r}, cam_t =\n{cam_t}")


if __name__ == "__main__":
    main()
