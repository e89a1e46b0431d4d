"""Record what demo.py --mode folder writes WITHOUT any optional flag on a seeded synthetic input, as sha256 digests of every array
of every result file (key, dtype, shape and bytes; the .npz container itself carries the zip entries' time stamps and is not hashed):

    python tools/gen_demo_plain_golden.py --out tests/golden/demo_plain_folder.json [--root <checkout>]

tests/test_demo_tta_gpu.py asserts that a run without --tta still writes exactly these arrays.  The fixture in tests/golden/ was
recorded on one MI355X with `--root` pointing at a checkout of the commit BEFORE test-time augmentation was added (DESIGN.md section
26), so it pins the no-flag path to that commit bit for bit.  Re-record it only with a change that is meant to alter the no-flag
results.  The input: resnet50-cliff with the synthetic weights of seed 0, the synthetic body model of seed 7, five 96 x 128 images
from default_rng(6) with two detections each, batch size 8."""
import argparse
import hashlib
import json
import os
import sys
import tempfile
from pathlib import Path

import numpy as np

H, W, NIMG = 96, 128, 5
CFG = "configs/demo_poco_cliff_resnet50.yaml"


def make_inputs(tmp: Path):
    """Checkpoint, body model, images and detections under `tmp`; returns (weights, frames, dets)."""
    import torch
    from PIL import Image
    from poco_amd import synth
    from tests import util
    w = util.synth_weights("resnet50-cliff")
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, tmp / "m1.pt")
    np.savez(tmp / "smpl.npz", **synth.synth_smpl(7))
    r = np.random.default_rng(6)
    (tmp / "imgs").mkdir()
    dets, frames = {}, {}
    for i in range(NIMG):
        frames[i] = r.integers(0, 256, (H, W, 3), dtype=np.uint8)
        Image.fromarray(frames[i]).save(tmp / "imgs" / f"{i:03d}.png")
        dets[f"{i:03d}.png"] = [[40.0 + 3 * i, 48.0, 60.0, 60.0], [84.0 - 2 * i, 50.0, 56.0, 64.0]]
    (tmp / "dets.json").write_text(json.dumps(dets))
    return w, frames, dets


def demo_args(tmp: Path, name: str, flags=()):
    return ["--cfg", CFG, "--ckpt", str(tmp / "m1.pt"), "--batch_size", "8", "--smpl", str(tmp / "smpl.npz"), "--no_render",
            "--output_folder", str(tmp / name), "--mode", "folder", "--image_folder", str(tmp / "imgs"), "--detections", str(tmp / "dets.json"),
            *flags]


def digest(arrays: dict) -> dict:
    """{key: sha256 of (dtype, shape, bytes)} of one result file's arrays."""
    out = {}
    for k in sorted(arrays):
        a = np.ascontiguousarray(arrays[k])
        h = hashlib.sha256()
        h.update(f"{a.dtype.str}|{a.shape}|".encode())
        h.update(a.tobytes())
        out[k] = h.hexdigest()
    return out


def result_digests(tmp: Path, name: str) -> dict:
    return {f"{i:03d}_poco.npz": digest(dict(np.load(tmp / name / "imgs_" / f"{i:03d}_poco.npz"))) for i in range(NIMG)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", required=True)
    ap.add_argument("--root", default=str(Path(__file__).resolve().parent.parent), help="the checkout whose demo.py is run")
    args = ap.parse_args()
    out = Path(args.out).resolve()
    root = Path(args.root).resolve()
    os.chdir(root)                                                   # demo.py reads configs/ relative to the checkout
    sys.path.insert(0, str(root))
    import demo
    with tempfile.TemporaryDirectory() as tmp:
        tmp = Path(tmp)
        make_inputs(tmp)
        demo.main(demo.parse_args(demo_args(tmp, "plain")))
        d = result_digests(tmp, "plain")
    out.parent.mkdir(parents=True, exist_ok=True)
    out.write_text(json.dumps(d, indent=1, sort_keys=True) + "\n")
    print(f"wrote {out}: {len(d)} files, {sum(len(v) for v in d.values())} arrays")


if __name__ == "__main__":
    main()
