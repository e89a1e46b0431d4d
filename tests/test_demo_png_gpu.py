"""GPU: demo.py --render --image_format png --encode gpu end to end, folder and video mode, on the synthetic assets of
tests/test_demo_gpu.py: the written .png files are the restatement's bytes of the rendered pictures and decode to exactly the
pixels of the default run's files, and the default run still writes what PIL writes."""
import io
import json

import numpy as np
import pytest
import torch
from PIL import Image

from poco_amd import synth
from tests import png_np, util

pytestmark = pytest.mark.gpu


def _assets(tmp_path, variant="resnet50-cliff"):
    w = util.synth_weights(variant)
    ckpt = tmp_path / "poco_synth.pt"
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, ckpt)
    smpl = synth.synth_smpl(7)
    smpl["faces"] = np.stack([np.arange(0, 3000), np.arange(1, 3001), np.arange(2, 3002)], 1).astype(np.int32)
    np.savez(tmp_path / "smpl.npz", **smpl)
    return ckpt, tmp_path / "smpl.npz"


def _pil_bytes(pic: np.ndarray) -> bytes:
    buf = io.BytesIO()
    Image.fromarray(pic).save(buf, "PNG")
    return buf.getvalue()


def test_demo_folder_png_on_gpu(tmp_path, cuda):
    import demo
    ckpt, smpl = _assets(tmp_path)
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    r = np.random.default_rng(0)
    sizes = [(200, 300), (240, 320)]                       # the second is larger: the tester re-creates its encoder
    frames = {f"im{i}.png": r.integers(0, 256, (h, w, 3), dtype=np.uint8) for i, (h, w) in enumerate(sizes)}
    for n, fr in frames.items():
        Image.fromarray(fr).save(imgs / n)
    dets = {"im0.png": [[200, 100, 120, 160]], "im1.png": [[160, 120, 150, 150], [80, 100, 90, 120]]}
    (tmp_path / "dets.json").write_text(json.dumps(dets))
    common = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(ckpt), "--mode", "folder", "--image_folder", str(imgs),
              "--batch_size", "4", "--smpl", str(smpl), "--detections", str(tmp_path / "dets.json"), "--render"]
    demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "gpu"), "--encode", "gpu"]))
    demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "host")]))
    for n, fr in frames.items():
        g = tmp_path / "gpu" / "imgs_" / "poco_results" / n
        h = tmp_path / "host" / "imgs_" / "poco_results" / n
        pic = np.asarray(Image.open(h))
        assert pic.shape == fr.shape and (pic != fr).any()                # something was drawn
        assert h.read_bytes() == _pil_bytes(pic)                          # the default run: PIL's file, as before
        assert g.read_bytes() == png_np.encode(pic)                       # --encode gpu: the contract's bytes of the same picture
        assert np.array_equal(np.asarray(Image.open(g).convert("RGB")), pic)


def test_demo_video_png_on_gpu(tmp_path, cuda):
    import demo
    ckpt, smpl = _assets(tmp_path)
    fr_dir = tmp_path / "frames"
    fr_dir.mkdir()
    r = np.random.default_rng(1)
    for i in range(4):
        Image.fromarray(r.integers(0, 256, (120, 160, 3), dtype=np.uint8)).save(fr_dir / f"{i:06d}.png")
    tracks = {"0": {"bbox": [[80, 60, 80, 80]] * 2, "frames": [0, 1]}, "1": {"bbox": [[50, 70, 60, 70]] * 2, "frames": [1, 2]}}
    (tmp_path / "tracks.json").write_text(json.dumps(tracks))                 # frame 3 has nobody: encoded like any other
    common = ["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(ckpt), "--mode", "video", "--vid_file", str(fr_dir),
              "--batch_size", "5", "--smpl", str(smpl), "--tracking", str(tmp_path / "tracks.json"), "--render", "--sideview"]
    demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "gpu"), "--encode", "gpu"]))
    demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "host")]))
    for k in range(4):
        g = tmp_path / "gpu" / "frames_" / "tmp_images_output" / f"{k:06d}.png"
        h = tmp_path / "host" / "frames_" / "tmp_images_output" / f"{k:06d}.png"
        pic = np.asarray(Image.open(h))
        assert pic.shape == (120, 320, 3)
        assert h.read_bytes() == _pil_bytes(pic)
        assert g.read_bytes() == png_np.encode(pic)
        assert np.array_equal(np.asarray(Image.open(g).convert("RGB")), pic)
