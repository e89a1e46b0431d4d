"""GPU: the JPEG encoder (csrc/jpeg_enc.hip) against its numpy restatement (tests/jpeg_np.py) BYTE for byte, its guard bands,
scratch reuse and argument checks, and demo.py --image_format jpg / --save_video end to end."""
import functools
import io
import json

import numpy as np
import pytest
import torch
from PIL import Image

from poco_amd import jpeg, render, synth
from poco_amd._lib import lib
from tests import jpeg_np, render_np, util
from tests.test_jpeg_cpu import parse_avi

pytestmark = pytest.mark.gpu

POISON = 0xA5


@functools.lru_cache(maxsize=None)
def _reference(fill, H, W, q):
    return jpeg_np.encode(jpeg_np.fixture(fill, H, W), q)


def _first_difference(a: bytes, b: bytes):
    n = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))[0]
    return (len(a), len(b), int(d[0]) if d.size else None)


@pytest.mark.parametrize("H,W", jpeg_np.FIXTURE_SHAPES)
def test_bytes_equal_the_restatement(cuda, H, W):
    enc = jpeg.JpegEncoder(cuda, H, W)
    for fill in jpeg_np.FIXTURE_FILLS:
        frame = torch.from_numpy(jpeg_np.fixture(fill, H, W)).to(cuda)
        for q in jpeg_np.FIXTURE_QUALITIES:
            got, ref = enc.encode(frame, q), _reference(fill, H, W, q)
            assert got == ref, (fill, q, _first_difference(got, ref))


@pytest.mark.parametrize("H,W", [(24, 700), (20, 1400)])
def test_wide_frames_take_every_path(cuda, H, W):
    """Sizes at which the kernels take another path than on the small fixtures: more than one transform tile of 16 MCUs (the last
    one partial), more than 256 blocks per interval (264 and 528: the entropy kernel codes them in rounds of 256 and carries the
    unfinished byte across), and at quality 100 more than 1024 bytes per round (several stuffing passes)."""
    enc = jpeg.JpegEncoder(cuda, H, W)
    for fill, q in (("noise", 100), ("noise", 50), ("gradient", 50), ("checker", 100)):
        got, ref = enc.encode(torch.from_numpy(jpeg_np.fixture(fill, H, W)).to(cuda), q), _reference(fill, H, W, q)
        assert got == ref, (fill, q, _first_difference(got, ref))


def test_guard_band_and_length(cuda):
    """Nothing outside out[0, len) changes: the buffer is poisoned beyond the reported length and in a guard band in front."""
    H, W, guard = 48, 208, 64
    cap = jpeg.worst_case_bytes(H, W)
    enc = jpeg.JpegEncoder(cuda, H, W)
    for fill, q in (("noise", 100), ("black", 50)):
        buf = torch.full((guard + cap + guard,), POISON, dtype=torch.uint8, device=cuda)
        out, n = enc.encode_into(torch.from_numpy(jpeg_np.fixture(fill, H, W)).to(cuda), buf[guard:guard + cap], q)
        assert out.data_ptr() == buf.data_ptr() + guard and n.dtype == torch.int32 and n.is_cuda
        host, n = buf.cpu().numpy(), int(n.item())
        ref = _reference(fill, H, W, q)
        assert n == len(ref) and host[guard:guard + n].tobytes() == ref
        assert (host[:guard] == POISON).all() and (host[guard + n:] == POISON).all()


def test_encoder_reuse_on_smaller_frames(cuda):
    """An encoder created for 64 x 224 codes three smaller sizes in a row: no stale coefficient, slot or length may leak."""
    enc = jpeg.JpegEncoder(cuda, 64, 224)
    for fill, H, W, q in (("noise", 48, 208, 100), ("checker", 33, 17, 50), ("gradient", 40, 56, 100), ("noise", 16, 16, 50)):
        got = enc.encode(torch.from_numpy(jpeg_np.fixture(fill, H, W)).to(cuda), q)
        ref = _reference(fill, H, W, q)
        assert got == ref, (fill, H, W, q, _first_difference(got, ref))


def test_rendered_frame(cuda):
    """The procedural mesh of tests/render_np.py drawn over a seeded background at 128 x 160, encoded from the device frame."""
    H, W = 128, 160
    r = np.random.default_rng(12)
    verts, faces = render_np.deformed_sphere(3, subdiv=3, radius=0.5)
    frame = torch.from_numpy(r.integers(0, 256, (H, W, 3), dtype=np.uint8)).to(cuda)
    before = frame.clone()
    R = render.Renderer(faces, verts.shape[0], cuda)
    R.render(frame, torch.from_numpy(verts[None]).to(cuda), [[1.2 * H / W, 1.2, 0.0, 0.0]],
             [render.vertex_color(np.full(24, 0.3, np.float32), "hrnet_w48_cls-cliff")], [render.MATERIAL_UNCERT])
    assert (frame != before).any(), "nothing was drawn"
    got = jpeg.JpegEncoder(cuda, H, W).encode(frame, 90)
    host = frame.cpu().numpy()
    assert got == jpeg_np.encode(host, 90)
    dec = np.asarray(Image.open(io.BytesIO(got)).convert("RGB"))
    assert dec.shape == (H, W, 3)


def test_argument_errors_leave_the_output_alone(cuda):
    H, W = 32, 48
    enc = jpeg.JpegEncoder(cuda, H, W)
    cap = jpeg.worst_case_bytes(H, W)
    frame = torch.zeros(H, W, 3, dtype=torch.uint8, device=cuda)
    out = torch.full((cap,), POISON, dtype=torch.uint8, device=cuda)
    n = torch.full((1,), -7, dtype=torch.int32, device=cuda)
    L = lib()
    f, o, ln, h = frame.data_ptr(), out.data_ptr(), n.data_ptr(), enc._h
    bad = [(h, f, 0, W, 90, o, cap, ln), (h, f, H, 0, 90, o, cap, ln), (h, f, H + 1, W, 90, o, cap, ln), (h, f, H, W + 1, 90, o, cap, ln),
           (h, f, H, W, 0, o, cap, ln), (h, f, H, W, 101, o, cap, ln), (None, f, H, W, 90, o, cap, ln), (h, None, H, W, 90, o, cap, ln),
           (h, f, H, W, 90, None, cap, ln), (h, f, H, W, 90, o, cap, None), (h, f, H, W, 90, o, cap - 1, ln)]
    for a in bad:
        assert L.poco_jpeg_encode(*a, None) == 1, a
        assert L.poco_last_error().startswith(b"poco_jpeg_encode")
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == POISON).all() and int(n.item()) == -7
    with pytest.raises(jpeg.PocoHipError, match="quality"):
        enc.encode(frame, 0)
    with pytest.raises(jpeg.PocoHipError, match="uint8"):
        enc.encode(frame.float())
    # the handle still works afterwards
    assert enc.encode(frame, 50) == jpeg_np.encode(np.zeros((H, W, 3), np.uint8), 50)


# ---- demo.py --image_format jpg / --save_video end to end (the synthetic setup of tests/test_demo_gpu.py) ------------------------
def _assets(tmp_path, variant="resnet50-cliff"):
    w = util.synth_weights(variant)
    ckpt = tmp_path / "poco_synth.pt"
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, ckpt)
    smpl = synth.synth_smpl(7)
    smpl["faces"] = np.stack([np.arange(0, 3000), np.arange(1, 3001), np.arange(2, 3002)], 1).astype(np.int32)
    np.savez(tmp_path / "smpl.npz", **smpl)
    return ckpt, tmp_path / "smpl.npz"


def test_demo_folder_jpg(tmp_path, cuda):
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
    demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "jpg"), "--image_format", "jpg"]))
    demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "png")]))
    for n, fr in frames.items():
        jp = tmp_path / "jpg" / "imgs_" / "poco_results" / (n[:-4] + ".jpg")
        pn = tmp_path / "png" / "imgs_" / "poco_results" / (n[:-4] + ".png")
        assert jp.exists() and not jp.with_suffix(".png").exists()
        assert pn.exists() and not pn.with_suffix(".jpg").exists()          # default flags still write .png
        im = Image.open(jp)
        assert im.format == "JPEG" and im.size == (fr.shape[1], fr.shape[0])
        # the .jpg is the encoder's picture of what the .png holds
        assert jp.read_bytes() == jpeg_np.encode(np.asarray(Image.open(pn)), 90)


def test_demo_video_save_video(tmp_path, cuda):
    import demo
    ckpt, smpl = _assets(tmp_path)
    fr_dir = tmp_path / "frames"
    fr_dir.mkdir()
    r = np.random.default_rng(1)
    for i in range(4):
        Image.fromarray(r.integers(0, 256, (120, 160, 3), dtype=np.uint8)).save(fr_dir / f"{i:06d}.png")
    tracks = {"0": {"bbox": [[80, 60, 80, 80]] * 2, "frames": [0, 1]}, "1": {"bbox": [[50, 70, 60, 70]] * 2, "frames": [1, 2]}}
    (tmp_path / "tracks.json").write_text(json.dumps(tracks))                 # frame 3 has nobody: encoded like any other
    demo.main(demo.parse_args(["--cfg", "configs/demo_poco_cliff_resnet50.yaml", "--ckpt", str(ckpt), "--mode", "video",
                               "--vid_file", str(fr_dir), "--batch_size", "5", "--smpl", str(smpl), "--tracking",
                               str(tmp_path / "tracks.json"), "--output_folder", str(tmp_path / "out"), "--render", "--sideview",
                               "--save_video", "--fps", "24", "--jpeg_quality", "80"]))
    out = tmp_path / "out" / "frames_"
    avi = parse_avi((out / "frames_poco_result.avi").read_bytes())
    assert len(avi["frames"]) == 4 and len(avi["idx1"]) == 4
    assert np.frombuffer(avi["avih"], "<u4")[[4, 8, 9]].tolist() == [4, 320, 120]
    for k in (0, 3):
        png = np.asarray(Image.open(out / "tmp_images_output" / f"{k:06d}.png"))     # the pictures stay .png by default
        assert png.shape == (120, 320, 3)
        assert avi["frames"][k][1] == jpeg_np.encode(png, 80)
        assert Image.open(io.BytesIO(avi["frames"][k][1])).size == (320, 120)
