"""GPU: demo.py --decode_png gpu end to end on a synthetic checkpoint: the same .npz contents and rendered .png bytes as the default
host decode, for a folder of mixed files, for a frames folder in video mode (group load) and with a damaged .png in the folder."""
import io
import json
import warnings
import zlib

import numpy as np
import pytest
from PIL import Image

from poco_amd import png
from tests.test_demo_decode_gpu import CFG, _assets, _jpg, _record_decodes, _same_npz
from tests.test_jpeg_cpu import photo_like
from tests.test_pngdec_cpu import assemble, filter_stream, make_png, pil_png

pytestmark = pytest.mark.gpu


def _folder_args(tmp_path, ckpt, smpl, imgs, dets):
    (tmp_path / "dets.json").write_text(json.dumps(dets))
    return ["--cfg", CFG, "--ckpt", str(ckpt), "--mode", "folder", "--image_folder", str(imgs), "--batch_size", "4", "--smpl",
            str(smpl), "--detections", str(tmp_path / "dets.json"), "--render"]


def _same_outputs(tmp_path, a, b, names):
    for n in names:
        stem = n.rsplit(".", 1)[0]
        _same_npz(tmp_path / a / "imgs_" / (stem + "_poco.npz"), tmp_path / b / "imgs_" / (stem + "_poco.npz"))
        x = tmp_path / a / "imgs_" / "poco_results" / (stem + ".png")
        y = tmp_path / b / "imgs_" / "poco_results" / (stem + ".png")
        assert x.read_bytes() == y.read_bytes(), n


def test_folder_decode_png_gpu_equals_host(tmp_path, cuda, monkeypatch):
    import demo
    ckpt, smpl = _assets(tmp_path)
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    rng = np.random.default_rng(3)
    grey16 = (np.arange(96 * 128, dtype=np.uint16).reshape(96, 128) * 5)
    buf = io.BytesIO()
    Image.fromarray(grey16).save(buf, "PNG")
    files = {"im0.png": pil_png(photo_like(200, 300, 40)),
             "im1.png": make_png(photo_like(240, 320, 41), 2, filters=[4]),
             "im2.png": make_png(rng.integers(0, 7, (96, 128), dtype=np.uint8), 3, filters=[0],
                                 palette=rng.integers(0, 256, 21, dtype=np.uint8).tobytes()),
             "im3.png": buf.getvalue(),
             "im4.png": adam7_png(photo_like(120, 160, 44)),
             "im5.jpg": _jpg(photo_like(180, 260, 45), quality=90)}
    for n, d in files.items():
        (imgs / n).write_bytes(d)
    accepted = {n: n.endswith(".png") and png.parse_png(d) is not None for n, d in files.items()}
    assert accepted == {"im0.png": True, "im1.png": True, "im2.png": True, "im3.png": False, "im4.png": False, "im5.jpg": False}
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(files["im4.png"])).convert("RGB")), photo_like(120, 160, 44))
    common = _folder_args(tmp_path, ckpt, smpl, imgs, {"im0.png": [[200, 100, 120, 160]], "im1.png": [[160, 120, 150, 150], [80, 100, 90, 120]]})
    demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "host")]))
    seen = _record_decodes(monkeypatch)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "png"), "--decode_png", "gpu"]))
        assert seen == accepted
        seen.clear()
        demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "both"), "--decode", "gpu", "--decode_png", "gpu"]))
        assert seen == {**accepted, "im5.jpg": True}
    _same_outputs(tmp_path, "host", "png", files)
    _same_outputs(tmp_path, "host", "both", files)


def adam7_png(img: np.ndarray) -> bytes:
    """An interlaced 8-bit RGB PNG (the seven Adam7 passes, filter 0), which PIL reads and parse_png declines."""
    H, W = img.shape[:2]
    raw = bytearray()
    for y0, x0, dy, dx in ((0, 0, 8, 8), (0, 4, 8, 8), (4, 0, 8, 4), (0, 2, 4, 4), (2, 0, 4, 2), (0, 1, 2, 2), (1, 0, 2, 1)):
        sub = img[y0::dy, x0::dx]
        if sub.size:
            raw += filter_stream(sub.reshape(sub.shape[0], -1), 3, [0])
    return assemble(H, W, 2, zlib.compress(bytes(raw)), interlace=1)


def test_video_decode_png_gpu_equals_host(tmp_path, cuda, monkeypatch):
    import demo
    from poco_amd.tester import POCOTester
    ckpt, smpl = _assets(tmp_path)
    fr_dir = tmp_path / "frames"
    fr_dir.mkdir()
    for i in range(6):
        (fr_dir / f"{i + 1:06d}.png").write_bytes(pil_png(photo_like(120, 160, seed=60 + i)))
    tracks = {"0": {"bbox": [[80, 60, 80, 80]] * 4, "frames": [0, 1, 2, 3]}, "1": {"bbox": [[50, 70, 60, 70]] * 4, "frames": [2, 3, 4, 5]}}
    (tmp_path / "tracks.json").write_text(json.dumps(tracks))
    seen = _record_decodes(monkeypatch)
    sizes, inner = [], POCOTester.decode_frames

    def counting(self, named):
        sizes.append(len(named))
        return inner(self, named)
    monkeypatch.setattr(POCOTester, "decode_frames", counting)
    for skip in ("1", "2"):
        common = ["--cfg", CFG, "--ckpt", str(ckpt), "--mode", "video", "--batch_size", "5", "--smpl", str(smpl), "--tracking",
                  str(tmp_path / "tracks.json"), "--render", "--skip_frame", skip, "--vid_file", str(fr_dir)]
        demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / ("host" + skip))]))
        assert seen == {} and sizes == []
        demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / ("gpu" + skip)), "--decode_png", "gpu"]))
        a, b = tmp_path / ("host" + skip) / "frames_", tmp_path / ("gpu" + skip) / "frames_"
        _same_npz(a / "poco_results.npz", b / "poco_results.npz")
        for i in range(6):
            assert (a / "tmp_images_output" / f"{i:06d}.png").read_bytes() == (b / "tmp_images_output" / f"{i:06d}.png").read_bytes()
        assert set(seen) == {f"{i + 1:06d}.png" for i in range(6)} and all(seen.values()), seen
        assert max(sizes) > 1 and max(sizes) <= 5, sizes                # the group load
        seen.clear()
        sizes.clear()


def test_damaged_png_in_the_folder(tmp_path, cuda, monkeypatch):
    """The one-row-short stream: PIL still opens it (the missing row stays black), the device reports it."""
    import demo
    ckpt, smpl = _assets(tmp_path)
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    photo = photo_like(120, 168, 11)
    raw = filter_stream(photo.reshape(120, 168 * 3), 3, [4])
    short = assemble(120, 168, 2, zlib.compress(raw[:-(1 + 168 * 3)]))
    assert png.parse_png(short) is not None and Image.open(io.BytesIO(short)).convert("RGB").size == (168, 120)
    (imgs / "a.png").write_bytes(pil_png(photo_like(96, 128, 50)))
    (imgs / "b.png").write_bytes(short)
    common = _folder_args(tmp_path, ckpt, smpl, imgs, {})
    demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "host")]))
    seen = _record_decodes(monkeypatch)
    with pytest.warns(UserWarning, match=r"--decode_png gpu: b\.png is damaged \(status \d+\); decoding it with PIL") as rec:
        demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "gpu"), "--decode_png", "gpu"]))
    assert sum("--decode_png gpu" in str(w.message) for w in rec) == 1
    assert seen == {"a.png": True, "b.png": False}
    _same_outputs(tmp_path, "host", "gpu", ["a.png", "b.png"])
