"""GPU: demo.py --decode gpu and --vid_file movie.avi end to end on a synthetic checkpoint: the same .npz contents and rendered
.png bytes as the default host decode, for folders of .jpg (mixed with .png and a progressive .jpg) and for a Motion-JPEG .avi."""
import io
import json

import numpy as np
import pytest
import torch
from PIL import Image

from poco_amd import jpeg, synth
from tests import util
from tests.test_jpeg_cpu import photo_like

pytestmark = pytest.mark.gpu

CFG = "configs/demo_poco_cliff_resnet50.yaml"


def _assets(tmp_path, variant="resnet50-cliff"):
    """The synthetic checkpoint and body model of tests/test_demo_gpu.py / tests/test_jpeg_gpu.py."""
    w = util.synth_weights(variant)
    ckpt = tmp_path / "poco_synth.pt"
    torch.save({"state_dict": {"model." + k: torch.from_numpy(v) for k, v in w.items()}}, ckpt)
    smpl = synth.synth_smpl(7)
    smpl["faces"] = np.stack([np.arange(0, 3000), np.arange(1, 3001), np.arange(2, 3002)], 1).astype(np.int32)
    np.savez(tmp_path / "smpl.npz", **smpl)
    return ckpt, tmp_path / "smpl.npz"


def _jpg(img, **kw):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", **kw)
    return buf.getvalue()


def _same_npz(a, b):
    with np.load(a) as x, np.load(b) as y:
        assert sorted(x.files) == sorted(y.files) and x.files
        for k in x.files:
            assert np.array_equal(x[k], y[k]), (a.name, k)


def _record_decodes(monkeypatch):
    """{frame name: whether decode_frames returned it as a device tensor}, filled while demo.main runs."""
    from poco_amd.tester import POCOTester
    seen, inner = {}, POCOTester.decode_frames

    def decode_frames(self, named):
        out = inner(self, named)
        seen.update({n: torch.is_tensor(f) and f.is_cuda and f.dtype == torch.uint8 for (n, _), f in zip(named, out)})
        return out
    monkeypatch.setattr(POCOTester, "decode_frames", decode_frames)
    return seen


def test_folder_decode_gpu_equals_host(tmp_path, cuda, monkeypatch):
    import demo
    ckpt, smpl = _assets(tmp_path)
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    sizes = [(200, 300), (240, 320), (200, 300), (96, 128), (180, 260), (368, 368)]
    kinds = [dict(quality=90), dict(quality=75, subsampling="4:4:4", optimize=True), None, dict(quality=85, progressive=True),
             dict(quality=95, subsampling="4:2:2", restart_marker_rows=1),
             dict(quality=50, subsampling="4:4:4", restart_marker_blocks=1)]       # 46 x 46 intervals: more than a decoder plans
    names = []
    for i, ((h, w), kw) in enumerate(zip(sizes, kinds)):
        fr = photo_like(h, w, seed=40 + i)
        if kw is None:
            names.append(f"im{i}.png")
            Image.fromarray(fr).save(imgs / names[-1])
        else:
            names.append(f"im{i}.jpg")
            (imgs / names[-1]).write_bytes(_jpg(fr, **kw))
    assert jpeg.parse_jpeg((imgs / "im3.jpg").read_bytes()) is None and jpeg.parse_jpeg((imgs / "im0.jpg").read_bytes()) is not None
    dets = {"im0.jpg": [[200, 100, 120, 160]], "im1.jpg": [[160, 120, 150, 150], [80, 100, 90, 120]], "im4.jpg": [[130, 90, 100, 140]]}
    (tmp_path / "dets.json").write_text(json.dumps(dets))
    common = ["--cfg", CFG, "--ckpt", str(ckpt), "--mode", "folder", "--image_folder", str(imgs), "--batch_size", "4", "--smpl",
              str(smpl), "--detections", str(tmp_path / "dets.json"), "--render"]
    demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "host")]))
    assert len(jpeg.parse_jpeg((imgs / "im5.jpg").read_bytes()).segments) > jpeg.SEGS_PER_IMAGE
    seen = _record_decodes(monkeypatch)
    with pytest.warns(UserWarning, match=r"--decode gpu: im5\.jpg: more than 2048 restart intervals") as rec:
        demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "gpu"), "--decode", "gpu"]))
    assert sum("--decode gpu" in str(w.message) for w in rec) == 1
    # the baseline files came back from the device decoder; only the .png, the progressive file and im5 went through PIL
    assert seen == {"im0.jpg": True, "im1.jpg": True, "im2.png": False, "im3.jpg": False, "im4.jpg": True, "im5.jpg": False}
    for n in names:
        stem = n.rsplit(".", 1)[0]
        _same_npz(tmp_path / "host" / "imgs_" / (stem + "_poco.npz"), tmp_path / "gpu" / "imgs_" / (stem + "_poco.npz"))
        a = tmp_path / "host" / "imgs_" / "poco_results" / (stem + ".png")
        b = tmp_path / "gpu" / "imgs_" / "poco_results" / (stem + ".png")
        assert a.read_bytes() == b.read_bytes(), n


@pytest.mark.parametrize("decode", ["host", "gpu"])
def test_avi_equals_the_folder_of_frames(tmp_path, cuda, decode, monkeypatch):
    import demo
    seen = _record_decodes(monkeypatch)
    ckpt, smpl = _assets(tmp_path)
    fr_dir = tmp_path / "frames"
    fr_dir.mkdir()
    frames = [_jpg(photo_like(120, 160, seed=60 + i), quality=88) for i in range(6)]
    with jpeg.MjpegWriter(str(tmp_path / "movie.avi"), 160, 120, fps=25) as w:
        for i, f in enumerate(frames):
            (fr_dir / f"{i + 1:06d}.jpg").write_bytes(f)
            w.add(f)
    tracks = {"0": {"bbox": [[80, 60, 80, 80]] * 4, "frames": [0, 1, 2, 3]}, "1": {"bbox": [[50, 70, 60, 70]] * 4, "frames": [2, 3, 4, 5]}}
    (tmp_path / "tracks.json").write_text(json.dumps(tracks))
    for skip in ("1", "2"):
        common = ["--cfg", CFG, "--ckpt", str(ckpt), "--mode", "video", "--batch_size", "5", "--smpl", str(smpl), "--tracking",
                  str(tmp_path / "tracks.json"), "--render", "--skip_frame", skip, "--decode", decode]
        demo.main(demo.parse_args(common + ["--vid_file", str(fr_dir), "--output_folder", str(tmp_path / ("dir" + skip))]))
        demo.main(demo.parse_args(common + ["--vid_file", str(tmp_path / "movie.avi"), "--output_folder", str(tmp_path / ("avi" + skip))]))
        a, b = tmp_path / ("dir" + skip) / "frames_", tmp_path / ("avi" + skip) / "movie_"
        _same_npz(a / "poco_results.npz", b / "poco_results.npz")
        if decode == "gpu":          # every frame the runs read (those of the tracks at least) came back from the device decoder
            assert {"000001.jpg", "000003.jpg", "000005.jpg"} <= set(seen) and all(seen.values()), seen
        else:
            assert seen == {}
        for i in range(6):
            assert (a / "tmp_images_output" / f"{i:06d}.png").read_bytes() == (b / "tmp_images_output" / f"{i:06d}.png").read_bytes()


def test_other_containers_are_refused(tmp_path):
    import demo
    (tmp_path / "clip.mp4").write_bytes(b"\0\0\0\x18ftypmp42" + bytes(64))
    with pytest.raises(SystemExit, match="only Motion-JPEG AVI is read.*folder"):
        demo.main(demo.parse_args(["--cfg", CFG, "--ckpt", "x.pt", "--mode", "video", "--vid_file", str(tmp_path / "clip.mp4")]))
