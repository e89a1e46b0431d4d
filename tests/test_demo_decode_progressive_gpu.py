"""GPU: demo.py --decode_progressive gpu end to end on a synthetic checkpoint: a folder of baseline .jpg, progressive .jpg and .png
files gives the same .npz contents and rendered .png bytes as the default host decode; the progressive files are decoded on the
device with the flag and by PIL without it.  A file with a scan script PIL never writes (DC scans of one component) goes to the
device too; one whose script ends above Al = 0 - libjpeg smooths its blocks - is PIL's under every setting."""
import warnings

from poco_amd import jpeg
from tests import jpegprog_cases as K
from tests.test_demo_decode_gpu import _assets, _jpg, _record_decodes
from tests.test_demo_decode_png_gpu import _folder_args, _same_outputs
from tests.test_jpeg_cpu import photo_like
from tests.test_pngdec_cpu import pil_png

import pytest

pytestmark = pytest.mark.gpu


def test_folder_decode_progressive_gpu_equals_host(tmp_path, cuda, monkeypatch):
    import demo
    ckpt, smpl = _assets(tmp_path)
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    files = {"im0.jpg": K.encode(photo_like(200, 300, 40), "420", quality=85),
             "im1.jpg": K.encode(photo_like(240, 320, 41), "444", quality=90, optimize=True),
             "im2.jpg": K.encode(photo_like(96, 128, 42), "grey", quality=75),
             "im3.jpg": _jpg(photo_like(180, 260, 45), quality=90),
             "im4.png": pil_png(photo_like(120, 160, 44))}
    for n, d in files.items():
        (imgs / n).write_bytes(d)
    prog = {n: jpeg.parse_progressive_jpeg(d) is not None for n, d in files.items()}
    assert prog == {"im0.jpg": True, "im1.jpg": True, "im2.jpg": True, "im3.jpg": False, "im4.png": False}
    assert jpeg.parse_jpeg(files["im3.jpg"]) is not None
    common = _folder_args(tmp_path, ckpt, smpl, imgs, {"im0.jpg": [[200, 100, 120, 160]], "im1.jpg": [[160, 120, 150, 150], [80, 100, 90, 120]]})
    demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "host")]))
    seen = _record_decodes(monkeypatch)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "prog"), "--decode", "gpu", "--decode_progressive", "gpu"]))
        assert seen == {**prog, "im3.jpg": True}                        # progressive and baseline on the device, the .png by PIL
        seen.clear()
        demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "only"), "--decode_progressive", "gpu"]))
        assert seen == prog
        seen.clear()
        demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "base"), "--decode", "gpu", "--decode_progressive", "host"]))
        assert seen == {n: n == "im3.jpg" for n in files}               # the progressive files are PIL's again
    for out in ("prog", "only", "base"):
        _same_outputs(tmp_path, "host", out, files)


def test_folder_with_unusual_scan_scripts_equals_host(tmp_path, cuda, monkeypatch):
    import demo
    from tests.jpegprog_enc_np import rescan
    ckpt, smpl = _assets(tmp_path)
    imgs = tmp_path / "imgs"
    imgs.mkdir()
    src = K.encode(photo_like(200, 300, 46), "420", quality=85)
    files = {"im0.jpg": rescan(src, K.scripts(3)["dc-split"]),
             "im1.jpg": K.cut_after(K.encode(photo_like(240, 320, 47), "420", quality=90), 5)}
    for n, d in files.items():
        (imgs / n).write_bytes(d)
    prog = {n: jpeg.parse_progressive_jpeg(d) is not None for n, d in files.items()}
    assert prog == {"im0.jpg": True, "im1.jpg": False}
    assert (K.reference(files["im0.jpg"]) == K.reference(src)).all()
    common = _folder_args(tmp_path, ckpt, smpl, imgs, {"im0.jpg": [[200, 100, 120, 160]], "im1.jpg": [[160, 120, 150, 150]]})
    demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "host")]))
    seen = _record_decodes(monkeypatch)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        demo.main(demo.parse_args(common + ["--output_folder", str(tmp_path / "prog"), "--decode_progressive", "gpu"]))
    assert seen == prog                                                 # the declined file came back from PIL
    _same_outputs(tmp_path, "host", "prog", files)
