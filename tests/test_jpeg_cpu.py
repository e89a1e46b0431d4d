"""CPU: the JPEG contract's numpy restatement (tests/jpeg_np.py) against PIL's libjpeg, the coverage of the fixture set the GPU
test compares bytes on, the Motion-JPEG .avi container of poco_amd/jpeg.py, and the argument errors that need no GPU."""
import ctypes as C
import io
import struct

import numpy as np
import pytest
from PIL import Image

from tests import jpeg_np

# PSNR of the restatement's decoded picture may fall below PIL's own encoder (quality q, 4:2:0, standard tables) by at most this.
# The arithmetic is libjpeg's, so on a picture of whole MCUs the decoded pixels are EQUAL (asserted below, gap 0).  On 120 x 168
# (7.5 x 10.5 MCUs) the two differ only in how the part outside the picture is filled (libjpeg: replication to whole blocks, then
# dummy blocks that repeat the DC; here: edge replication to whole MCUs): measured gap PIL - restatement over quality 50, 75, 90,
# 100 = -0.0179, +0.0015, -0.0070, -0.0007 dB.  Margin = twice the largest gap.
PSNR_MARGIN_DB = 0.0031


def photo_like(H, W, seed=0):
    """Smooth gradients + hard edges + noise."""
    r = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([128 + 100 * np.sin(x / 37.0) * np.cos(y / 23.0), 255.0 * x / W, 255.0 * y / H], -1)
    img[H // 4:H // 2, W // 3:2 * W // 3] = [250, 20, 30]
    img[(x + y) % 40 < 3] = [5, 5, 5]
    img += r.normal(0, 6, (H, W, 3))
    return np.clip(img, 0, 255).astype(np.uint8)


def psnr(a, b):
    return 10 * np.log10(255.0 ** 2 / np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2))


def decode(data: bytes) -> np.ndarray:
    im = Image.open(io.BytesIO(data))
    im.load()
    assert im.format == "JPEG" and im.mode == "RGB"
    return np.asarray(im)


def pil_encode(img, q):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=q, subsampling="4:2:0", optimize=False)
    return buf.getvalue()


def tables_of(data: bytes):
    """{(marker, table id byte): payload} of the DQT / DHT segments in front of SOS (a segment may hold several tables)."""
    out, i = {}, 2
    while data[i + 1] != 0xDA:
        m, n = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        p, j = data[i + 4:i + 2 + n], 0
        while m in (0xDB, 0xC4) and j < len(p):
            k = 65 if m == 0xDB else 17 + sum(p[j + 1:j + 17])
            out[(m, p[j])] = p[j:j + k]
            j += k
        i += 2 + n
    return out


def parse_avi(data: bytes):
    """A small RIFF reader: {"avih", "strh", "strf": payloads, "frames": [(offset of the chunk header, payload)], "idx1": [(ckid,
    flags, offset from the movi fourcc, size)], "movi": position of the movi fourcc}.  Asserts that chunk sizes add up."""
    assert data[:4] == b"RIFF" and data[8:12] == b"AVI " and struct.unpack("<I", data[4:8])[0] == len(data) - 8
    out = {"frames": []}

    def walk(lo, hi, in_movi):
        p = lo
        while p < hi:
            cid, n = data[p:p + 4], struct.unpack("<I", data[p + 4:p + 8])[0]
            assert p + 8 + n <= hi, (cid, p, n, hi)
            if cid == b"LIST":
                kind = data[p + 8:p + 12]
                if kind == b"movi":
                    out["movi"] = p + 8
                walk(p + 12, p + 8 + n, kind == b"movi")
            elif in_movi:
                assert cid == b"00dc"
                out["frames"].append((p, data[p + 8:p + 8 + n]))
            elif cid == b"idx1":
                out["idx1"] = [struct.unpack("<4sIII", data[q:q + 16]) for q in range(p + 8, p + 8 + n, 16)]
            else:
                out[cid.decode()] = data[p + 8:p + 8 + n]
            p += 8 + n + (n & 1)                                   # chunks are word-aligned
        assert p == hi, (p, hi)

    walk(12, len(data), False)
    return out


def test_restatement_decodes_with_size_and_mode():
    for H, W in ((8, 8), (33, 17), (120, 168)):
        img = photo_like(H, W, seed=H)
        data = jpeg_np.encode(img, 90)
        assert data[:2] == b"\xff\xd8" and data[-2:] == b"\xff\xd9"
        got = decode(data)
        assert got.shape == (H, W, 3)
        assert psnr(got, img) > 20
        assert len(data) <= jpeg_np.worst_case_bytes(H, W)


@pytest.mark.parametrize("q", [50, 75, 90, 100])
def test_psnr_against_pil(q):
    worst = -1e9
    for H, W in ((96, 128), (120, 168)):
        img = photo_like(H, W)
        mine, theirs = jpeg_np.encode(img, q), pil_encode(img, q)
        assert tables_of(mine) == tables_of(theirs)              # the quality-scaled DQT and the four Annex K DHT payloads
        dm, dp = decode(mine), decode(theirs)
        gap = psnr(dp, img) - psnr(dm, img)
        print(f"{H}x{W} q={q}: restatement {psnr(dm, img):.4f} dB, PIL {psnr(dp, img):.4f} dB, gap {gap:+.4f} dB")
        worst = max(worst, gap)
        if H % 16 == 0 and W % 16 == 0:
            assert np.array_equal(dm, dp)                        # same quantised coefficients: libjpeg's arithmetic exactly
        assert psnr(dm, img) >= psnr(dp, img) - PSNR_MARGIN_DB
    assert worst <= PSNR_MARGIN_DB


def test_fixture_set_covers_the_hard_cases():
    """The shapes x fills x qualities the GPU test compares bytes on must, taken together, contain ZRL symbols, EOB-only blocks,
    stuffed bytes, category >= 10 coefficients, more than 8 restart intervals (RSTm wraps) and an interval of more than 64 blocks."""
    tot = {"zrl": 0, "eob": 0, "eob_only_blocks": 0, "stuffed": 0, "max_category": 0, "intervals": 0, "max_interval_blocks": 0}
    for H, W in jpeg_np.FIXTURE_SHAPES:
        for fill in jpeg_np.FIXTURE_FILLS:
            for q in jpeg_np.FIXTURE_QUALITIES:
                data, st = jpeg_np.encode_stats(jpeg_np.fixture(fill, H, W), q)
                assert decode(data).shape == (H, W, 3)
                for k in ("zrl", "eob", "eob_only_blocks", "stuffed"):
                    tot[k] += st[k]
                for k in ("max_category", "intervals", "max_interval_blocks"):
                    tot[k] = max(tot[k], st[k])
    print(tot)
    assert tot["zrl"] > 0 and tot["eob"] > 0 and tot["eob_only_blocks"] > 0 and tot["stuffed"] > 0
    assert tot["max_category"] >= 10 and tot["intervals"] > 8 and tot["max_interval_blocks"] > 64


def test_restart_markers_count_modulo_8():
    data = jpeg_np.encode(jpeg_np.fixture("noise", 160, 48), 50)         # 10 intervals
    sos = data.index(b"\xff\xda")
    body = data[sos + 14:]
    marks = [body[i + 1] for i in range(len(body) - 1) if body[i] == 0xFF and body[i + 1] not in (0x00,)]
    assert marks == [0xD0 + (i & 7) for i in range(9)] + [0xD9]
    assert data[data.index(b"\xff\xdd") + 4:data.index(b"\xff\xdd") + 6] == (3).to_bytes(2, "big")   # DRI = MCUs per row


def test_mjpeg_writer_container(tmp_path):
    from poco_amd.jpeg import MjpegWriter
    H, W = 40, 56
    imgs = [photo_like(H, W, seed=s) for s in range(5)]
    frames = [jpeg_np.encode(im, 80 + s) for s, im in enumerate(imgs)]
    assert any(len(f) & 1 for f in frames) and any(not len(f) & 1 for f in frames)        # odd and even lengths
    path = tmp_path / "v.avi"
    w = MjpegWriter(str(path), W, H, fps=25)
    for f in frames:
        w.add(f)
    assert w.frames == 5
    w.close()
    w.close()                                                       # idempotent
    data = path.read_bytes()
    avi = parse_avi(data)
    avih = struct.unpack("<14I", avi["avih"])
    assert avih[0] == 40000 and avih[3] & 0x10 and avih[4] == 5 and avih[6] == 1 and avih[8:10] == (W, H)
    strh = struct.unpack("<4s4sIHHIIIIIIII4H", avi["strh"])
    assert strh[0] == b"vids" and strh[1] == b"MJPG" and strh[7] / strh[6] == 25 and strh[9] == 5
    strf = struct.unpack("<IiiHH4sIiiII", avi["strf"])
    assert strf[0] == 40 and strf[1:3] == (W, H) and strf[5] == b"MJPG"
    assert [p for _, p in avi["frames"]] == frames
    assert len(avi["idx1"]) == 5
    for (ckid, flags, off, size), (pos, payload) in zip(avi["idx1"], avi["frames"]):
        assert ckid == b"00dc" and flags & 0x10 and avi["movi"] + off == pos and size == len(payload)
        assert data[pos:pos + 4] == b"00dc" and pos % 2 == 0        # word-aligned: odd-length frames are padded
    for (_, payload), im in zip(avi["frames"], imgs):
        got = decode(payload)                                       # every frame decodes to the picture that went in
        assert got.shape == (H, W, 3) and psnr(got, im) > 20


def test_mjpeg_writer_argument_errors(tmp_path):
    from poco_amd import jpeg
    with pytest.raises(ValueError, match="width and height"):
        jpeg.MjpegWriter(str(tmp_path / "a.avi"), 0, 10)
    with pytest.raises(ValueError, match="fps"):
        jpeg.MjpegWriter(str(tmp_path / "a.avi"), 16, 16, fps=0)
    w = jpeg.MjpegWriter(str(tmp_path / "b.avi"), 16, 16)
    with pytest.raises(ValueError, match="JPEG"):
        w.add(b"not a jpeg")
    frame = jpeg_np.encode(np.zeros((16, 16, 3), np.uint8), 50)
    w.add(frame)
    # files above 2 GB are refused with a clear error (the limit is lowered instead of writing 2 GB)
    old, jpeg.AVI_MAX_BYTES = jpeg.AVI_MAX_BYTES, w._pos + 8 + len(frame) + (len(frame) & 1) + 8 + 16 * 2
    try:
        with pytest.raises(ValueError, match="2 GB"):
            w.add(frame + b"\0\0")
        w.add(frame)                                                # exactly at the limit still fits
    finally:
        jpeg.AVI_MAX_BYTES = old
    w.close()
    assert len(parse_avi((tmp_path / "b.avi").read_bytes())["frames"]) == 2
    with pytest.raises(ValueError, match="close"):
        w.add(frame)


def test_encoder_argument_errors_without_gpu():
    """Bad sizes are refused before any GPU work, by the wrapper and by the C entry; the worst-case bound is the documented one."""
    from poco_amd import jpeg
    from poco_amd._lib import PocoHipError, lib
    for h, w in ((0, 16), (16, 0), (16385, 16), (16, 16385)):
        with pytest.raises(PocoHipError, match="max_h, max_w"):
            jpeg.JpegEncoder(None, h, w)
    L = lib()
    assert hasattr(L, "poco_jpeg_encode") and hasattr(L, "poco_jpeg_encoder_destroy")
    L.poco_jpeg_encoder_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    assert L.poco_jpeg_encoder_create(0, 16, C.byref(h)) == 1 and not h.value
    assert L.poco_jpeg_encoder_create(16, 16385, C.byref(h)) == 1 and not h.value
    assert L.poco_jpeg_encoder_create(16, 16, None) == 1
    assert b"max_h" in L.poco_last_error() or b"null" in L.poco_last_error()
    L.poco_jpeg_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    assert L.poco_jpeg_encode(None, None, 16, 16, 90, None, 0, None, None) == 1
    assert jpeg.worst_case_bytes(1080, 1920) == jpeg_np.worst_case_bytes(1080, 1920) == 629 + 68 * (120 * 2592 + 2)
    assert jpeg.HEADER_BYTES == len(jpeg_np.header(33, 17, 50))


def test_demo_flags():
    import demo
    base = ["--cfg", "c.yaml", "--ckpt", "x.pt"]
    a = demo.parse_args(base)
    assert a.image_format == "png" and a.jpeg_quality == 90 and not a.save_video and a.fps == 30
    a = demo.parse_args(base + ["--image_format", "jpg", "--jpeg_quality", "75", "--save_video", "--fps", "24"])
    assert a.image_format == "jpg" and a.jpeg_quality == 75 and a.save_video and a.fps == 24
    with pytest.raises(SystemExit):
        demo.parse_args(base + ["--image_format", "bmp"])
    with pytest.raises(SystemExit, match="--save_video"):
        demo.main(demo.parse_args(base + ["--save_video", "--mode", "video"]))       # without --render
