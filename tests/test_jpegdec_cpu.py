"""The baseline JPEG decoder's contract without a GPU: the numpy restatement (tests/jpegdec_np.py) against PIL BYTE for byte on a
fixture set whose coverage is asserted, the same on the streams libjpeg's writer never makes (tests/jpegdec_cases.py),
parse_jpeg's refusals, damaged streams, and MjpegReader against MjpegWriter."""
import ctypes as C
import functools
import io
import struct

import numpy as np
import pytest
from PIL import Image

from poco_amd import jpeg
from tests import jpeg_np, jpegdec_cases, jpegdec_np
from tests.jpegbase_enc_np import recode
from tests.test_jpeg_cpu import photo_like

SIZES = [(1, 1), (8, 8), (17, 33), (96, 128), (120, 168), (24, 700)]         # H x W
SAMPLINGS = ["4:4:4", "4:2:2", "4:2:0", "gray"]


def pil_jpeg(img, sampling, quality, **kw):
    buf = io.BytesIO()
    if sampling == "gray":
        Image.fromarray(np.ascontiguousarray(img[..., 1])).save(buf, "JPEG", quality=quality, **kw)
    else:
        Image.fromarray(img).save(buf, "JPEG", quality=quality, subsampling=sampling, **kw)
    return buf.getvalue()


def pil_pixels(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def noise(H, W, seed):
    return np.random.default_rng(seed).integers(0, 256, (H, W, 3), dtype=np.uint8)


def strip_dht(data: bytes) -> bytes:
    """The same file without its DHT segments (what Motion-JPEG frames inside AVI look like)."""
    out, i = bytearray(data[:2]), 2
    while data[i + 1] != 0xDA:
        n = int.from_bytes(data[i + 2:i + 4], "big")
        if data[i + 1] != 0xC4:
            out += data[i:i + 2 + n]
        i += 2 + n
    return bytes(out + data[i:])


@functools.lru_cache(maxsize=None)
def fixture_set():
    """{name: bytes}.  Every size with every sampling (the options rotate so that each kind of stream is there at several
    sizes), the thresholds of the fancy filters (chroma widths 2 and 3), this project's own encoder, a frame without DHT, and
    two noise pictures without restart markers: 16+ subsequences, and a lane that needs more than one round."""
    opts = [dict(), dict(optimize=True), dict(restart_marker_rows=1), dict(restart_marker_blocks=3)]
    quals = [30, 75, 95, 100]
    out, k = {}, 0
    for (H, W) in SIZES:
        img = photo_like(H, W, seed=H * 1000 + W)
        for s in SAMPLINGS:
            for j in range(2):
                o, q = opts[(k + j) % 4], quals[(k // 2 + j) % 4]
                out[f"{H}x{W}_{s}_q{q}_{'_'.join(o) or 'plain'}"] = pil_jpeg(img, s, q, **o)
            k += 1
    for (H, W) in [(4, 4), (6, 5), (5, 6), (2, 40), (40, 3)]:
        for s in ("4:2:2", "4:2:0"):
            out[f"{H}x{W}_{s}_edge"] = pil_jpeg(photo_like(H, W, seed=H + W), s, 90)
    for (H, W) in [(33, 17), (48, 208)]:
        out[f"{H}x{W}_own_encoder"] = jpeg_np.encode(jpeg_np.fixture("noise", H, W), 100)
        out[f"{H}x{W}_own_encoder_gradient"] = jpeg_np.encode(jpeg_np.fixture("gradient", H, W), 50)
    out["96x128_no_dht"] = strip_dht(pil_jpeg(photo_like(96, 128, 5), "4:2:0", 75))
    out["64x96_noise_q100"] = pil_jpeg(noise(64, 96, 7), "4:4:4", 100)
    out["120x168_noise_q30"] = pil_jpeg(noise(120, 168, 8), "4:2:0", 30)
    out["64x2048_noise_q95"] = pil_jpeg(noise(64, 2048, 9), "4:2:0", 95)
    return out


@functools.lru_cache(maxsize=None)
def restated(name):
    """(pixels, stats) of the restatement, computed once and shared with tests/test_jpegdec_gpu.py."""
    px, st = jpegdec_np.decode_stats(fixture_set()[name])
    px.setflags(write=False)
    return px, st


@pytest.mark.parametrize("name", list(fixture_set()))
def test_restatement_equals_pil(name):
    data = fixture_set()[name]
    ref = pil_pixels(data)
    got = restated(name)[0]
    assert got.shape == ref.shape and got.dtype == np.uint8
    assert np.array_equal(got, ref), (name, np.argwhere(got != ref)[:4].tolist())


def test_fixture_set_covers_the_hard_cases():
    fs = fixture_set()
    st = {n: restated(n)[1] for n in fs}
    assert sum(s["stuffed"] for s in st.values()) > 0
    assert sum(s["zrl"] for s in st.values()) > 0 and sum(s["eob"] for s in st.values()) > 0
    assert sum(s["long_codes"] for s in st.values()) > 0                      # codes longer than the lookahead table
    assert max(s["max_category"] for s in st.values()) >= 10
    infos = {n: jpeg.parse_jpeg(d) for n, d in fs.items()}
    assert all(i is not None for i in infos.values())
    assert {(i.ncomp, i.hsamp, i.vsamp) for i in infos.values()} == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    assert any(len(i.segments) > 8 and i.restart_interval == 3 for i in infos.values())         # RSTm wraps, intervals end mid-row
    assert any(len(i.segments) == 1 and i.segments[0, 1] >= 16 * jpeg.SUBSEQ_BYTES for i in infos.values())
    assert any(len(i.segments) == 1 and i.segments[0, 1] > 256 * jpeg.SUBSEQ_BYTES for i in infos.values())   # more than one block's lanes
    assert any(i.dc[0] == jpeg.ANNEX_K_TABLES[(0, 0)] and b"\xff\xc4" not in fs[n][:i.scan_offset] for n, i in infos.items())
    rounds = {n: jpegdec_np.sync_rounds(fs[n]) for n in ("64x96_noise_q100", "120x168_noise_q30")}
    assert max(rounds.values()) >= 2, rounds                                   # the synchronisation loop is exercised
    assert all(jpegdec_np.sync_rounds(d) == 1 for n, d in fs.items() if n.startswith("1x1_"))      # one subsequence: nothing to guess


@functools.lru_cache(maxsize=None)
def hand_restated(name):
    """(pixels, stats) of the restatement for a hand case, computed once and shared with tests/test_jpegdec_gpu.py."""
    px, st = jpegdec_np.decode_stats(jpegdec_cases.hand_cases()[name])
    px.setflags(write=False)
    return px, st


@pytest.mark.parametrize("name", list(jpegdec_cases.hand_cases()))
def test_hand_case_equals_pil(name):
    data = jpegdec_cases.hand_cases()[name]
    assert jpeg.parse_jpeg(data) is not None
    ref = pil_pixels(data)
    got = hand_restated(name)[0]
    assert got.shape == ref.shape and got.dtype == np.uint8
    assert np.array_equal(got, ref), (name, np.argwhere(got != ref)[:4].tolist())


def test_transcoder_keeps_the_pixels():
    """Without `edit` a recoded file is the source's picture, whatever the tables, ids, restart interval and DHT layout."""
    for k, s in enumerate(("420", "422", "444", "grey")):
        src = jpegdec_cases.source(s, 13, 17)
        ref = pil_pixels(src)
        for j, (t, ids) in enumerate((t, i) for t in jpegdec_cases.TABLES for i in jpegdec_cases.IDS):
            out = recode(src, t, ids, (0, 1, 2, 5)[(j + k) % 4], dht=("each", "joined")[j & 1])
            assert np.array_equal(pil_pixels(out), ref), (s, t, ids)
    assert recode(src, "flat", dht="each").count(b"\xff\xc4") == 2 and recode(src, "flat", dht="joined").count(b"\xff\xc4") == 1
    with pytest.raises(AssertionError, match="DC difference"):
        recode(src, edit=[(0, 0, 1500), (1, 0, -1500)])
    with pytest.raises(AssertionError, match="AC coefficient"):
        recode(src, edit=[(0, 5, 1024)])


def test_hand_cases_cover_what_libjpeg_never_writes():
    """Each property on the case named for it.  Of these the old fixture set has no symbol 0xFA, no three ZRLs in front of
    coefficient 63, no positive DC difference of category 11, no DC code longer than 10 bits, one table id layout only, and
    at most 59 rounds of synchronisation; its boundary properties are there, but by luck."""
    hc = jpegdec_cases.hand_cases()
    st = {n: hand_restated(n)[1] for n in hc}
    infos = {n: jpeg.parse_jpeg(d) for n, d in hc.items()}
    assert len(set(hc.values())) == len(hc)
    assert all(i.height <= 150 and i.width <= 200 for i in infos.values())
    # tables: every deep stream uses 16-bit codes, and under every id layout one uses every length 10 .. 16 for DC and for AC
    deep = [n for n in hc if "deep" in n]
    assert len(deep) >= 12 and all(st[n]["max_code_len"] == 16 for n in deep)
    every = set(range(10, 17))
    for ids in jpegdec_cases.IDS:
        assert st[f"tables-deep-{ids}-420-33x47"]["dc_code_lens"] == every == st[f"tables-deep-{ids}-420-33x47"]["ac_code_lens"]
    assert all(st[n]["max_code_len"] == 9 and st[n]["long_codes"] == 0 for n in hc if "flat" in n)
    # table ids: whichever id carries it, luma gets the table made from luma's symbols (shared and swapped parse alike, from
    # different scan headers); per_component gives three different tables of each class
    def layout(i):
        return tuple(i.dc.index(t) for t in i.dc), tuple(i.ac.index(t) for t in i.ac)
    for s in ("420", "444"):
        for t in jpegdec_cases.TABLES:
            i3 = {ids: infos[f"tables-{t}-{ids}-{s}-33x47"] for ids in jpegdec_cases.IDS}
            assert i3["shared"].dc == i3["swapped"].dc and i3["shared"].ac == i3["swapped"].ac
            if t != "flat":                                # (flat tables are the same table under every id)
                assert layout(i3["shared"]) == ((0, 1, 1), (0, 1, 1)) and layout(i3["per_component"]) == ((0, 1, 2), (0, 1, 2))
                assert i3["shared"].dc[1] != i3["per_component"].dc[1] and i3["shared"].ac[1] != i3["per_component"].ac[1]
    ids_seen = set()
    for n, d in hc.items():
        k = d.index(b"\xff\xda")
        ids_seen.add(tuple(d[k + 6 + 2 * c] for c in range(d[k + 4])))
    assert {(0x00, 0x11, 0x11), (0x11, 0x00, 0x00), (0x00, 0x11, 0x33), (0x00,), (0x11,)} <= ids_seen
    # restart intervals
    assert infos["dri1-420-33x47"].restart_interval == 1 and len(infos["dri1-420-33x47"].segments) == 9 > 8
    assert len(infos["dri1-noise"].segments) == 192 and len(infos["dri1-444-200x120"].segments) == 375 >= 256
    assert len(infos["dri1-deep-per_component-444-200x120"].segments) >= 256 and st["dri1-deep-per_component-444-200x120"]["max_code_len"] == 16
    assert max(infos["dri1-444-200x120"].segments[:, 1]) < jpeg.SUBSEQ_BYTES                   # far shorter than a subsequence
    assert infos["dri7-noise"].restart_interval == 7 and len(infos["dri7-noise"].segments) == 28 > 8              # RSTm wraps
    assert infos["dri-whole-420-33x47"].restart_interval == 9 and len(infos["dri-whole-420-33x47"].segments) == 1
    assert b"\xff\xdd" in hc["dri-whole-420-33x47"] and b"\xff\xd0" not in hc["dri-whole-420-33x47"]
    # subsequence boundaries
    for prop, name in jpegdec_cases.BOUNDARY.items():
        assert st[name][prop] > 0, (prop, name)
        if prop in jpegdec_cases.LATER_INTERVAL:
            assert st[name]["later_intervals"][prop] > 0 and min(infos[name].segments[:, 1]) > jpeg.SUBSEQ_BYTES, (prop, name)
    assert "deep" in jpegdec_cases.BOUNDARY["long_symbol_straddles"]
    # extremes
    for n in ("extreme-dc11-checkerboard", "extreme-dc11-checkerboard-deep"):
        assert st[n]["max_dc_category"] == 11 and st[n]["dc11_signs"] == {1, -1}, n
    for n in ("extreme-edited-blocks", "extreme-edited-blocks-deep"):
        assert st[n]["sym_fa"] >= 4 and st[n]["zrl3_then_63"] >= 2 and st[n]["full_blocks"] > 2 and st[n]["max_category"] == 10, n
    # ... none of which the old set has
    old = [restated(n)[1] for n in fixture_set()]
    assert sum(s["sym_fa"] + s["zrl3_then_63"] for s in old) == 0 and all(1 not in s["dc11_signs"] for s in old)
    assert max(max(s["dc_code_lens"]) for s in old) <= 10


def test_slow_synchronisation_case():
    """The flat-table noise stream needs more rounds than anything in the old fixture set, and no fewer than when it was written."""
    rounds = jpegdec_np.sync_rounds(jpegdec_cases.hand_cases()["slow-sync"])
    print("sync_rounds of slow-sync:", rounds)
    assert rounds >= jpegdec_cases.SLOW_SYNC_ROUNDS
    old = max(jpegdec_np.sync_rounds(d) for d in fixture_set().values())
    print("the old fixture set's maximum:", old)
    assert rounds > old


def test_unowned_code_is_reported():
    """Sixteen 1-bits where a symbol starts: the restatement names that byte."""
    bad, bp = jpegdec_cases.unowned_code(jpegdec_cases.hand_cases()["tables-deep-per_component-444-33x47"])
    info = jpeg.parse_jpeg(bad)
    assert info is not None and bp - info.scan_offset >= 2 * jpeg.SUBSEQ_BYTES
    with pytest.raises(jpegdec_np.JpegError, match=f"no Huffman code at byte {bp}$"):
        jpegdec_np.decode(bad)


def test_parse_jpeg_fields():
    data = pil_jpeg(photo_like(40, 56, 1), "4:2:0", 75, restart_marker_rows=1)
    i = jpeg.parse_jpeg(data)
    assert (i.height, i.width, i.ncomp, i.hsamp, i.vsamp, i.restart_interval) == (40, 56, 3, 2, 2, 4) and i.mcus == (3, 4)
    assert i.qt.shape == (3, 64) and i.qt.dtype == np.uint16 and len(i.dc) == len(i.ac) == 3
    assert i.segments.tolist() == [[o, n, m] for o, n, m in i.segments.tolist()] and i.segments[:, 2].tolist() == [0, 4, 8]
    scan = data[i.scan_offset:i.scan_offset + i.scan_length]
    assert data[i.scan_offset + i.scan_length:] == b"\xff\xd9"
    for (o, n, _), nxt in zip(i.segments.tolist(), [0xD0, 0xD1, 0xD9]):
        assert data[i.scan_offset + o + n] == 0xFF and data[i.scan_offset + o + n + 1] == nxt
    assert sum(n for _, n, _ in i.segments.tolist()) + 2 * (len(i.segments) - 1) == len(scan)
    q = Image.open(io.BytesIO(data)).quantization
    assert np.array_equal(i.qt[0][jpeg._ZIGZAG], np.asarray(q[0])) or np.array_equal(i.qt[0], np.asarray(q[0]))


def test_parse_jpeg_declines():
    img = photo_like(32, 48, 2)
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", progressive=True)
    assert jpeg.parse_jpeg(buf.getvalue()) is None
    buf = io.BytesIO()
    Image.fromarray(img).convert("CMYK").save(buf, "JPEG")
    assert jpeg.parse_jpeg(buf.getvalue()) is None
    # PIL's writer takes subsampling 4:4:4, 4:2:2 and 4:2:0 only ("4:4:0" is refused), so the 4:4:0 file is a substitute: a
    # 4:4:4 file that PIL wrote with the luma sampling byte of its SOF0 set to 1 x 2 by hand
    base = pil_jpeg(img, "4:4:4", 80)
    k = base.index(b"\xff\xc0")
    assert base[k + 11] == 0x11
    v2 = base[:k + 11] + b"\x12" + base[k + 12:]                              # luma 1 x 2: the 4:4:0 layout
    assert jpeg.parse_jpeg(v2) is None
    for junk in (b"", b"\xff\xd8", b"\xff\xd8\xff", b"not a jpeg at all", base[:k + 6], base[:100], bytes(500)):
        assert jpeg.parse_jpeg(junk) is None
    with pytest.raises(jpegdec_np.JpegError):
        jpegdec_np.decode(buf.getvalue())


def test_damaged_streams_are_reported():
    """Truncated and byte-flipped streams: the restatement raises JpegError or decodes (a flip may leave a valid stream); it
    never indexes out of range, and parse_jpeg never raises."""
    data = pil_jpeg(photo_like(48, 64, 3), "4:2:0", 90)
    info = jpeg.parse_jpeg(data)
    for cut in (info.scan_offset + 1, info.scan_offset + info.scan_length // 2, len(data) - 3):
        with pytest.raises(jpegdec_np.JpegError):
            jpegdec_np.decode(data[:cut])
    r = np.random.default_rng(4)
    errors = 0
    for _ in range(40):
        b = bytearray(data)
        for p in r.integers(2, len(b), 3):
            b[p] ^= 1 << int(r.integers(0, 8))
        try:
            if jpeg.parse_jpeg(bytes(b)) is not None:
                jpegdec_np.decode(bytes(b))
        except jpegdec_np.JpegError:
            errors += 1
    assert errors > 0
    for cut in range(0, info.scan_offset + 2, 7):
        jpeg.parse_jpeg(data[:cut])


def _frames(n, H=24, W=40):
    return [pil_jpeg(photo_like(H, W, seed=s), "4:2:0", 80) for s in range(n)]


def test_mjpeg_reader_reads_the_writer(tmp_path):
    frames = _frames(5) + [jpeg_np.encode(jpeg_np.fixture("noise", 24, 40), 90)]     # odd and even lengths
    p = tmp_path / "a.avi"
    with jpeg.MjpegWriter(str(p), 40, 24, fps=24) as w:
        for f in frames:
            w.add(f)
    with jpeg.MjpegReader(str(p)) as r:
        assert (len(r), r.width, r.height, r.fps) == (6, 40, 24, 24.0)
        assert list(r) == frames and r[3] == frames[3] and r[-1] == frames[-1]
        with pytest.raises(IndexError):
            r[6]
    raw = p.read_bytes()
    k = raw.index(b"idx1")
    noidx = bytearray(raw[:k])
    noidx[4:8] = struct.pack("<I", len(noidx) - 8)
    (tmp_path / "b.avi").write_bytes(bytes(noidx))
    with jpeg.MjpegReader(str(tmp_path / "b.avi")) as r:
        assert list(r) == frames
    with jpeg.MjpegWriter(str(tmp_path / "c.avi"), 40, 24, fps=29.97) as w:
        w.add(frames[0])
    assert abs(jpeg.MjpegReader(str(tmp_path / "c.avi")).fps - 29.97) < 1e-9


def test_mjpeg_reader_frames_without_dht(tmp_path):
    """A hand-built file (mjpg handler in lower case, db chunks, no index) whose frames carry no DHT: they decode with Annex K."""
    frames = [strip_dht(f) for f in _frames(3)]
    assert all(b"\xff\xc4" not in f[:f.index(b"\xff\xda")] for f in frames)
    movi = b"movi" + b"".join(b"00db" + struct.pack("<I", len(f)) + f + b"\0" * (len(f) & 1) for f in frames)
    avih = struct.pack("<14I", 40000, 0, 0, 0, 3, 0, 1, 0, 40, 24, 0, 0, 0, 0)
    strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"mjpg", 0, 0, 0, 0, 1, 25, 0, 3, 0, 0, 0, 0, 0, 40, 24)
    strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh
    hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
    body = b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl + b"LIST" + struct.pack("<I", len(movi)) + movi
    (tmp_path / "h.avi").write_bytes(b"RIFF" + struct.pack("<I", len(body)) + body)
    with jpeg.MjpegReader(str(tmp_path / "h.avi")) as r:
        assert len(r) == 3 and r.fps == 25.0 and list(r) == frames
        for f in r:
            assert np.array_equal(jpegdec_np.decode(f), pil_pixels(f))


def test_mjpeg_reader_refusals(tmp_path):
    p = tmp_path / "a.avi"
    with jpeg.MjpegWriter(str(p), 40, 24) as w:
        w.add(_frames(1)[0])
    raw = p.read_bytes()
    k = raw.index(b"vidsMJPG")
    (tmp_path / "x.avi").write_bytes(raw[:k + 4] + b"H264" + raw[k + 8:])
    with pytest.raises(ValueError, match="not MJPG.*Motion-JPEG AVI.*folder"):
        jpeg.MjpegReader(str(tmp_path / "x.avi"))
    (tmp_path / "y.mp4").write_bytes(b"\0\0\0\x18ftypmp42" + bytes(64))
    with pytest.raises(ValueError, match="only Motion-JPEG AVI is read.*folder"):
        jpeg.MjpegReader(str(tmp_path / "y.mp4"))
    k = raw.index(b"LIST", 12)
    odml = b"LIST" + struct.pack("<I", 4) + b"odml"
    (tmp_path / "z.avi").write_bytes(raw[:12] + odml + raw[12:])
    with pytest.raises(ValueError, match="OpenDML"):
        jpeg.MjpegReader(str(tmp_path / "z.avi"))


def test_mjpeg_reader_short_header_chunks(tmp_path):
    """A damaged avih or strh chunk is a ValueError like every other refusal, so demo.py ends with its message."""
    import struct

    import demo

    def chunk(cid, body):
        return cid + struct.pack("<I", len(body)) + body + bytes(len(body) & 1)

    def riff(hdrl):
        body = b"AVI " + chunk(b"LIST", b"hdrl" + hdrl) + chunk(b"LIST", b"movi")
        return b"RIFF" + struct.pack("<I", len(body)) + body
    files = {"avih": riff(chunk(b"avih", bytes(8))),
             "strh": riff(chunk(b"avih", bytes(56)) + chunk(b"LIST", b"strl" + chunk(b"strh", b"vidsMJPG" + bytes(4))))}
    for name, data in files.items():
        path = tmp_path / (name + ".avi")
        path.write_bytes(data)
        with pytest.raises(ValueError, match=f"damaged: its {name} chunk"):
            jpeg.MjpegReader(str(path))
        with pytest.raises(SystemExit, match="--vid_file: MjpegReader.*damaged"):
            demo.main(demo.parse_args(["--cfg", "c.yaml", "--ckpt", "x.pt", "--mode", "video", "--vid_file", str(path)]))


def test_decoder_argument_errors_without_gpu():
    from poco_amd._lib import PocoHipError, lib
    for a in ((None, 0, 16), (None, 16, 16385), (None, 16, 16, 0), (None, 16, 16, 4097), (None, 16, 16, 1, (1 << 30) + 1)):
        with pytest.raises(PocoHipError, match="max_"):
            jpeg.JpegDecoder(*a)
    L = lib()
    assert hasattr(L, "poco_jpeg_decode") and hasattr(L, "poco_jpeg_decoder_destroy")
    L.poco_jpeg_decoder_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    assert L.poco_jpeg_decoder_create(0, 16, 1, 1024, C.byref(h)) == 1 and not h.value
    assert L.poco_jpeg_decoder_create(16, 16, 0, 1024, C.byref(h)) == 1 and not h.value
    assert L.poco_jpeg_decoder_create(16, 16, 1, 0, C.byref(h)) == 1 and not h.value
    assert L.poco_jpeg_decoder_create(16, 16, 1, 1024, None) == 1
    assert L.poco_last_error().startswith(b"poco_jpeg_decoder_create")
    L.poco_jpeg_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    assert L.poco_jpeg_decode(None, None, 1, None, None) == 1
    assert C.sizeof(jpeg._CImage) == 1352


def test_demo_flags():
    import demo
    base = ["--cfg", "c.yaml", "--ckpt", "x.pt"]
    assert demo.parse_args(base).decode == "host"
    assert demo.parse_args(base + ["--decode", "gpu"]).decode == "gpu"
    with pytest.raises(SystemExit):
        demo.parse_args(base + ["--decode", "fast"])
