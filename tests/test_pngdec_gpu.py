"""GPU: the PNG decoder (csrc/png_dec.hip) against PIL and its numpy restatement (tests/pngdec_np.py, pinned on zlib and PIL in
tests/test_pngdec_cpu.py) BYTE for byte: the fixture set image by image and in one mixed call, guard bands, reuse, the encoder's
round trip, damaged streams and argument errors."""
import ctypes as C

import numpy as np
import pytest
import torch

from poco_amd import png
from poco_amd._lib import lib
from tests import pngdec_np
from tests.test_jpeg_cpu import photo_like
from tests.test_pngdec_cpu import damaged_set, fixture_set, pil_rgb, restated

pytestmark = pytest.mark.gpu

POISON = 0xA5
MAX_H, MAX_W = 260, 700


@pytest.fixture(scope="module")
def dec(cuda):
    return png.PngDecoder(cuda, MAX_H, MAX_W, max_batch=len(fixture_set()), max_bytes=4 << 20)


def _diff(got: torch.Tensor, ref: np.ndarray):
    g = got.cpu().numpy()
    if g.shape != ref.shape:
        return (g.shape, ref.shape)
    d = np.argwhere(g != ref)
    return None if d.size == 0 else (len(d), d[:4].tolist(), g[tuple(d[0])], ref[tuple(d[0])])


def _poisoned(cuda, shapes, guard, shift=0):
    sizes = [int(np.prod(s)) for s in shapes]
    buf = torch.full((sum(sizes) + guard * (len(shapes) + 1) + 8,), POISON, dtype=torch.uint8, device=cuda)
    outs, pos, spans = [], guard + shift, []
    for s, n in zip(shapes, sizes):
        outs.append(buf[pos:pos + n].view(s))
        spans.append((pos, pos + n))
        pos += n + guard
    return buf, outs, spans


def _outside_intact(buf, spans):
    host = buf.cpu().numpy()
    mask = np.ones(host.size, bool)
    for lo, hi in spans:
        mask[lo:hi] = False
    return host, bool((host[mask] == POISON).all())


def test_every_stream_alone(dec):
    for name, data in fixture_set().items():
        (out,), st = dec.decode([data], return_status=True)
        assert st == [0], name
        assert _diff(out, pil_rgb(data)) is None, (name, _diff(out, pil_rgb(data)))
        assert np.array_equal(restated(name)[0], pil_rgb(data)), name


def test_one_call_mixes_everything(dec):
    names = list(fixture_set())
    infos = [png.parse_png(fixture_set()[n]) for n in names]
    assert {i.colour_type for i in infos} == {0, 2, 3, 4, 6} and len({(i.height, i.width) for i in infos}) >= 8
    outs, st = dec.decode(infos, return_status=True)
    assert st == [0] * len(names)
    for n, o in zip(names, outs):
        assert _diff(o, restated(n)[0]) is None, (n, _diff(o, restated(n)[0]))


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_guard_bands(dec, cuda, shift):
    """Outputs inside a poisoned buffer at every byte alignment: nothing outside the pictures changes."""
    names = ["17x33_filters_from3", "1x1_rgb", "40x50_palette_trns", "120x168_pil_default"]
    refs = [restated(n)[0] for n in names]
    buf, outs, spans = _poisoned(cuda, [r.shape for r in refs], 64, shift)
    st = dec.decode_into([fixture_set()[n] for n in names], outs)
    assert st.cpu().tolist() == [0] * len(names)
    host, intact = _outside_intact(buf, spans)
    for (lo, hi), r, n in zip(spans, refs, names):
        assert np.array_equal(host[lo:hi].reshape(r.shape), r), n
    assert intact


def test_decoder_reuse_on_smaller_batches(dec):
    """Large batch, then smaller pictures and batches on the same scratch: nothing stale may leak."""
    fs = fixture_set()
    big = [n for n in fs if n.startswith(("120x168", "96x700", "240x320"))]
    small = [n for n in fs if n.startswith(("1x", "7x1", "17x33", "33x20"))]
    for names in (big, small, small[:3], big[:1], small[-1:]):
        outs, st = dec.decode([fs[n] for n in names], return_status=True)
        assert st == [0] * len(names)
        for n, o in zip(names, outs):
            assert _diff(o, restated(n)[0]) is None, n


def test_round_trip_of_the_encoder(cuda):
    H, W = 90, 150
    frame = torch.from_numpy(photo_like(H, W, 21)).to(cuda)
    data = png.PngEncoder(cuda, H, W).encode(frame)
    (out,), st = png.PngDecoder(cuda, H, W).decode([data], return_status=True)
    assert st == [0] and torch.equal(out, frame)


def test_damaged_streams_in_a_batch(dec, cuda):
    """The damaged set mixed with good streams: a non-zero status for exactly the damaged ones (the restatement's verdict), the good
    ones decoded, guard bands intact, and a clean decode afterwards.  Ordinary inputs the kernel must survive."""
    fs, ds = fixture_set(), damaged_set()
    good = ["120x168_pil_default", "17x33_filters_from1", "40x50_palette_trns", "33x20_grey_alpha"]
    batch = []
    for k, (name, (data, _)) in enumerate(ds.items()):
        batch.append((name, data, True))
        if k % 3 == 0:
            batch.append((good[(k // 3) % len(good)], fs[good[(k // 3) % len(good)]], False))
    infos = [png.parse_png(d) for _, d, _ in batch]
    assert all(i is not None for i in infos)
    verdict = [pngdec_np.decode(i)[1] != 0 for i in infos]
    assert verdict == [bad for _, _, bad in batch]
    buf, outs, spans = _poisoned(cuda, [(i.height, i.width, 3) for i in infos], 256)
    st = dec.decode_into(infos, outs).cpu().tolist()
    assert [s != 0 for s in st] == verdict, st
    host, intact = _outside_intact(buf, spans)
    assert intact
    for (name, _, bad), (lo, hi) in zip(batch, spans):
        if not bad:
            assert np.array_equal(host[lo:hi].reshape(restated(name)[0].shape), restated(name)[0]), name
    outs, st = dec.decode([fs[n] for n in good], return_status=True)
    assert st == [0] * len(good) and all(_diff(o, restated(n)[0]) is None for n, o in zip(good, outs))


def test_argument_errors_leave_the_decoder_usable(cuda):
    fs = fixture_set()
    name = "17x33_filters_from0"
    small = png.PngDecoder(cuda, 40, 40, max_batch=2, max_bytes=4096)
    PE = png.PocoHipError
    with pytest.raises(PE, match="created for"):
        small.decode([fs[name]] * 3)
    with pytest.raises(PE, match="created for"):
        small.decode([])
    with pytest.raises(PE, match="size the decoder was created for"):
        small.decode([fs["120x168_pil_default"]])
    noise = np.random.default_rng(0).integers(0, 256, (40, 40, 3), dtype=np.uint8)
    from tests.test_pngdec_cpu import make_png
    with pytest.raises(PE, match="exceed"):
        small.decode([make_png(noise, 2)] * 2)                                     # 2 x 4.8 KB
    with pytest.raises(PE, match="parse_png"):
        small.decode([b"\x89PNG\r\n\x1a\n nothing"])
    info = png.parse_png(fs[name])
    ok = torch.empty(17, 33, 3, dtype=torch.uint8, device=cuda)
    for out in (torch.empty(17, 33, 3, dtype=torch.uint8), ok.float(), torch.empty(33, 17, 3, dtype=torch.uint8, device=cuda), ok[:, ::2]):
        with pytest.raises(PE, match="output"):
            small.decode_into([info], [out])
    with pytest.raises(PE, match="status"):
        small.decode_into([info], [ok], status=torch.zeros(1, device=cuda))
    # the C entry refuses what the wrapper cannot express, before any GPU work
    L = lib()
    st = torch.full((2,), -7, dtype=torch.int32, device=cuda)
    ok.fill_(POISON)
    arr = (png._CPngImage * 1)()
    assert L.poco_png_decode(small._h, C.cast(arr, C.c_void_p), 1, st.data_ptr(), None) == 1            # null pointers
    assert L.poco_png_decode(small._h, None, 1, st.data_ptr(), None) == 1
    assert L.poco_png_decode(small._h, C.cast(arr, C.c_void_p), 1, None, None) == 1
    assert L.poco_last_error().startswith(b"poco_png_decode")
    for field, value in (("colour_type", 5), ("colour_type", 1), ("idat", [(len(fs[name]) - 4, 64)]), ("idat", [(40, 3)])):
        bad = png.PngInfo(**{**info.__dict__})
        setattr(bad, field, value)
        with pytest.raises(PE, match="poco_png_decode"):
            small.decode_into([bad], [ok])
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [-7, -7] and bool((ok == POISON).all())
    (out,), s = small.decode([fs[name]], return_status=True)
    assert s == [0] and _diff(out, restated(name)[0]) is None
