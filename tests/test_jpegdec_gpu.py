"""GPU: the JPEG decoder (csrc/jpeg_dec.hip) against its numpy restatement (tests/jpegdec_np.py, pinned on PIL in
tests/test_jpegdec_cpu.py) BYTE for byte: the fixture set image by image and in one mixed call, a restart interval longer than one
workgroup's lanes, guard bands, reuse, the encoder's round trip, damaged streams and argument errors - and the streams libjpeg's
writer never makes (tests/jpegdec_cases.py): alone, batched with the fixture set, around the slowest synchronisation, damaged."""
import ctypes as C

import numpy as np
import pytest
import torch

from poco_amd import jpeg
from poco_amd._lib import lib
from tests import jpeg_np, jpegdec_np
from tests.jpegdec_cases import BOUNDARY, hand_cases, unowned_code
from tests.test_jpegdec_cpu import fixture_set, hand_restated, pil_jpeg, restated
from tests.test_jpeg_cpu import photo_like

pytestmark = pytest.mark.gpu

POISON = 0xA5
MAX_H, MAX_W = 120, 2048


@pytest.fixture(scope="module")
def dec(cuda):
    return jpeg.JpegDecoder(cuda, MAX_H, MAX_W, max_batch=len(fixture_set()) + len(hand_cases()), max_bytes=4 << 20)


def _diff(got: torch.Tensor, ref: np.ndarray):
    g = got.cpu().numpy()
    if g.shape != ref.shape:
        return (g.shape, ref.shape)
    d = np.argwhere(g != ref)
    return None if d.size == 0 else (len(d), d[:4].tolist(), g[tuple(d[0])], ref[tuple(d[0])])


def test_every_stream_alone(dec):
    for name, data in fixture_set().items():
        (out,), st = dec.decode([data], return_status=True)
        assert st == [0], name
        assert _diff(out, restated(name)[0]) is None, (name, _diff(out, restated(name)[0]))


def test_one_call_mixes_everything(dec):
    """All streams in one call: four samplings, every size, restart intervals of every kind, frames without DHT."""
    names = list(fixture_set())
    infos = [jpeg.parse_jpeg(fixture_set()[n]) for n in names]
    assert {(i.ncomp, i.hsamp, i.vsamp) for i in infos} == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    assert len({(i.height, i.width) for i in infos}) >= 6
    outs, st = dec.decode(infos, return_status=True)
    assert st == [0] * len(names)
    for n, o in zip(names, outs):
        assert _diff(o, restated(n)[0]) is None, (n, _diff(o, restated(n)[0]))


def test_interval_longer_than_a_workgroup(dec):
    """64 x 2048 noise without restart markers: one interval of more than 256 subsequences, so states cross workgroups."""
    name = "64x2048_noise_q95"
    info = jpeg.parse_jpeg(fixture_set()[name])
    assert len(info.segments) == 1 and info.segments[0, 1] > 4 * 256 * jpeg.SUBSEQ_BYTES
    (out,), st = dec.decode([info], return_status=True)
    assert st == [0] and _diff(out, restated(name)[0]) is None, _diff(out, restated(name)[0])


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
def test_guard_bands(dec, cuda, shift):
    """Outputs inside a poisoned buffer at every byte alignment: nothing outside the pictures changes."""
    names = ["17x33_4:2:0", "1x1_4:2:2", "24x700_gray", "120x168_4:4:4"]
    names = [next(n for n in fixture_set() if n.startswith(p)) for p in names]
    guard = 64
    refs = [restated(n)[0] for n in names]
    sizes = [r.size for r in refs]
    buf = torch.full((sum(sizes) + guard * (len(names) + 1) + 8,), POISON, dtype=torch.uint8, device=cuda)
    outs, pos, spans = [], guard + shift, []
    for r in refs:
        outs.append(buf[pos:pos + r.size].view(r.shape))
        spans.append((pos, pos + r.size))
        pos += r.size + guard
    st = dec.decode_into([fixture_set()[n] for n in names], outs)
    assert st.cpu().tolist() == [0] * len(names)
    host = buf.cpu().numpy()
    mask = np.ones(host.size, bool)
    for (lo, hi), r, n in zip(spans, refs, names):
        assert np.array_equal(host[lo:hi].reshape(r.shape), r), n
        mask[lo:hi] = False
    assert (host[mask] == POISON).all()


def test_decoder_reuse_on_smaller_batches(dec):
    """Large batch, then smaller pictures and batches on the same scratch: no stale state, coefficient or plane may leak."""
    fs = fixture_set()
    big = [n for n in fs if n.startswith(("120x168", "24x700", "96x128"))]
    small = [n for n in fs if n.startswith(("8x8", "17x33", "1x1"))]
    for names in (big, small, small[:3], big[:1], small[-1:]):
        outs, st = dec.decode([fs[n] for n in names], return_status=True)
        assert st == [0] * len(names)
        for n, o in zip(names, outs):
            assert _diff(o, restated(n)[0]) is None, n


def test_round_trip_of_the_encoder(cuda):
    H, W = 90, 150
    frame = torch.from_numpy(photo_like(H, W, 21)).to(cuda)
    data = jpeg.JpegEncoder(cuda, H, W).encode(frame, 85)
    (out,) = jpeg.JpegDecoder(cuda, H, W).decode([data])
    assert _diff(out, jpegdec_np.decode(data)) is None


def test_damaged_streams_in_a_batch(dec, cuda):
    """A stream cut at half and one with a code that is in no table: non-zero status for exactly those, the others decoded,
    guard bands intact, and a clean decode afterwards."""
    fs = fixture_set()
    good = [n for n in fs if n.startswith(("96x128_4:2:0", "17x33_4:4:4"))][:3]
    cut_src = fs[next(n for n in fs if n.startswith("120x168_4:2:2"))]
    cut = cut_src[:len(cut_src) // 2]
    assert jpeg.parse_jpeg(cut) is not None
    # an optimised table leaves code space unused: fill the scan's first bytes with 1-bits - the all-ones word is never a code
    src = pil_jpeg(photo_like(40, 64, 9), "4:2:0", 75, optimize=True)
    info = jpeg.parse_jpeg(src)
    bad = src[:info.scan_offset + 8] + b"\xff\x00" * 4 + src[info.scan_offset + 16:]
    assert jpeg.parse_jpeg(bad) is not None
    with pytest.raises(jpegdec_np.JpegError):
        jpegdec_np.decode(bad)
    batch = [fs[good[0]], cut, fs[good[1]], bad, fs[good[2]]]
    infos = [jpeg.parse_jpeg(b) for b in batch]
    guard = 256
    total = sum(i.height * i.width * 3 + guard for i in infos) + guard
    buf = torch.full((total,), POISON, dtype=torch.uint8, device=cuda)
    outs, pos, spans = [], guard, []
    for i in infos:
        n = i.height * i.width * 3
        outs.append(buf[pos:pos + n].view(i.height, i.width, 3))
        spans.append((pos, pos + n))
        pos += n + guard
    st = dec.decode_into(infos, outs).cpu().tolist()
    assert [s != 0 for s in st] == [False, True, False, True, False], st
    host = buf.cpu().numpy()
    mask = np.ones(host.size, bool)
    for lo, hi in spans:
        mask[lo:hi] = False
    assert (host[mask] == POISON).all()
    for k, n in ((0, good[0]), (2, good[1]), (4, good[2])):
        assert np.array_equal(host[spans[k][0]:spans[k][1]].reshape(restated(n)[0].shape), restated(n)[0]), n
    outs, st = dec.decode([fs[n] for n in good], return_status=True)
    assert st == [0, 0, 0] and all(_diff(o, restated(n)[0]) is None for n, o in zip(good, outs))


def test_every_hand_case_alone(dec):
    for name, data in hand_cases().items():
        (out,), st = dec.decode([data], return_status=True)
        assert st == [0], name
        assert _diff(out, hand_restated(name)[0]) is None, (name, _diff(out, hand_restated(name)[0]))


def test_one_call_mixes_hand_cases_and_fixtures(dec):
    """Optimal, flat and deep tables under every id layout, restart intervals of one MCU and none, next to what PIL writes."""
    refs = [(n, hand_restated(n)[0], d) for n, d in hand_cases().items()] + [(n, restated(n)[0], d) for n, d in fixture_set().items()]
    refs = refs[0::2] + refs[1::2]                                         # neighbours in the batch are of different kinds
    outs, st = dec.decode([d for _, _, d in refs], return_status=True)
    assert st == [0] * len(refs)
    for (n, ref, _), o in zip(refs, outs):
        assert _diff(o, ref) is None, (n, _diff(o, ref))


def test_boundary_cases_around_the_slowest_synchronisation(dec):
    """The boundary cases first and last in the batch, the stream whose every lane waits for its predecessor between them;
    then smaller batches on the same scratch: no entry or exit state of the many-round image may leak into the next call."""
    hc = hand_cases()
    b = list(BOUNDARY.values())
    small = [n for n in hc if n.endswith("17x13")]
    assert len(b) == 4 and len(small) >= 6
    for names in (b[:2] + ["slow-sync"] + b[2:], small, ["slow-sync"], small[:3], b[2:3], ["slow-sync", b[0]], small[-1:]):
        outs, st = dec.decode([hc[n] for n in names], return_status=True)
        assert st == [0] * len(names), names
        for n, o in zip(names, outs):
            assert _diff(o, hand_restated(n)[0]) is None, (n, _diff(o, hand_restated(n)[0]))


def test_code_that_no_table_owns(dec):
    """A deep-table stream with sixteen 1-bits where a symbol starts, two subsequences into the scan: the window holds no code.
    Non-zero status for that image, as the restatement reports it; its neighbours are what they are alone."""
    hc = hand_cases()
    good = ["tables-deep-shared-420-33x47", "tables-deep-per_component-444-33x47", "tables-flat-swapped-444-17x13"]
    bad, bp = unowned_code(hc[good[1]])
    with pytest.raises(jpegdec_np.JpegError, match=f"no Huffman code at byte {bp}$"):
        jpegdec_np.decode(bad)
    solo = [dec.decode([hc[n]])[0] for n in good]
    outs, st = dec.decode([hc[good[0]], bad, hc[good[1]], hc[good[2]]], return_status=True)
    assert [s != 0 for s in st] == [False, True, False, False], st
    for n, o, alone in zip(good, [outs[0], outs[2], outs[3]], solo):
        assert torch.equal(o, alone) and _diff(o, hand_restated(n)[0]) is None, n
    outs, st = dec.decode([hc[good[1]]], return_status=True)               # and a clean decode afterwards
    assert st == [0] and _diff(outs[0], hand_restated(good[1])[0]) is None


def test_argument_errors_leave_the_decoder_usable(cuda):
    fs = fixture_set()
    name = next(n for n in fs if n.startswith("17x33_4:2:0"))
    small = jpeg.JpegDecoder(cuda, 40, 40, max_batch=2, max_bytes=4096)
    PE = jpeg.PocoHipError
    with pytest.raises(PE, match="created for"):
        small.decode([fs[name]] * 3)
    with pytest.raises(PE, match="created for"):
        small.decode([])
    with pytest.raises(PE, match="size the decoder was created for"):
        small.decode([fs[next(n for n in fs if n.startswith("96x128"))]])
    with pytest.raises(PE, match="exceed"):
        small.decode([pil_jpeg(np.random.default_rng(0).integers(0, 256, (40, 40, 3), dtype=np.uint8), "4:4:4", 100)] * 2)   # 2 x 7 KB
    with pytest.raises(PE, match="parse_jpeg"):
        small.decode([b"\xff\xd8 nothing"])
    info = jpeg.parse_jpeg(fs[name])
    ok = torch.empty(17, 33, 3, dtype=torch.uint8, device=cuda)
    for out in (torch.empty(17, 33, 3, dtype=torch.uint8), ok.float(), torch.empty(33, 17, 3, dtype=torch.uint8, device=cuda), ok[:, ::2]):
        with pytest.raises(PE, match="output"):
            small.decode_into([info], [out])
    with pytest.raises(PE, match="status"):
        small.decode_into([info], [ok], status=torch.zeros(1, device=cuda))
    # the C entry refuses what the wrapper cannot express, before any GPU work
    L = lib()
    st = torch.full((2,), -7, dtype=torch.int32, device=cuda)
    arr = (jpeg._CImage * 1)()
    assert L.poco_jpeg_decode(small._h, C.cast(arr, C.c_void_p), 1, st.data_ptr(), None) == 1          # null pointers
    assert L.poco_jpeg_decode(small._h, None, 1, st.data_ptr(), None) == 1
    assert L.poco_jpeg_decode(small._h, C.cast(arr, C.c_void_p), 1, None, None) == 1
    assert L.poco_last_error().startswith(b"poco_jpeg_decode")
    # dc_bits: a prefix code of 18 symbols, more than the 16 a DC table holds
    for field, value in (("segs", [[0, 1 << 20, 0]]), ("segs", [[0, 4, 1]]), ("hsamp", 3), ("ac_bits", bytes([255] * 16)),
                         ("dc_bits", bytes([0] + [2] * 9 + [0] * 6))):
        bad = jpeg.JpegInfo(**{**info.__dict__})
        if field == "segs":
            bad.segments = np.array(value, np.uint32)
        elif field == "hsamp":
            bad.hsamp = 3
        elif field == "dc_bits":
            bad.dc = [(value, info.dc[0][1])] * 3
        else:
            bad.ac = [(value, info.ac[0][1])] * 3
        with pytest.raises(PE, match="poco_jpeg_decode"):
            small.decode_into([bad], [ok])
    torch.cuda.synchronize()
    assert st.cpu().tolist() == [-7, -7]
    (out,), s = small.decode([fs[name]], return_status=True)
    assert s == [0] and _diff(out, restated(name)[0]) is None
