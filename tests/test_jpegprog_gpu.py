"""GPU: the progressive JPEG decoder (poco_amd.jpeg.ProgressiveJpegDecoder over poco_jpeg_prog_decode, csrc/jpeg_prog.hip) gives
PIL's pixels byte for byte over the matrix of tests/jpegprog_cases.py - alone, in one mixed batch and call after call - and
reports a file cut short in its fifth scan in that image's status word only."""
import numpy as np
import pytest
import torch

from poco_amd import jpeg
from tests import jpegprog_cases as K
from tests import jpegprog_np as P

pytestmark = pytest.mark.gpu

CASES = K.cases()


@pytest.fixture(scope="module")
def dec(cuda):
    return jpeg.ProgressiveJpegDecoder(cuda, 256, 256, max_batch=len(CASES) + 1, max_bytes=2 << 20)


@pytest.fixture(scope="module")
def refs():
    return {n: K.reference(d) for n, d in CASES.items()}


def _diff(got: torch.Tensor, ref: np.ndarray):
    g = got.cpu().numpy()
    if g.shape != ref.shape:
        return (g.shape, ref.shape)
    d = np.argwhere(g != ref)
    return None if d.size == 0 else (len(d), d[:4].tolist(), g[tuple(d[0])], ref[tuple(d[0])])


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_file_alone(dec, refs, name):
    info = jpeg.parse_progressive_jpeg(CASES[name])
    assert dec.fits(info)
    (out,), st = dec.decode([info], return_status=True)
    assert st == [0]
    assert _diff(out, refs[name]) is None, _diff(out, refs[name])


def test_one_call_mixes_everything_and_a_second_call_repeats_it(dec, refs):
    """All samplings, sizes and qualities in one call; the same call again gives the same bytes (no stale coefficients); then a
    call of the files in reverse order, so that every image lands on another part of the scratch."""
    names = sorted(CASES)
    infos = [jpeg.parse_progressive_jpeg(CASES[n]) for n in names]
    assert {(i.ncomp, i.hsamp, i.vsamp) for i in infos} == {(1, 1, 1), (3, 1, 1), (3, 2, 1), (3, 2, 2)}
    first, st = dec.decode(infos, return_status=True)
    assert st == [0] * len(names)
    second, st = dec.decode(infos, return_status=True)
    assert st == [0] * len(names)
    third, st = dec.decode(infos[::-1], return_status=True)
    assert st == [0] * len(names)
    for n, a, b, c in zip(names, first, second, third[::-1]):
        assert _diff(a, refs[n]) is None, (n, _diff(a, refs[n]))
        assert torch.equal(a, b) and torch.equal(a, c), n


def test_decode_into_writes_only_the_pictures(dec, refs, cuda):
    """Outputs at odd addresses inside a poisoned buffer, a caller-owned status tensor."""
    names = ["420-q75-17x13", "grey-q95-33x47", "422-q30-1x1"]
    sizes = [refs[n].shape for n in names]
    buf = torch.full((sum(h * w * 3 for h, w, _ in sizes) + 64,), 0xA5, dtype=torch.uint8, device=cuda)
    outs, off = [], 1
    for h, w, _ in sizes:
        outs.append(buf[off:off + h * w * 3].view(h, w, 3))
        off += h * w * 3 + 7
    status = torch.full((4,), 99, dtype=torch.int32, device=cuda)
    assert dec.decode_into([CASES[n] for n in names], outs, status) is status
    assert status.cpu().tolist() == [0, 0, 0, 99]
    mask = torch.ones_like(buf, dtype=torch.bool)
    off = 1
    for (h, w, _), n, o in zip(sizes, names, outs):
        assert _diff(o, refs[n]) is None, n
        mask[off:off + h * w * 3] = False
        off += h * w * 3 + 7
    assert bool((buf[mask] == 0xA5).all())


def test_truncated_file_sets_its_status_word_only(dec, refs):
    cut = K.truncated()
    assert P.decode_status(cut)[1] == P.ERR_SHORT                       # known on the CPU first (tests/test_jpegprog_cpu.py)
    names = ["420-q75-200x150", "444-q95-33x47"]
    outs, st = dec.decode([CASES[names[0]], cut, CASES[names[1]]], return_status=True)
    assert st[0] == 0 and st[2] == 0 and st[1] == P.ERR_SHORT
    assert _diff(outs[0], refs[names[0]]) is None and _diff(outs[2], refs[names[1]]) is None


def test_argument_errors(dec, cuda):
    from poco_amd._lib import PocoHipError
    with pytest.raises(PocoHipError, match="parse_progressive_jpeg"):
        dec.decode([K.encode(K.picture(16, 16), "420", progressive=False)])
    small = jpeg.ProgressiveJpegDecoder(cuda, 16, 16)
    with pytest.raises(PocoHipError, match="poco_jpeg_prog_decode"):
        small.decode([CASES["420-q75-33x47"]])
    assert not small.fits(jpeg.parse_progressive_jpeg(CASES["420-q75-33x47"]))
    with pytest.raises(PocoHipError, match="1..1"):
        small.decode([CASES["420-q75-8x8"]] * 2)
