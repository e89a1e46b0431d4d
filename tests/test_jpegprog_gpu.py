"""GPU: the progressive JPEG decoder (poco_amd.jpeg.ProgressiveJpegDecoder over poco_jpeg_prog_decode, csrc/jpeg_prog.hip) gives
PIL's pixels byte for byte over the matrix of tests/jpegprog_cases.py - alone, in one mixed batch and call after call - and
reports a file cut short in its fifth scan in that image's status word only.  The scan scripts, table shapes and table id layouts
PIL never writes (K.script_cases(), held to libjpeg and to the restatement in tests/test_jpegprog_cpu.py) are decoded alone and in
one call with the matrix; files with more tables than a decoder plans and scripts that end above Al = 0 are refused before any
GPU work."""
import numpy as np
import pytest
import torch

from poco_amd import jpeg
from tests import jpegprog_cases as K
from tests import jpegprog_np as P

pytestmark = pytest.mark.gpu

CASES = K.cases()
SCRIPTS = K.script_cases()
DECODABLE = sorted(n for n, c in SCRIPTS.items() if c.decodable)
SMALL = [n for n in DECODABLE if not SCRIPTS[n].big]


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


# ---- scan scripts PIL never writes ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def sdec(cuda):
    return jpeg.ProgressiveJpegDecoder(cuda, 256, 256, max_batch=len(CASES) + len(SMALL), max_bytes=4 << 20)


@pytest.fixture(scope="module")
def srefs():
    return {n: K.reference(SCRIPTS[n].data) for n in SMALL}


@pytest.mark.parametrize("name", DECODABLE)
def test_every_script_case_alone(sdec, cuda, name):
    c = SCRIPTS[name]
    info = jpeg.parse_progressive_jpeg(c.data)
    d = jpeg.ProgressiveJpegDecoder(cuda, K.EOB_CAP_SIDE, K.EOB_CAP_SIDE, max_bytes=1 << 16) if c.big else sdec
    assert d.fits(info)
    (out,), st = d.decode([info], return_status=True)
    assert st == [0]
    ref = K.reference(c.data)
    assert _diff(out, ref) is None, _diff(out, ref)


def test_one_call_mixes_script_cases_with_the_matrix(sdec, refs, srefs):
    """Scripts of one to five levels, 64-scan files and libjpeg's own script share the level launches of one call: forward and
    reverse order, twice each."""
    files = [(n, CASES[n], refs[n]) for n in sorted(CASES)] + [(n, SCRIPTS[n].data, srefs[n]) for n in SMALL]
    infos = [jpeg.parse_progressive_jpeg(d) for _, d, _ in files]
    assert {len(i.scans) for i in infos} >= {2, 4, 6, 10, 12, 15, 16, 19, 64}
    runs = []
    for order in (infos, infos[::-1], infos, infos[::-1]):
        outs, st = sdec.decode(order, return_status=True)
        assert st == [0] * len(files)
        runs.append(outs if order is infos else outs[::-1])
    for k, (n, _, ref) in enumerate(files):
        assert _diff(runs[0][k], ref) is None, (n, _diff(runs[0][k], ref))
        assert all(torch.equal(runs[0][k], r[k]) for r in runs[1:]), n


def test_more_tables_than_planned_are_refused_before_gpu_work(sdec, srefs):
    from poco_amd._lib import PocoHipError
    (many,) = [n for n, c in SCRIPTS.items() if c.kind == "tables-many"]
    info = jpeg.parse_progressive_jpeg(SCRIPTS[many].data)
    assert info is not None and not sdec.fits(info)
    names = ["dc-split-420-q95-33x47", "deep-444-q95-17x13"]
    with pytest.raises(PocoHipError, match="more than 16 Huffman tables"):
        sdec.decode([SCRIPTS[names[0]].data, info, SCRIPTS[names[1]].data])
    outs, st = sdec.decode([SCRIPTS[n].data for n in names], return_status=True)
    assert st == [0, 0]
    for n, o in zip(names, outs):
        assert _diff(o, srefs[n]) is None, n


@pytest.mark.parametrize("name", sorted(n for n, c in SCRIPTS.items() if c.kind == "ends-above-zero"))
def test_script_that_ends_above_zero_is_refused(sdec, srefs, name):
    """By the parser, and by poco_jpeg_prog_decode itself for a caller that brings its own scan table; the same bytes without
    EOI are a file cut short: taken, and reported in its status word only."""
    import dataclasses
    from poco_amd._lib import PocoHipError
    data = SCRIPTS[name].data
    d = sdec
    with pytest.raises(PocoHipError, match="parse_progressive_jpeg"):
        d.decode([data])
    cut = jpeg.parse_progressive_jpeg(data[:-2])
    assert cut is not None and cut.cut
    with pytest.raises(PocoHipError, match="above Al = 0"):
        d.decode([dataclasses.replace(cut, cut=False)])
    assert P.decode_status(data[:-2])[1] == P.ERR_SHORT
    good = "dc-split-422-q95-17x13"
    outs, st = d.decode([SCRIPTS[good].data, cut, SCRIPTS[good].data], return_status=True)
    assert st == [0, P.ERR_SHORT, 0]
    assert _diff(outs[0], srefs[good]) is None and _diff(outs[2], srefs[good]) is None
