"""CPU: the progressive JPEG parser (poco_amd.jpeg.parse_progressive_jpeg) and the numpy restatement of the progressive coefficient
stage (tests/jpegprog_np.py), which must give PIL's pixels byte for byte - the contract csrc/jpeg_prog.hip is tested against on
the GPU (tests/test_jpegprog_gpu.py).  The scan scripts PIL never writes come from the transcoder tests/jpegprog_enc_np.py, which is
held to libjpeg alone (PIL's pixels of a rescanned file equal PIL's pixels of its source) before the parser and the restatement
are held to its files; what each case is there to reach is asserted on the restatement's counters."""
import functools
import io

import numpy as np
import pytest
from PIL import Image

from tests import jpegprog_cases as K
from tests import jpegprog_np as P
from poco_amd import _lib
from poco_amd.jpeg import MAX_SCANS, TABLES_PER_IMAGE, _scan_tables, parse_jpeg, parse_progressive_jpeg

CASES = K.cases()
SCRIPTS = K.script_cases()


def test_pil_writes_progressive_files_with_all_four_scan_kinds():
    data = CASES["420-q75-200x150"]
    assert data.count(b"\xff\xc2") >= 1 and b"\xff\xc0" not in data[:data.index(b"\xff\xda")]
    info = parse_progressive_jpeg(data)
    assert info is not None and len(info.scans) == 10 and (info.height, info.width, info.ncomp) == (150, 200, 3)
    kinds = {(s.ss == 0, s.ah == 0) for s in info.scans}
    assert kinds == {(True, True), (True, False), (False, True), (False, False)}
    assert info.scans[0].comps == (0, 1, 2) and all(len(s.comps) == 1 for s in info.scans if s.ss)
    assert len(parse_progressive_jpeg(CASES["grey-q75-200x150"]).scans) == 6


@pytest.mark.parametrize("name", sorted(CASES))
def test_parser_accepts_and_baseline_parser_declines(name):
    data = CASES[name]
    info = parse_progressive_jpeg(data)
    assert info is not None and 1 < len(info.scans) <= MAX_SCANS
    assert parse_jpeg(data) is None                                    # --decode gpu keeps sending these through PIL
    ref = K.reference(data)
    assert (info.height, info.width) == ref.shape[:2]
    for s in info.scans:
        assert data[s.offset - 1] != 0xFF and s.offset + s.length <= len(data)
        assert data[s.offset + s.length:s.offset + s.length + 1] == b"\xff"


def test_parser_declines_what_the_decoder_does_not_take():
    rgb = K.picture(33, 47)
    assert parse_progressive_jpeg(K.encode(rgb, "420", progressive=False)) is None                    # baseline: parse_jpeg's
    assert parse_jpeg(K.encode(rgb, "420", progressive=False)) is not None
    data = CASES["420-q75-33x47"]
    sof = data.index(b"\xff\xc2")
    assert parse_progressive_jpeg(data[:sof] + b"\xff\xca" + data[sof + 2:]) is None                  # SOF10: arithmetic coding
    buf = io.BytesIO()
    Image.fromarray(rgb).convert("CMYK").save(buf, "JPEG", progressive=True)
    assert parse_progressive_jpeg(buf.getvalue()) is None                                             # four components
    first = parse_progressive_jpeg(data).scans[0]
    for cut in (2, sof + 5, first.offset - 3):                                                        # a header cut short
        assert parse_progressive_jpeg(data[:cut]) is None
    assert parse_progressive_jpeg(b"") is None and parse_progressive_jpeg(b"\x89PNG\r\n\x1a\n") is None
    # 12 bit, a restart interval, other sampling factors
    assert parse_progressive_jpeg(data[:sof + 4] + b"\x0c" + data[sof + 5:]) is None
    assert parse_progressive_jpeg(data[:sof] + b"\xff\xdd\x00\x04\x00\x08" + data[sof:]) is None
    assert parse_progressive_jpeg(data[:sof + 11] + b"\x41" + data[sof + 12:]) is None


def test_parser_validates_the_scan_script():
    data = CASES["420-q75-33x47"]
    info = parse_progressive_jpeg(data)

    def patched(scan, field, value):                       # the SOS header ends right before the scan's bytes: Ss Se AhAl
        b = bytearray(data)
        b[scan.offset - 3 + field] = value
        return bytes(b)
    ac = next(s for s in info.scans if s.ss)
    assert parse_progressive_jpeg(patched(info.scans[0], 1, 5)) is None            # a DC scan with Se = 5
    assert parse_progressive_jpeg(patched(ac, 0, ac.se + 1)) is None               # Ss > Se
    assert parse_progressive_jpeg(patched(ac, 1, 64)) is None                      # Se > 63
    ref = next(s for s in info.scans if s.ss and s.ah)
    assert parse_progressive_jpeg(patched(ref, 2, ((ref.ah + 1) << 4) | ref.al)) is None      # Ah != Al + 1
    assert parse_progressive_jpeg(patched(ref, 2, ref.al)) is None                 # a second first scan of the band
    # a script that leaves coefficients without any scan: the file cut before its last first scan of a band
    fifth = info.scans[4]
    assert parse_progressive_jpeg(data[:fifth.offset - 14]) is None


def test_truncated_file_is_parsed_and_the_restatement_reports_it():
    cut = K.truncated()
    info = parse_progressive_jpeg(cut)
    assert info is not None and len(info.scans) == 5 and info.cut
    px, status = P.decode_status(cut)
    assert px is None and status == P.ERR_SHORT


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_pil(name):
    data = CASES[name]
    stats = {}
    px, status = P.decode_status(data, stats)
    assert status == 0
    assert np.array_equal(px, K.reference(data))
    if name == "flat-256":
        assert stats["eobrun"] >= 256                      # one run over hundreds of blocks
    if name == "noise-64-q95":
        assert stats["corrections"] > 64 * 64              # correction bits on nearly every coefficient of the luma blocks


def test_matrix_reaches_zero_runs_inside_refinement():
    stats = {}
    P.decode_status(CASES["420-q95-200x150"], stats)
    assert stats["refine_zrl"] > 0 and stats["corrections"] > 0 and stats["eobrun"] > 1


def test_c_abi_entries_are_declared_and_exported():
    syms = _lib.header_symbols()
    L = _lib.lib()
    for s in ("poco_jpeg_prog_decoder_create", "poco_jpeg_prog_decode", "poco_jpeg_prog_decoder_destroy"):
        assert s in syms and hasattr(L, s), s
    assert "#define POCO_ABI_VERSION 4" in _lib.HEADER.read_text()     # additions only


# ---- scan scripts PIL never writes ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _decoded(name):
    """(pixels, status, stats) of the restatement, once per case."""
    stats = {}
    px, status = P.decode_status(SCRIPTS[name].data, stats)
    return px, status, stats


def _names(**want):
    return sorted(n for n, c in SCRIPTS.items() if all(getattr(c, k) == v for k, v in want.items()))


def test_script_cases_hold_every_kind_and_source():
    kinds = {c.kind for c in SCRIPTS.values()}
    assert kinds == {"spectral", "dc-split", "deep", "bands-64", "bands-65", "resplit-join", "resplit-split", "component-major",
                     "eob-cap", "eob-corrections", "tables-flat", "tables-deep", "tables-one-id", "tables-many", "ends-above-zero"}
    for kind in ("spectral", "deep", "resplit-join", "resplit-split", "eob-corrections"):
        assert {n[len(kind) + 1:] for n in _names(kind=kind)} == set(K.SMALL_SOURCES), kind
    assert {n[len("dc-split") + 1:] for n in _names(kind="dc-split")} == {f"{s}-q95-{z}" for s in ("420", "422") for z in ("33x47", "17x13")}
    assert len(_names(kind="ends-above-zero")) == 3 + len(K.SMALL_SOURCES)
    assert [n for n, c in SCRIPTS.items() if c.big] == ["eob-cap"]
    for c in SCRIPTS.values():
        assert c.decodable <= (c.parses and c.complete)


@pytest.mark.parametrize("name", _names(complete=True))
def test_transcoder_keeps_the_pixels_libjpeg_gives(name):
    """The coefficients are the source's, so libjpeg decodes both files to the same picture: the transcoder's self-check, which
    involves no code of this repository's decoder."""
    c = SCRIPTS[name]
    assert np.array_equal(K.reference(c.data), K.reference(c.source))


@pytest.mark.parametrize("name", _names(parses=True))
def test_parser_reads_the_script_back(name):
    c = SCRIPTS[name]
    info = parse_progressive_jpeg(c.data)
    assert info is not None and not info.cut
    assert [(s.comps, s.ss, s.se, s.ah, s.al) for s in info.scans] == [tuple(s) for s in c.script]
    assert parse_jpeg(c.data) is None
    for s in info.scans:
        assert (s.ac is not None) == (s.ss > 0) and all((t is not None) == (s.ss == 0 and s.ah == 0) for t in s.dc)


@pytest.mark.parametrize("name", _names(parses=True))
def test_restatement_equals_pil_on_script_cases(name):
    px, status, _ = _decoded(name)
    assert status == 0
    assert np.array_equal(px, K.reference(SCRIPTS[name].data))


def test_script_cases_reach_what_they_are_there_for():
    """On the restatement's counters alone."""
    for n in _names(kind="spectral"):
        assert _decoded(n)[2]["levels"] == 1 and _decoded(n)[2]["corrections"] == 0
    for n in _names(kind="dc-split"):
        st = _decoded(n)[2]
        info = parse_progressive_jpeg(SCRIPTS[n].data)
        assert -(-info.width // 8) % info.hsamp != 0                    # luma's own raster is narrower than the MCUs'
        assert st["dc_alone"] == 9 and st["dc_refine_ragged_luma"] == 2 and st["levels"] == 3
    for n in _names(kind="deep"):
        st = _decoded(n)[2]
        assert st["levels"] == 5 and st["corrections"] > 0 and st["refine_zrl"] > 0
        assert len(_scan_tables(parse_progressive_jpeg(SCRIPTS[n].data))[0]) <= TABLES_PER_IMAGE
    st = _decoded("eob-cap")[2]
    assert st["eobrun"] == 0x7FFF and st["eobrun_cap"] == 1 and st["refine_eobrun"] == 0x7FFF
    for n in _names(kind="eob-corrections"):
        assert _decoded(n)[2]["eob_corrections"] > 0, n
    for n in _names(kind="tables-deep"):
        st = _decoded(n)[2]
        assert st["symbols"] > 1000 and 2 * st["long_codes"] > st["symbols"]
    for n in _names(kind="tables-flat") + _names(kind="bands-64"):
        st = _decoded(n)[2]
        assert st["symbols"] > 1000 and st["long_codes"] == 0
        info = parse_progressive_jpeg(SCRIPTS[n].data)
        lengths = {ln + 1 for _, bits, _ in _scan_tables(info)[0] for ln in range(16) if bits[ln]}
        assert lengths == {8, 9}                                       # the last code the lookahead table holds, and the one before
    for n in _names(kind="tables-one-id"):
        data = SCRIPTS[n].data
        dht = [i for i in range(len(data) - 4) if data[i:i + 2] == b"\xff\xc4" and data[i + 4] & 15 == 0]
        assert len(dht) >= len(SCRIPTS[n].script) - 2                  # a table in id 0 before every scan that has symbols
    for n in _names(kind="resplit-join") + _names(kind="resplit-split") + _names(kind="component-major"):
        assert _decoded(n)[2]["levels"] == 2 and _decoded(n)[2]["corrections"] > 0


def test_64_scans_parse_and_65_do_not():
    (n64,), (n65,) = _names(kind="bands-64"), _names(kind="bands-65")
    info = parse_progressive_jpeg(SCRIPTS[n64].data)
    assert len(info.scans) == MAX_SCANS == 64 and all(s.ss == s.se for s in info.scans)
    assert len(_scan_tables(info)[0]) == 2                              # one DC and one AC table, written 64 times
    assert len(SCRIPTS[n65].script) == 65 and parse_progressive_jpeg(SCRIPTS[n65].data) is None
    assert np.array_equal(K.reference(SCRIPTS[n65].data), K.reference(SCRIPTS[n65].source))      # (a file libjpeg takes)


def test_more_tables_than_a_decoder_plans_do_not_fit():
    from poco_amd.jpeg import ProgressiveJpegDecoder
    (name,) = _names(kind="tables-many")
    info = parse_progressive_jpeg(SCRIPTS[name].data)
    assert info is not None and len(_scan_tables(info)[0]) > TABLES_PER_IMAGE == 16
    dec = ProgressiveJpegDecoder.__new__(ProgressiveJpegDecoder)      # fits() reads the planned sizes only: no device is needed
    dec.max_h = dec.max_w = 256
    assert not dec.fits(info)
    assert dec.fits(parse_progressive_jpeg(SCRIPTS[_names(kind="bands-64")[0]].data))


@pytest.mark.parametrize("name", _names(kind="ends-above-zero"))
def test_script_that_ends_above_zero_is_declined(name):
    """libjpeg smooths the blocks of such pictures (jdcoefct.c): without that the restatement - and the device - would give
    other pixels than PIL with status 0 (73875 of 90000 bytes, up to 12 levels, for 420-q75-200x150 cut after five scans).
    The parser declines them, so every caller decodes them with PIL."""
    c = SCRIPTS[name]
    K.reference(c.data)                                                 # a file PIL takes
    assert parse_progressive_jpeg(c.data) is None and parse_jpeg(c.data) is None
    with pytest.raises(P.JpegError):
        P.decode_status(c.data)
    # the same bytes without their EOI are a file cut short: parsed, and damaged whatever the last scan decodes to
    info = parse_progressive_jpeg(c.data[:-2])
    assert info is not None and info.cut
    assert P.decode_status(c.data[:-2]) == (None, P.ERR_SHORT)
