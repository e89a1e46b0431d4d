"""CPU: the progressive JPEG parser (poco_amd.jpeg.parse_progressive_jpeg) and the numpy restatement of the progressive coefficient
stage (tests/jpegprog_np.py), which must give PIL's pixels byte for byte - the contract csrc/jpeg_prog.hip is tested against on
the GPU (tests/test_jpegprog_gpu.py)."""
import io

import numpy as np
import pytest
from PIL import Image

from tests import jpegprog_cases as K
from tests import jpegprog_np as P
from poco_amd import _lib
from poco_amd.jpeg import MAX_SCANS, parse_jpeg, parse_progressive_jpeg

CASES = K.cases()


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
    assert info is not None and len(info.scans) == 5
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
