"""Rendered frames as baseline JPEG, encoded on the GPU where they are (a binding of poco_jpeg_* in include/poco_hip.h,
csrc/jpeg_enc.hip), and a Motion-JPEG .avi writer on top of it: the result video the reference makes with ffmpeg
(demo.py:148-157, demo_utils.py:237-245 images_to_video, -pix_fmt yuv420p) without shelling out.

    enc = JpegEncoder(device, 1080, 1920)
    data = enc.encode(frame_u8_cuda, quality=90)          # bytes of a .jpg file: a few hundred KB cross PCIe instead of 6 MB
    with MjpegWriter("out.avi", 1920, 1080, fps=30) as w:
        w.add(data)

The way back is here too: parse_jpeg walks a file's markers on the host, JpegDecoder hands the entropy-coded bytes of a whole
batch to the device decoder (poco_jpeg_decode, csrc/jpeg_dec.hip) and MjpegReader reads a Motion-JPEG .avi frame by frame.

    dec = JpegDecoder(device, 1080, 1920, max_batch=16, max_bytes=32 << 20)
    frames = dec.decode([open(p, "rb").read() for p in paths])       # uint8 [H,W,3] device tensors, PIL's pixels
    for data in MjpegReader("movie.avi"): ...

Progressive files (SOF2) have their own pair: parse_progressive_jpeg records every scan of the file, ProgressiveJpegDecoder
(poco_jpeg_prog_decode, csrc/jpeg_prog.hip) decodes a batch of them with the same call shape.
"""
from __future__ import annotations

import ctypes as C
import struct
from dataclasses import dataclass
from typing import List, Optional

import numpy as np
import torch

from ._lib import PocoHipError, check, lib

HEADER_BYTES = 629
MAX_SIDE = 16384
AVI_MAX_BYTES = (1 << 31) - 1          # one RIFF chunk; OpenDML (AVIX) is not written


def worst_case_bytes(H: int, W: int) -> int:
    """The out_cap poco_jpeg_encode asks for: header + per MCU row (6 blocks per MCU, 64 x 27 bits each, doubled by byte
    stuffing) + its marker."""
    return HEADER_BYTES + ((H + 15) // 16) * (((W + 15) // 16) * 6 * 432 + 2)


class JpegEncoder:
    """Baseline JPEG (4:2:0, Annex K Huffman tables, one restart interval per MCU row) of uint8 [H,W,3] RGB device frames up to
    max_h x max_w.  All scratch is planned here; encode / encode_into allocate nothing on the C side."""

    def __init__(self, device, max_h: int, max_w: int):
        max_h, max_w = int(max_h), int(max_w)
        if not (1 <= max_h <= MAX_SIDE and 1 <= max_w <= MAX_SIDE):
            raise PocoHipError(f"JpegEncoder: max_h, max_w must be in 1..{MAX_SIDE}, got {max_h} x {max_w}")
        self.max_h, self.max_w = max_h, max_w
        self._h = C.c_void_p()
        self._out = None
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        L = lib()
        L.poco_jpeg_encoder_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.poco_jpeg_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p,
                                       C.c_void_p]
        L.poco_jpeg_encoder_destroy.argtypes = [C.c_void_p]
        L.poco_jpeg_encoder_destroy.restype = None
        with torch.cuda.device(self.device):
            check(L.poco_jpeg_encoder_create(max_h, max_w, C.byref(self._h)), "poco_jpeg_encoder_create")

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().poco_jpeg_encoder_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def encode_into(self, frame: torch.Tensor, out: torch.Tensor, quality: int = 90, length: torch.Tensor = None):
        """Enqueue the encode of `frame` (contiguous uint8 [H,W,3] on the device) into `out` (uint8, at least
        worst_case_bytes(H, W) long) on the current stream; returns (out, length) with `length` an int32 [1] device tensor
        holding the number of bytes.  No host synchronisation."""
        if not (torch.is_tensor(frame) and frame.device.type == "cuda" and frame.dtype == torch.uint8 and frame.dim() == 3
                and frame.shape[2] == 3 and frame.is_contiguous()):
            raise PocoHipError("JpegEncoder: frame must be a contiguous uint8 [H,W,3] device tensor")
        if not (torch.is_tensor(out) and out.device == frame.device and out.dtype == torch.uint8 and out.is_contiguous()):
            raise PocoHipError("JpegEncoder: out must be a contiguous uint8 tensor on the frame's device")
        if not 1 <= int(quality) <= 100:
            raise PocoHipError(f"JpegEncoder: quality must be in 1..100, got {quality}")
        if length is None:
            length = torch.empty(1, dtype=torch.int32, device=frame.device)
        elif not (torch.is_tensor(length) and length.device == frame.device and length.dtype == torch.int32 and length.numel() >= 1):
            raise PocoHipError("JpegEncoder: length must be an int32 tensor on the frame's device")
        check(lib().poco_jpeg_encode(self._h, frame.data_ptr(), int(frame.shape[0]), int(frame.shape[1]), int(quality),
                                     out.data_ptr(), out.numel(), length.data_ptr(),
                                     C.c_void_p(torch.cuda.current_stream(frame.device).cuda_stream)), "poco_jpeg_encode")
        return out, length

    def encode(self, frame: torch.Tensor, quality: int = 90) -> bytes:
        """The bytes of the .jpg file of `frame`: the length and exactly that many bytes are copied to the host."""
        if self._out is None:
            self._out = torch.empty(worst_case_bytes(self.max_h, self.max_w), dtype=torch.uint8, device=self.device)
        out, length = self.encode_into(frame, self._out, quality)
        return out[:int(length.item())].cpu().numpy().tobytes()


class MjpegWriter:
    """A plain RIFF AVI file with one Motion-JPEG video stream: hdrl (avih, one strl: strh vids/MJPG + strf BITMAPINFOHEADER),
    movi (one word-aligned 00dc chunk per frame), idx1.  close() writes the index and patches sizes and frame counts.  Files are
    held below 2 GB (one RIFF chunk): a frame that would cross it is refused."""

    def __init__(self, path: str, width: int, height: int, fps: float = 30.0):
        width, height, fps = int(width), int(height), float(fps)
        if not (1 <= width <= 65535 and 1 <= height <= 65535):
            raise ValueError(f"MjpegWriter: width and height must be in 1..65535, got {width} x {height}")
        if not 0 < fps <= 1000:
            raise ValueError(f"MjpegWriter: fps must be in (0, 1000], got {fps}")
        self.width, self.height, self.fps = width, height, fps
        self._scale = 1 if fps == int(fps) else 1000
        self._rate = int(round(fps * self._scale))
        self._index = []                # (offset from the 'movi' fourcc, size) per frame
        self._max = 0
        self._f = open(path, "wb")
        self._f.write(self._headers(0))
        self._movi = self._f.tell() - 4  # position of the 'movi' fourcc
        self._pos = self._f.tell()

    def _headers(self, movi_bytes: int) -> bytes:
        n = len(self._index)
        avih = struct.pack("<14I", int(round(1e6 * self._scale / self._rate)), int(self._max * self._rate / self._scale), 0, 0x10,
                           n, 0, 1, self._max, self.width, self.height, 0, 0, 0, 0)
        strh = struct.pack("<4s4sIHHIIIIIIII4H", b"vids", b"MJPG", 0, 0, 0, 0, self._scale, self._rate, 0, n, self._max,
                           0xFFFFFFFF, 0, 0, 0, self.width, self.height)
        strf = struct.pack("<IiiHH4sIiiII", 40, self.width, self.height, 1, 24, b"MJPG", self.width * self.height * 3, 0, 0, 0, 0)
        strl = b"strl" + b"strh" + struct.pack("<I", len(strh)) + strh + b"strf" + struct.pack("<I", len(strf)) + strf
        hdrl = b"hdrl" + b"avih" + struct.pack("<I", len(avih)) + avih + b"LIST" + struct.pack("<I", len(strl)) + strl
        body = b"AVI " + b"LIST" + struct.pack("<I", len(hdrl)) + hdrl + b"LIST" + struct.pack("<I", 4 + movi_bytes) + b"movi"
        riff = len(body) + movi_bytes + (8 + 16 * n)
        return b"RIFF" + struct.pack("<I", riff) + body

    def add(self, jpeg: bytes) -> None:
        """Append one frame: the bytes of a JPEG file (JpegEncoder.encode) of the writer's size."""
        if self._f is None:
            raise ValueError("MjpegWriter: add() after close()")
        data = bytes(jpeg)
        if len(data) < 4 or data[:2] != b"\xff\xd8":
            raise ValueError("MjpegWriter: a frame must be the bytes of a JPEG file (it starts with SOI, FF D8)")
        padded = len(data) + (len(data) & 1)
        if self._pos + 8 + padded + 8 + 16 * (len(self._index) + 1) > AVI_MAX_BYTES:
            raise ValueError(f"MjpegWriter: frame {len(self._index)} would take the file past 2 GB; AVI files over 2 GB "
                             "(OpenDML) are not written - close this file and start another")
        self._f.write(b"00dc" + struct.pack("<I", len(data)) + data + b"\0" * (padded - len(data)))
        self._index.append((self._pos - self._movi, len(data)))
        self._max = max(self._max, len(data))
        self._pos += 8 + padded

    @property
    def frames(self) -> int:
        return len(self._index)

    def close(self) -> None:
        if self._f is None:
            return
        idx = b"".join(struct.pack("<4sIII", b"00dc", 0x10, off, size) for off, size in self._index)
        self._f.write(b"idx1" + struct.pack("<I", len(idx)) + idx)
        self._f.seek(0)
        self._f.write(self._headers(self._pos - self._movi - 4))
        self._f.close()
        self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


# ---- decoding: the marker walk, the device decoder's binding, the .avi reader ----------------------------------------------------
SUBSEQ_BYTES = 128                     # the device's subsequence size (JD_SUBSEQ in csrc/jpeg_dec.hip)
SEGS_PER_IMAGE = 2048                  # restart intervals a decoder plans per image of its batch (JD_SEGS_PER_IMAGE there)

# ITU-T T.81 Annex K: the tables of a frame that carries no DHT (Motion-JPEG frames inside AVI commonly omit them)
_K_DC_BITS = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], [0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0])
_K_AC_BITS = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7D], [0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77])
_K_AC_VALS = (bytes.fromhex(
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546"
    "4748494a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8"
    "b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa"), bytes.fromhex(
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445"
    "464748494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6"
    "b7b8b9bac2c3c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa"))
ANNEX_K_TABLES = {(0, t): (bytes(_K_DC_BITS[t]), bytes(range(12))) for t in (0, 1)}
ANNEX_K_TABLES.update({(1, t): (bytes(_K_AC_BITS[t]), _K_AC_VALS[t]) for t in (0, 1)})

_ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21,
                    28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61,
                    54, 47, 55, 62, 63])


@dataclass
class JpegInfo:
    """What parse_jpeg found.  Tables are per component, as the frame and scan headers select them."""
    height: int
    width: int
    ncomp: int                         # 1 (grayscale) or 3 (YCbCr)
    hsamp: int                         # luma sampling, chroma is 1 x 1: (1,1) 4:4:4, (2,1) 4:2:2, (2,2) 4:2:0
    vsamp: int
    qt: np.ndarray                     # uint16 [ncomp, 64], natural (row-major) order
    dc: list                           # per component (bits: 16 bytes, huffval: bytes)
    ac: list
    restart_interval: int              # MCUs per restart interval, 0 = none
    scan_offset: int                   # the entropy-coded data: data[scan_offset : scan_offset + scan_length]
    scan_length: int
    segments: np.ndarray               # uint32 [nseg, 3]: offset from scan_offset, length, first MCU of every restart interval
    data: bytes

    @property
    def mcus(self):
        """(MCU rows, MCU columns)"""
        return (-(-self.height // (8 * self.vsamp)), -(-self.width // (8 * self.hsamp)))


def _parse(data: bytes) -> Optional[JpegInfo]:
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        return None
    qts, huff = {}, {}
    frame, dri, adobe = None, 0, None
    i = 2
    while True:
        if i + 4 > n or data[i] != 0xFF:
            return None
        m = data[i + 1]
        if m == 0xFF:                  # fill byte
            i += 1
            continue
        ln = (data[i + 2] << 8) | data[i + 3]
        if m in (0xD8, 0xD9, 0x01) or 0xD0 <= m <= 0xD7 or ln < 2 or i + 2 + ln > n:
            return None
        p = data[i + 4:i + 2 + ln]
        i += 2 + ln
        if m == 0xC0:
            if frame is not None or len(p) < 6 or p[0] != 8:
                return None
            H, W, nc = (p[1] << 8) | p[2], (p[3] << 8) | p[4], p[5]
            if len(p) != 6 + 3 * nc or nc not in (1, 3) or not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
                return None
            frame = (H, W, [(p[6 + 3 * c], p[7 + 3 * c] >> 4, p[7 + 3 * c] & 15, p[8 + 3 * c]) for c in range(nc)])
        elif 0xC1 <= m <= 0xCF and m not in (0xC4, 0xC8, 0xCC):
            return None                # extended, progressive, lossless, arithmetic: not decoded here
        elif m == 0xCC:
            return None
        elif m == 0xC4:
            j = 0
            while j < len(p):
                if j + 17 > len(p):
                    return None
                tc, th = p[j] >> 4, p[j] & 15
                cnt = sum(p[j + 1:j + 17])
                if tc > 1 or th > 3 or cnt > 256 or j + 17 + cnt > len(p):
                    return None
                huff[(tc, th)] = (bytes(p[j + 1:j + 17]), bytes(p[j + 17:j + 17 + cnt]))
                j += 17 + cnt
        elif m == 0xDB:
            j = 0
            while j < len(p):
                if p[j] >> 4 != 0 or (p[j] & 15) > 3 or j + 65 > len(p):       # 16-bit entries: not baseline
                    return None
                q = np.zeros(64, np.uint16)
                q[_ZIGZAG] = np.frombuffer(p[j + 1:j + 65], np.uint8)
                qts[p[j] & 15] = q
                j += 65
        elif m == 0xDD:
            if len(p) != 2:
                return None
            dri = (p[0] << 8) | p[1]
        elif m == 0xEE and len(p) >= 12 and p[:5] == b"Adobe":
            adobe = p[11]
        elif m == 0xDA:
            break
        # other APPn (JFIF, Exif ...) and COM: skipped
    if frame is None:
        return None
    H, W, comps = frame
    nc = len(comps)
    if len(p) != 4 + 2 * nc or p[0] != nc or p[1 + 2 * nc] != 0 or p[2 + 2 * nc] != 63 or p[3 + 2 * nc] != 0:
        return None                    # not one interleaved scan of all components
    if nc == 3:
        if [c[0] for c in comps] == [82, 71, 66] or adobe == 0 or adobe == 2:      # RGB / YCCK files
            return None
        if (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
            return None
    elif (comps[0][1], comps[0][2]) != (1, 1):
        return None
    hs, vs = comps[0][1], comps[0][2]
    dc, ac, qt = [], [], np.zeros((nc, 64), np.uint16)
    for c in range(nc):
        if p[1 + 2 * c] != comps[c][0] or comps[c][3] not in qts:
            return None
        td, ta = p[2 + 2 * c] >> 4, p[2 + 2 * c] & 15
        qt[c] = qts[comps[c][3]]
        for tc, th, dst in ((0, td, dc), (1, ta, ac)):
            t = huff.get((tc, th)) if huff else ANNEX_K_TABLES.get((tc, th))
            if t is None or not _prefix_code(t[0]) or (tc == 0 and (len(t[1]) > 16 or any(v > 15 for v in t[1]))):
                return None
            dst.append(t)
    # the entropy-coded data ends at the first marker that is neither stuffing nor RSTm; anything but EOI there is another scan
    a = np.frombuffer(data, np.uint8, offset=i)
    ff = np.flatnonzero(a[:-1] == 0xFF) if a.size > 1 else np.zeros(0, np.int64)
    nxt = a[ff + 1]
    is_rst = (nxt >= 0xD0) & (nxt <= 0xD7)
    other = ff[(nxt != 0) & ~is_rst & (nxt != 0xFF)]
    end = a.size                       # a truncated file: the device reports it in the image's status word
    if other.size:
        if a[other[0] + 1] != 0xD9:
            return None
        end = int(other[0])
    rst = ff[is_rst & (ff < end)]
    mcuy, mcux = -(-H // (8 * vs)), -(-W // (8 * hs))
    nmcu = mcuy * mcux
    if dri == 0 or rst.size == 0:
        segs = np.array([[0, end, 0]], np.uint32)
    else:
        if rst.size > (nmcu - 1) // dri or not np.array_equal(a[rst + 1] - 0xD0, np.arange(rst.size) & 7):
            return None
        start = np.concatenate([[0], rst + 2])
        stop = np.concatenate([rst, [end]])
        segs = np.stack([start, stop - start, np.arange(start.size) * dri], 1).astype(np.uint32)
    return JpegInfo(H, W, nc, hs, vs, qt, dc, ac, dri, i, end, segs, data)


def _prefix_code(bits: bytes) -> bool:
    """Kraft: the counts per length describe a prefix code that leaves the all-ones code word free."""
    code = 0
    for ln in range(16):
        code += bits[ln]
        if bits[ln] and code >= (2 << ln):
            return False
        code <<= 1
    return any(bits)


def parse_jpeg(data) -> Optional[JpegInfo]:
    """The marker walk of one .jpg file: sizes, sampling, tables, the restart interval and the table of restart intervals of
    its entropy-coded data - or None for a file the device decoder does not take (progressive, lossless, arithmetic coding, 12
    bit, CMYK / YCCK / RGB, other sampling factors, more than one scan, a damaged header); the caller then decodes with PIL.  A
    file cut short inside its scan is parsed: the decoder reports it in the image's status word."""
    try:
        return _parse(bytes(data))
    except (IndexError, ValueError):
        return None


# ---- progressive files: the scan table --------------------------------------------------------------------------------------------
MAX_SCANS = 64                         # scans a progressive file may have (JP_MAX_SCANS in csrc/jpeg_prog.hip)
TABLES_PER_IMAGE = 16                  # distinct Huffman tables a decoder plans per image of its batch (JP_TABS_PER_IMAGE there)


@dataclass
class ProgressiveScan:
    """One SOS of a progressive file and the tables in force there."""
    comps: tuple                       # indices into the frame's components
    ss: int
    se: int
    ah: int
    al: int
    dc: list                           # per component of the scan (bits, huffval) - of a first DC scan, else None
    ac: Optional[tuple]                # (bits, huffval) of an AC scan (first or refinement), else None
    offset: int                        # the entropy-coded bytes: data[offset : offset + length], up to the next marker
    length: int


@dataclass
class ProgressiveJpegInfo:
    """What parse_progressive_jpeg found."""
    height: int
    width: int
    ncomp: int                         # 1 (grayscale) or 3 (YCbCr)
    hsamp: int                         # luma sampling, chroma is 1 x 1
    vsamp: int
    qt: np.ndarray                     # uint16 [ncomp, 64], natural order: the table in force at the component's first scan
    scans: list                        # ProgressiveScan, in file order
    data: bytes
    cut: bool = False                  # the file ends inside (or right after) its last scan, without EOI

    @property
    def mcus(self):
        """(MCU rows, MCU columns)"""
        return (-(-self.height // (8 * self.vsamp)), -(-self.width // (8 * self.hsamp)))

    @property
    def stream_length(self) -> int:
        """Bytes from the first scan's data to the end of the last: what a decode call copies to the device."""
        return self.scans[-1].offset + self.scans[-1].length - self.scans[0].offset


def _parse_progressive(data: bytes) -> Optional[ProgressiveJpegInfo]:
    n = len(data)
    if n < 4 or data[0] != 0xFF or data[1] != 0xD8:
        return None
    a = np.frombuffer(data, np.uint8)
    markers = np.flatnonzero((a[:-1] == 0xFF) & (a[1:] != 0))       # every FF that is no stuffed data byte
    qts, huff = {}, {}
    frame, adobe = None, None
    scans, qt, coef_bits = [], None, None
    cut = False
    i = 2
    while True:
        if i >= n and scans:           # cut short inside (or right after) a scan: the device reports it
            cut = True
            break
        if i + 2 > n or data[i] != 0xFF:
            return None
        m = data[i + 1]
        if m == 0xFF:                  # fill byte
            i += 1
            continue
        if m == 0xD9:
            break
        if i + 4 > n:
            return None
        ln = (data[i + 2] << 8) | data[i + 3]
        if m in (0xD8, 0x01) or 0xD0 <= m <= 0xD7 or ln < 2 or i + 2 + ln > n:
            return None
        p = data[i + 4:i + 2 + ln]
        i += 2 + ln
        if m == 0xC2:
            if frame is not None or len(p) < 6 or p[0] != 8:
                return None
            H, W, nc = (p[1] << 8) | p[2], (p[3] << 8) | p[4], p[5]
            if len(p) != 6 + 3 * nc or nc not in (1, 3) or not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
                return None
            comps = [(p[6 + 3 * c], p[7 + 3 * c] >> 4, p[7 + 3 * c] & 15, p[8 + 3 * c]) for c in range(nc)]
            if len({c[0] for c in comps}) != nc:
                return None
            if nc == 3:
                if (comps[0][1], comps[0][2]) not in ((1, 1), (2, 1), (2, 2)) or any((c[1], c[2]) != (1, 1) for c in comps[1:]):
                    return None
            elif (comps[0][1], comps[0][2]) != (1, 1):
                return None
            frame = (H, W, comps)
            qt = np.zeros((nc, 64), np.uint16)
            coef_bits = np.full((nc, 64), -1, np.int64)             # jdphuff.c: the Al each coefficient has been sent down to
        elif 0xC0 <= m <= 0xCF and m not in (0xC4, 0xC8):
            return None                # baseline, extended, lossless, arithmetic (and DAC): not decoded here
        elif m == 0xC4:
            j = 0
            while j < len(p):
                if j + 17 > len(p):
                    return None
                tc, th = p[j] >> 4, p[j] & 15
                cnt = sum(p[j + 1:j + 17])
                if tc > 1 or th > 3 or cnt > 256 or j + 17 + cnt > len(p):
                    return None
                huff[(tc, th)] = (bytes(p[j + 1:j + 17]), bytes(p[j + 17:j + 17 + cnt]))
                j += 17 + cnt
        elif m == 0xDB:
            j = 0
            while j < len(p):
                if p[j] >> 4 != 0 or (p[j] & 15) > 3 or j + 65 > len(p):
                    return None
                q = np.zeros(64, np.uint16)
                q[_ZIGZAG] = np.frombuffer(p[j + 1:j + 65], np.uint8)
                qts[p[j] & 15] = q
                j += 65
        elif m == 0xDD:
            if len(p) != 2 or p[0] or p[1]:
                return None            # restart intervals in a progressive file: left to PIL
        elif m == 0xEE and len(p) >= 12 and p[:5] == b"Adobe":
            adobe = p[11]
        elif m == 0xDA:
            if frame is None or len(scans) >= MAX_SCANS or len(p) < 1:
                return None
            H, W, comps = frame
            nc = len(comps)
            if nc == 3 and not scans and ([c[0] for c in comps] == [82, 71, 66] or adobe == 0 or adobe == 2):
                return None            # RGB / YCCK files
            ns = p[0]
            if len(p) != 4 + 2 * ns or ns not in (1, nc):
                return None
            ss, se, ah, al = p[1 + 2 * ns], p[2 + 2 * ns], p[3 + 2 * ns] >> 4, p[3 + 2 * ns] & 15
            ids = [c[0] for c in comps]
            if any(p[1 + 2 * k] not in ids for k in range(ns)):
                return None
            cs = tuple(ids.index(p[1 + 2 * k]) for k in range(ns))
            if ns > 1 and cs != tuple(range(nc)):
                return None
            # jdphuff.c start_pass_phuff_decoder, with its warnings taken as errors
            if (ss == 0 and se != 0) or (ss > 0 and (se < ss or se > 63 or ns != 1)) or al > 13 or (ah != 0 and ah != al + 1):
                return None
            dc, ac = [None] * ns, None
            for k, c in enumerate(cs):
                if ss > 0 and coef_bits[c, 0] < 0:
                    return None        # an AC scan before the component's DC scan
                band = coef_bits[c, ss:se + 1]
                if np.any(band != (ah if ah else -1)):
                    return None        # a first scan of coefficients sent before, or a refinement that does not follow Al = Ah
                if np.all(coef_bits[c] < 0):
                    if comps[c][3] not in qts:
                        return None
                    qt[c] = qts[comps[c][3]]
                band[:] = al
                td, ta = p[2 + 2 * k] >> 4, p[2 + 2 * k] & 15
                if ss == 0 and ah == 0:
                    dc[k] = t = huff.get((0, td))
                    if t is None or not _prefix_code(t[0]) or len(t[1]) > 16 or any(v > 15 for v in t[1]):
                        return None
                elif ss > 0:
                    ac = t = huff.get((1, ta))
                    if t is None or not _prefix_code(t[0]):
                        return None
            j = int(np.searchsorted(markers, i))
            end = int(markers[j]) if j < markers.size else n
            scans.append(ProgressiveScan(cs, ss, se, ah, al, dc, ac, i, end - i))
            i = end
        # other APPn (JFIF, Exif ...) and COM: skipped
    if frame is None or not scans or np.any(coef_bits < 0):
        return None                    # a coefficient no scan sends: libjpeg smooths such blocks, this decoder does not
    if np.any(coef_bits > 0) and not cut:
        return None                    # a script that ends above Al = 0: libjpeg smooths such pictures too (jdcoefct.c smoothing_ok)
    H, W, comps = frame
    return ProgressiveJpegInfo(H, W, len(comps), comps[0][1], comps[0][2], qt, scans, data, cut)


def parse_progressive_jpeg(data) -> Optional[ProgressiveJpegInfo]:
    """The marker walk of one progressive .jpg file (SOF2, 8 bit, Huffman): sizes, sampling, quantisation tables and per scan its
    components, band (Ss, Se), successive approximation (Ah, Al), the Huffman tables in force at its SOS and where its
    entropy-coded bytes lie - or None for a file ProgressiveJpegDecoder does not take (baseline - that is parse_jpeg's -,
    arithmetic coding, 12 bit, CMYK / YCCK / RGB, other sampling factors, a restart interval, more than 64 scans, a scan of two
    of three components, a scan script that breaks jdphuff.c's rules, leaves a coefficient of a component without any scan or
    ends with any coefficient of any component above Al = 0 - libjpeg smooths the blocks of such pictures, this decoder does
    not, so only PIL gives PIL's pixels for them -, a damaged header); the caller then decodes with PIL.  A file cut short
    inside a scan (no EOI behind its last scan; `cut` is set) keeps being parsed when the scans it still has cover every
    coefficient, whatever Al they end at: it yields no pixels, the decoder reports it in the image's status word - non-zero
    whenever the script it still has ends above Al = 0, also when the cut falls exactly between two scans.  A file may hold more
    distinct Huffman tables than a decoder plans per image (TABLES_PER_IMAGE): it is parsed, ProgressiveJpegDecoder.fits says
    no and decode refuses it."""
    try:
        return _parse_progressive(bytes(data))
    except (IndexError, ValueError):
        return None


class _CImage(C.Structure):
    _fields_ = [("data", C.c_void_p), ("nbytes", C.c_size_t), ("segs", C.c_void_p), ("nseg", C.c_int), ("H", C.c_int),
                ("W", C.c_int), ("ncomp", C.c_int), ("hsamp", C.c_int), ("vsamp", C.c_int), ("qt", C.c_uint16 * 64 * 3),
                ("dc_bits", C.c_uint8 * 16 * 3), ("dc_vals", C.c_uint8 * 16 * 3), ("ac_bits", C.c_uint8 * 16 * 3),
                ("ac_vals", C.c_uint8 * 256 * 3), ("d_rgb", C.c_void_p)]


class JpegDecoder:
    """Baseline JPEG files -> uint8 [H,W,3] RGB device tensors holding the pixels PIL gives, up to max_batch images of up to
    max_h x max_w and max_bytes of entropy-coded data and tables per call, of mixed sizes and samplings.  Device scratch and
    the pinned staging buffer are planned here; decode / decode_into allocate nothing on the C side."""

    def __init__(self, device, max_h: int, max_w: int, max_batch: int = 1, max_bytes: int = 0):
        max_h, max_w, max_batch = int(max_h), int(max_w), int(max_batch)
        max_bytes = int(max_bytes) or max_batch * max(1 << 16, max_h * max_w)
        if not (1 <= max_h <= MAX_SIDE and 1 <= max_w <= MAX_SIDE):
            raise PocoHipError(f"JpegDecoder: max_h, max_w must be in 1..{MAX_SIDE}, got {max_h} x {max_w}")
        if not 1 <= max_batch <= 4096:
            raise PocoHipError(f"JpegDecoder: max_batch must be in 1..4096, got {max_batch}")
        if not 1 <= max_bytes <= 1 << 30:
            raise PocoHipError(f"JpegDecoder: max_bytes must be in 1..2^30, got {max_bytes}")
        self.max_h, self.max_w, self.max_batch, self.max_bytes = max_h, max_w, max_batch, max_bytes
        self._h = C.c_void_p()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        L = lib()
        L.poco_jpeg_decoder_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
        L.poco_jpeg_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.poco_jpeg_decoder_destroy.argtypes = [C.c_void_p]
        L.poco_jpeg_decoder_destroy.restype = None
        with torch.cuda.device(self.device):
            check(L.poco_jpeg_decoder_create(max_h, max_w, max_batch, max_bytes, C.byref(self._h)), "poco_jpeg_decoder_create")

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().poco_jpeg_decoder_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def fits(self, info: JpegInfo) -> bool:
        """The picture's size and its number of restart intervals are within what every image of a batch may have."""
        return info.height <= self.max_h and info.width <= self.max_w and len(info.segments) <= SEGS_PER_IMAGE

    def decode_into(self, images, outs, status: torch.Tensor = None) -> torch.Tensor:
        """Enqueue the decode of `images` (bytes of .jpg files or JpegInfo, at most max_batch) into `outs` (contiguous uint8
        [H,W,3] device tensors of the files' sizes) on the current stream: one host-to-device copy, no host synchronisation.
        Returns `status`, an int32 [n] device tensor: 0 per decoded image, non-zero for a damaged stream."""
        infos = []
        for im in images:
            info = im if isinstance(im, JpegInfo) else parse_jpeg(im)
            if info is None:
                raise PocoHipError("JpegDecoder: not a baseline JPEG file this decoder takes (parse_jpeg returned None)")
            infos.append(info)
        n = len(infos)
        if not 1 <= n <= self.max_batch:
            raise PocoHipError(f"JpegDecoder: {n} images in one call, the decoder was created for 1..{self.max_batch}")
        if len(outs) != n:
            raise PocoHipError(f"JpegDecoder: {n} images but {len(outs)} output tensors")
        for info, o in zip(infos, outs):
            if not (torch.is_tensor(o) and o.device == self.device and o.dtype == torch.uint8 and o.is_contiguous()
                    and tuple(o.shape) == (info.height, info.width, 3)):
                raise PocoHipError(f"JpegDecoder: an output must be a contiguous uint8 [{info.height},{info.width},3] tensor on "
                                   f"{self.device}")
        if status is None:
            status = torch.empty(n, dtype=torch.int32, device=self.device)
        elif not (torch.is_tensor(status) and status.device == self.device and status.dtype == torch.int32
                  and status.is_contiguous() and status.numel() >= n):
            raise PocoHipError("JpegDecoder: status must be a contiguous int32 tensor of at least n elements on the decoder's device")
        arr = (_CImage * n)()
        keep = []
        for s, info, o in zip(arr, infos, outs):
            buf = np.frombuffer(info.data, np.uint8)
            segs = np.ascontiguousarray(info.segments, np.uint32)
            qt = np.ascontiguousarray(info.qt, np.uint16)
            keep += [buf, segs, qt]
            s.data, s.nbytes = buf.ctypes.data + info.scan_offset, info.scan_length
            s.segs, s.nseg = segs.ctypes.data, segs.shape[0]
            s.H, s.W, s.ncomp, s.hsamp, s.vsamp = info.height, info.width, info.ncomp, info.hsamp, info.vsamp
            C.memmove(s.qt, qt.ctypes.data, info.ncomp * 128)
            for c in range(info.ncomp):
                C.memmove(s.dc_bits[c], info.dc[c][0], 16)
                C.memmove(s.dc_vals[c], info.dc[c][1], len(info.dc[c][1]))
                C.memmove(s.ac_bits[c], info.ac[c][0], 16)
                C.memmove(s.ac_vals[c], info.ac[c][1], len(info.ac[c][1]))
            s.d_rgb = o.data_ptr()
        check(lib().poco_jpeg_decode(self._h, C.cast(arr, C.c_void_p), n, status.data_ptr(),
                                     C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "poco_jpeg_decode")
        return status

    def decode(self, images, return_status: bool = False):
        """The pictures of `images` as new device tensors.  return_status: also the list of status words (this reads them back,
        the call's only host synchronisation)."""
        infos = [im if isinstance(im, JpegInfo) else parse_jpeg(im) for im in images]
        if any(i is None for i in infos):
            raise PocoHipError("JpegDecoder: not a baseline JPEG file this decoder takes (parse_jpeg returned None)")
        outs = [torch.empty(i.height, i.width, 3, dtype=torch.uint8, device=self.device) for i in infos]
        status = self.decode_into(infos, outs)
        return (outs, status.cpu().tolist()) if return_status else outs


class _CProgTable(C.Structure):
    _fields_ = [("bits", C.c_uint8 * 16), ("vals", C.c_uint8 * 256)]


class _CProgScan(C.Structure):
    _fields_ = [("offset", C.c_uint), ("length", C.c_uint), ("ncomp", C.c_uint8), ("comp", C.c_uint8 * 3), ("ss", C.c_uint8),
                ("se", C.c_uint8), ("ah", C.c_uint8), ("al", C.c_uint8), ("tab", C.c_short * 3), ("flags", C.c_short)]


PROG_SCAN_CUT = 1                      # POCO_JPEG_PROG_SCAN_CUT


class _CProgImage(C.Structure):
    _fields_ = [("data", C.c_void_p), ("nbytes", C.c_size_t), ("scans", C.c_void_p), ("nscan", C.c_int), ("tables", C.c_void_p),
                ("ntable", C.c_int), ("H", C.c_int), ("W", C.c_int), ("ncomp", C.c_int), ("hsamp", C.c_int), ("vsamp", C.c_int),
                ("qt", C.c_uint16 * 64 * 3), ("d_rgb", C.c_void_p)]


def _scan_tables(info: ProgressiveJpegInfo):
    """The distinct Huffman tables of a file's scans, as (is AC, bits, huffval), and per scan the indices of its tables."""
    tables, index, per_scan = [], {}, []
    for sc in info.scans:
        used = [(1, *sc.ac)] if sc.ac is not None else [(0, *t) for t in sc.dc if t is not None]
        ids = []
        for t in used:
            if t not in index:
                index[t] = len(tables)
                tables.append(t)
            ids.append(index[t])
        per_scan.append(ids)
    return tables, per_scan


class ProgressiveJpegDecoder:
    """Progressive JPEG files -> uint8 [H,W,3] RGB device tensors holding the pixels PIL gives: JpegDecoder's call shape for the
    files parse_progressive_jpeg accepts (a binding of poco_jpeg_prog_* in include/poco_hip.h, csrc/jpeg_prog.hip).  Up to
    max_batch images of up to max_h x max_w and max_bytes of scan data per call, of mixed sizes, samplings and scan scripts."""

    def __init__(self, device, max_h: int, max_w: int, max_batch: int = 1, max_bytes: int = 0):
        max_h, max_w, max_batch = int(max_h), int(max_w), int(max_batch)
        max_bytes = int(max_bytes) or max_batch * max(1 << 16, max_h * max_w)
        if not (1 <= max_h <= MAX_SIDE and 1 <= max_w <= MAX_SIDE):
            raise PocoHipError(f"ProgressiveJpegDecoder: max_h, max_w must be in 1..{MAX_SIDE}, got {max_h} x {max_w}")
        if not 1 <= max_batch <= 4096:
            raise PocoHipError(f"ProgressiveJpegDecoder: max_batch must be in 1..4096, got {max_batch}")
        if not 1 <= max_bytes <= 1 << 30:
            raise PocoHipError(f"ProgressiveJpegDecoder: max_bytes must be in 1..2^30, got {max_bytes}")
        self.max_h, self.max_w, self.max_batch, self.max_bytes = max_h, max_w, max_batch, max_bytes
        self._h = C.c_void_p()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        L = lib()
        L.poco_jpeg_prog_decoder_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
        L.poco_jpeg_prog_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.poco_jpeg_prog_decoder_destroy.argtypes = [C.c_void_p]
        L.poco_jpeg_prog_decoder_destroy.restype = None
        with torch.cuda.device(self.device):
            check(L.poco_jpeg_prog_decoder_create(max_h, max_w, max_batch, max_bytes, C.byref(self._h)),
                  "poco_jpeg_prog_decoder_create")

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().poco_jpeg_prog_decoder_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def fits(self, info: ProgressiveJpegInfo) -> bool:
        """The picture's size and its number of distinct Huffman tables are within what every image of a batch may have."""
        return info.height <= self.max_h and info.width <= self.max_w and len(_scan_tables(info)[0]) <= TABLES_PER_IMAGE

    def decode_into(self, images, outs, status: torch.Tensor = None) -> torch.Tensor:
        """Enqueue the decode of `images` (bytes of progressive .jpg files or ProgressiveJpegInfo, at most max_batch) into `outs`
        (contiguous uint8 [H,W,3] device tensors of the files' sizes) on the current stream: one host-to-device copy, no host
        synchronisation.  Returns `status`, an int32 [n] device tensor: 0 per decoded image, non-zero for a damaged stream."""
        infos = []
        for im in images:
            info = im if isinstance(im, ProgressiveJpegInfo) else parse_progressive_jpeg(im)
            if info is None:
                raise PocoHipError("ProgressiveJpegDecoder: not a progressive JPEG file this decoder takes (parse_progressive_jpeg "
                                   "returned None)")
            infos.append(info)
        n = len(infos)
        if not 1 <= n <= self.max_batch:
            raise PocoHipError(f"ProgressiveJpegDecoder: {n} images in one call, the decoder was created for 1..{self.max_batch}")
        if len(outs) != n:
            raise PocoHipError(f"ProgressiveJpegDecoder: {n} images but {len(outs)} output tensors")
        for info, o in zip(infos, outs):
            if not (torch.is_tensor(o) and o.device == self.device and o.dtype == torch.uint8 and o.is_contiguous()
                    and tuple(o.shape) == (info.height, info.width, 3)):
                raise PocoHipError(f"ProgressiveJpegDecoder: an output must be a contiguous uint8 [{info.height},{info.width},3] "
                                   f"tensor on {self.device}")
        if status is None:
            status = torch.empty(n, dtype=torch.int32, device=self.device)
        elif not (torch.is_tensor(status) and status.device == self.device and status.dtype == torch.int32
                  and status.is_contiguous() and status.numel() >= n):
            raise PocoHipError("ProgressiveJpegDecoder: status must be a contiguous int32 tensor of at least n elements on the "
                               "decoder's device")
        arr = (_CProgImage * n)()
        keep = []
        for s, info, o in zip(arr, infos, outs):
            buf = np.frombuffer(info.data, np.uint8)
            qt = np.ascontiguousarray(info.qt, np.uint16)
            tables, per_scan = _scan_tables(info)
            ctab = (_CProgTable * max(1, len(tables)))()
            for ct, (_, bits, vals) in zip(ctab, tables):
                C.memmove(ct.bits, bits, 16)
                C.memmove(ct.vals, vals, len(vals))
            base = info.scans[0].offset
            cscan = (_CProgScan * len(info.scans))()
            for cs, sc, tabs in zip(cscan, info.scans, per_scan):
                cs.offset, cs.length, cs.ncomp = sc.offset - base, sc.length, len(sc.comps)
                cs.ss, cs.se, cs.ah, cs.al = sc.ss, sc.se, sc.ah, sc.al
                for k, c in enumerate(sc.comps):
                    cs.comp[k] = c
                for k, t in enumerate(tabs):
                    cs.tab[k] = t
            cscan[len(info.scans) - 1].flags = PROG_SCAN_CUT if info.cut else 0
            keep += [buf, qt, ctab, cscan]
            s.data, s.nbytes = buf.ctypes.data + base, info.stream_length
            s.scans, s.nscan = C.addressof(cscan), len(info.scans)
            s.tables, s.ntable = C.addressof(ctab), len(tables)
            s.H, s.W, s.ncomp, s.hsamp, s.vsamp = info.height, info.width, info.ncomp, info.hsamp, info.vsamp
            C.memmove(s.qt, qt.ctypes.data, info.ncomp * 128)
            s.d_rgb = o.data_ptr()
        check(lib().poco_jpeg_prog_decode(self._h, C.cast(arr, C.c_void_p), n, status.data_ptr(),
                                          C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "poco_jpeg_prog_decode")
        return status

    def decode(self, images, return_status: bool = False):
        """The pictures of `images` as new device tensors.  return_status: also the list of status words (this reads them back,
        the call's only host synchronisation)."""
        infos = [im if isinstance(im, ProgressiveJpegInfo) else parse_progressive_jpeg(im) for im in images]
        if any(i is None for i in infos):
            raise PocoHipError("ProgressiveJpegDecoder: not a progressive JPEG file this decoder takes (parse_progressive_jpeg "
                               "returned None)")
        outs = [torch.empty(i.height, i.width, 3, dtype=torch.uint8, device=self.device) for i in infos]
        status = self.decode_into(infos, outs)
        return (outs, status.cpu().tolist()) if return_status else outs


class MjpegReader:
    """A plain RIFF AVI file with one Motion-JPEG video stream, frame by frame: the inverse of MjpegWriter.  width, height and
    fps come from avih / strh, the frame table from idx1 when the file has one and from a walk of movi otherwise.  len(),
    reader[i] (the bytes of frame i's JPEG file) and iteration; each access reads from the file, nothing is held."""

    def __init__(self, path: str):
        self.path = path
        self._f = open(path, "rb")
        try:
            self._read_headers()
        except Exception:
            self._f.close()
            raise

    def _read_headers(self):
        f = self._f
        size = f.seek(0, 2)
        f.seek(0)
        head = f.read(12)
        if len(head) < 12 or head[:4] != b"RIFF" or head[8:12] != b"AVI ":
            raise ValueError(f"MjpegReader: {self.path} is not a RIFF AVI file; only Motion-JPEG AVI is read - extract the frames "
                             "to a folder and pass the folder")
        riff_end = min(size, 8 + struct.unpack("<I", head[4:8])[0])
        self.width = self.height = 0
        self.fps = 0.0
        handler, stream_type, movi, idx = None, None, None, None
        stack = [(12, riff_end)]
        while stack:
            p, hi = stack.pop()
            while p + 8 <= hi:
                f.seek(p)
                cid, n = struct.unpack("<4sI", f.read(8))
                if cid == b"LIST":
                    kind = f.read(4)
                    if kind == b"movi":
                        movi = (p + 8, min(p + 8 + n, size))
                    elif kind in (b"hdrl", b"strl"):
                        stack.append((p + 12, min(p + 8 + n, hi)))
                    elif kind == b"odml":
                        raise ValueError(f"MjpegReader: {self.path} is an OpenDML (AVI 2.0) file, which is not read")
                elif cid == b"avih":
                    h = f.read(min(n, 56))
                    if len(h) < 56:
                        raise ValueError(f"MjpegReader: {self.path} is damaged: its avih chunk holds {len(h)} bytes, not 56")
                    a = struct.unpack("<14I", h)
                    self.width, self.height = a[8], a[9]
                    if a[0]:
                        self.fps = 1e6 / a[0]
                elif cid == b"strh" and handler is None:
                    h = f.read(min(n, 56))
                    if len(h) < 28:
                        raise ValueError(f"MjpegReader: {self.path} is damaged: its strh chunk holds {len(h)} bytes, not 56")
                    stream_type, handler = h[:4], h[4:8]
                    scale, rate = struct.unpack("<II", h[20:28])
                    if scale and rate:
                        self.fps = rate / scale
                elif cid == b"indx":
                    raise ValueError(f"MjpegReader: {self.path} is an OpenDML (AVI 2.0) file, which is not read")
                elif cid == b"idx1":
                    idx = (p + 8, n)
                p += 8 + n + (n & 1)
        if riff_end + 12 <= size:
            f.seek(riff_end)
            if f.read(4) == b"RIFF" and f.read(8)[4:] == b"AVIX":
                raise ValueError(f"MjpegReader: {self.path} is an OpenDML (AVI 2.0) file, which is not read")
        if stream_type != b"vids" or handler not in (b"MJPG", b"mjpg"):
            raise ValueError(f"MjpegReader: the stream of {self.path} has handler {handler!r}, not MJPG: only Motion-JPEG AVI is "
                             "read - extract the frames to a folder and pass the folder")
        if movi is None:
            raise ValueError(f"MjpegReader: {self.path} has no movi list")
        self._frames = []              # (file offset of the payload, size)
        if idx is not None:
            f.seek(idx[0])
            raw = f.read(idx[1])
            ent = np.frombuffer(raw[:len(raw) - len(raw) % 16], "<u4").reshape(-1, 4)
            vid = ent[(ent[:, 0] == 0x63643030) | (ent[:, 0] == 0x62643030)]          # '00dc' | '00db'
            if vid.size:
                # offsets count from the movi fourcc, in some writers from the start of the file: the first entry tells which
                f.seek(movi[0] + int(vid[0, 2]))
                base = movi[0] if f.read(4) in (b"00dc", b"00db") else 0
                self._frames = [(base + int(o) + 8, int(s)) for o, s in zip(vid[:, 2], vid[:, 3]) if s > 0]
        if not self._frames:
            p = movi[0] + 4
            while p + 8 <= movi[1]:
                f.seek(p)
                cid, n = struct.unpack("<4sI", f.read(8))
                if cid == b"LIST":     # 'rec ' groups
                    p += 12
                    continue
                if cid in (b"00dc", b"00db") and n > 0:
                    self._frames.append((p + 8, n))
                p += 8 + n + (n & 1)
        if any(o + s > size for o, s in self._frames):
            raise ValueError(f"MjpegReader: {self.path} is cut short: a frame lies past the end of the file")

    def __len__(self) -> int:
        return len(self._frames)

    def __getitem__(self, i: int) -> bytes:
        off, n = self._frames[range(len(self._frames))[i]]
        self._f.seek(off)
        return self._f.read(n)

    def __iter__(self):
        for i in range(len(self._frames)):
            yield self[i]

    def close(self) -> None:
        if self._f is not None:
            self._f.close()
            self._f = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
