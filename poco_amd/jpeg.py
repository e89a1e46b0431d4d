"""Rendered frames as baseline JPEG, encoded on the GPU where they are (a binding of poco_jpeg_* in include/poco_hip.h,
csrc/jpeg_enc.hip), and a Motion-JPEG .avi writer on top of it: the result video the reference makes with ffmpeg
(demo.py:148-157, demo_utils.py:237-245 images_to_video, -pix_fmt yuv420p) without shelling out.

    enc = JpegEncoder(device, 1080, 1920)
    data = enc.encode(frame_u8_cuda, quality=90)          # bytes of a .jpg file: a few hundred KB cross PCIe instead of 6 MB
    with MjpegWriter("out.avi", 1920, 1080, fps=30) as w:
        w.add(data)
"""
from __future__ import annotations

import ctypes as C
import struct

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
