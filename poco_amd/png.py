"""Rendered frames as PNG, filtered and deflated on the GPU where they are (a binding of poco_png_* in include/poco_hip.h,
csrc/png_enc.hip): the lossless pictures the reference writes with cv2.imwrite (pocolib/core/tester.py:350, :572) without the
frame crossing to the host.

    enc = PngEncoder(device, 1080, 1920)
    data = enc.encode(frame_u8_cuda)          # bytes of a .png file: PIL reads back exactly the frame

The bytes are a function of the frame alone (tests/png_np.py restates them in numpy); they are not the bytes PIL or libpng
would write for the same pixels.

The way back is here too: parse_png walks a file's chunks on the host and checks their CRCs, PngDecoder hands the IDAT payloads
of a whole batch to the device decoder (poco_png_decode, csrc/png_dec.hip: inflate and unfilter).

    dec = PngDecoder(device, 1080, 1920, max_batch=16)
    frames = dec.decode([open(p, "rb").read() for p in paths])       # uint8 [H,W,3] device tensors, PIL's pixels
"""
from __future__ import annotations

import ctypes as C
import struct
import zlib
from dataclasses import dataclass
from typing import List, Optional, Tuple

import numpy as np
import torch

from ._lib import PocoHipError, check, lib

MAX_SIDE = 16384
SEGMENT = 32768


def worst_case_bytes(H: int, W: int) -> int:
    """The out_cap poco_png_encode asks for: signature, IHDR, IEND, zlib header and Adler-32 (51 bytes), the filtered stream
    S = H (1 + 3W), and per segment of 32 768 bytes 10 bytes of block framing + 12 of its IDAT chunk."""
    S = H * (1 + 3 * W)
    return 51 + S + 22 * (-(-S // SEGMENT))


class PngEncoder:
    """PNG (8-bit RGB, no interlace) of uint8 [H,W,3] device frames up to max_h x max_w.  All scratch is planned here; encode /
    encode_into allocate nothing on the C side."""

    def __init__(self, device, max_h: int, max_w: int):
        max_h, max_w = int(max_h), int(max_w)
        if not (1 <= max_h <= MAX_SIDE and 1 <= max_w <= MAX_SIDE):
            raise PocoHipError(f"PngEncoder: max_h, max_w must be in 1..{MAX_SIDE}, got {max_h} x {max_w}")
        self.max_h, self.max_w = max_h, max_w
        self._h = C.c_void_p()
        self._out = None
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        L = lib()
        L.poco_png_encoder_create.argtypes = [C.c_int, C.c_int, C.POINTER(C.c_void_p)]
        L.poco_png_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
        L.poco_png_encoder_destroy.argtypes = [C.c_void_p]
        L.poco_png_encoder_destroy.restype = None
        with torch.cuda.device(self.device):
            check(L.poco_png_encoder_create(max_h, max_w, C.byref(self._h)), "poco_png_encoder_create")

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().poco_png_encoder_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def encode_into(self, frame: torch.Tensor, out: torch.Tensor, length: torch.Tensor = None):
        """Enqueue the encode of `frame` (contiguous uint8 [H,W,3] on the device) into `out` (uint8, at least
        worst_case_bytes(H, W) long) on the current stream; returns (out, length) with `length` an int32 [1] device tensor
        holding the number of bytes.  No host synchronisation."""
        if not (torch.is_tensor(frame) and frame.device.type == "cuda" and frame.dtype == torch.uint8 and frame.dim() == 3
                and frame.shape[2] == 3 and frame.is_contiguous()):
            raise PocoHipError("PngEncoder: frame must be a contiguous uint8 [H,W,3] device tensor")
        if not (torch.is_tensor(out) and out.device == frame.device and out.dtype == torch.uint8 and out.is_contiguous()):
            raise PocoHipError("PngEncoder: out must be a contiguous uint8 tensor on the frame's device")
        if length is None:
            length = torch.empty(1, dtype=torch.int32, device=frame.device)
        elif not (torch.is_tensor(length) and length.device == frame.device and length.dtype == torch.int32 and length.numel() >= 1):
            raise PocoHipError("PngEncoder: length must be an int32 tensor on the frame's device")
        check(lib().poco_png_encode(self._h, frame.data_ptr(), int(frame.shape[0]), int(frame.shape[1]), out.data_ptr(), out.numel(),
                                    length.data_ptr(), C.c_void_p(torch.cuda.current_stream(frame.device).cuda_stream)),
              "poco_png_encode")
        return out, length

    def encode(self, frame: torch.Tensor) -> bytes:
        """The bytes of the .png file of `frame`: the length and exactly that many bytes are copied to the host."""
        if self._out is None:
            self._out = torch.empty(worst_case_bytes(self.max_h, self.max_w), dtype=torch.uint8, device=self.device)
        out, length = self.encode_into(frame, self._out)
        return out[:int(length.item())].cpu().numpy().tobytes()


# ---- decoding: the chunk walk and the device decoder's binding --------------------------------------------------------------------
SIGNATURE = b"\x89PNG\r\n\x1a\n"
BPP = {0: 1, 2: 3, 3: 1, 4: 2, 6: 4}   # bytes per pixel by colour type, bit depth 8


@dataclass
class PngInfo:
    """What parse_png found."""
    height: int
    width: int
    colour_type: int                   # 0 grey, 2 RGB, 3 palette, 4 grey + alpha, 6 RGBA
    bpp: int
    palette: bytes                     # 256 x 3 bytes, padded with zeros
    idat: List[Tuple[int, int]]        # (offset, length) of every IDAT payload in data
    stream_length: int                 # the deflate stream: the payloads without the 2-byte zlib header and the 4-byte Adler-32
    data: bytes


def _parse(data: bytes) -> Optional[PngInfo]:
    n = len(data)
    if n < 8 or data[:8] != SIGNATURE:
        return None
    i, first = 8, True
    ihdr, palette, idat, idat_closed, seen_end = None, None, [], False, False
    while i < n:
        if i + 12 > n:
            return None
        ln, typ = struct.unpack(">I4s", data[i:i + 8])
        if i + 12 + ln > n:
            return None
        body = i + 8
        if first != (typ == b"IHDR"):
            return None
        first = False
        if typ in (b"IHDR", b"PLTE", b"IDAT", b"IEND"):
            if zlib.crc32(data[i + 4:body + ln]) != struct.unpack(">I", data[body + ln:body + ln + 4])[0]:
                return None
        if typ == b"IHDR":
            if ln != 13:
                return None
            W, H, depth, ctype, comp, filt, lace = struct.unpack(">IIBBBBB", data[body:body + 13])
            if depth != 8 or ctype not in BPP or comp != 0 or filt != 0 or lace != 0:
                return None
            if not (1 <= H <= MAX_SIDE and 1 <= W <= MAX_SIDE):
                return None
            ihdr = (H, W, ctype)
        elif typ == b"PLTE":
            if palette is not None or idat or ln % 3 or not 3 <= ln <= 768:
                return None
            palette = data[body:body + ln] + bytes(768 - ln)
        elif typ == b"IDAT":
            if idat_closed:
                return None            # IDAT chunks must be consecutive
            idat.append((body, ln))
        elif typ == b"acTL":
            return None                # APNG
        elif typ == b"IEND":
            seen_end = True
            break
        if idat and typ != b"IDAT":
            idat_closed = True
        i = body + ln + 4
    if ihdr is None or not seen_end or not idat:
        return None
    H, W, ctype = ihdr
    if ctype == 3 and palette is None:
        return None
    total = sum(l for _, l in idat)
    if total < 6:
        return None
    head = b""
    for o, l in idat:                  # the zlib header may straddle chunks
        head += data[o:o + min(l, 2 - len(head))]
        if len(head) == 2:
            break
    cmf, flg = head[0], head[1]
    if cmf & 15 != 8 or cmf >> 4 > 7 or (cmf * 256 + flg) % 31 or flg & 0x20:
        return None
    return PngInfo(H, W, ctype, BPP[ctype], palette if palette is not None else bytes(768), idat, total - 6, data)


def parse_png(data) -> Optional[PngInfo]:
    """The chunk walk of one .png file: sizes, colour type, palette and the list of IDAT payloads - or None for a file the
    device decoder does not take (16-bit, depths below 8, Adam7, APNG, a bad CRC in IHDR / PLTE / IDAT / IEND, a bad zlib header,
    fewer than 6 payload bytes, a file cut short); the caller then decodes with PIL.  Ancillary chunks are skipped: they do not
    change what Image.open(f).convert("RGB") returns.  Never raises on file content."""
    try:
        return _parse(bytes(data))
    except (IndexError, ValueError, struct.error):
        return None


class _CPngImage(C.Structure):
    _fields_ = [("data", C.c_void_p), ("nbytes", C.c_size_t), ("idat", C.c_void_p), ("nidat", C.c_int), ("H", C.c_int),
                ("W", C.c_int), ("colour_type", C.c_int), ("palette", C.c_uint8 * 768), ("d_rgb", C.c_void_p)]


class PngDecoder:
    """PNG files -> uint8 [H,W,3] RGB device tensors holding the pixels PIL gives, up to max_batch images of up to max_h x max_w
    and max_bytes of deflate stream per call, of mixed sizes and colour types.  Device scratch and the pinned staging buffer are
    planned here; decode / decode_into allocate nothing on the C side."""

    def __init__(self, device, max_h: int, max_w: int, max_batch: int = 1, max_bytes: int = 0):
        max_h, max_w, max_batch = int(max_h), int(max_w), int(max_batch)
        max_bytes = int(max_bytes) or min(1 << 30, max_batch * max(1 << 16, 2 * max_h * max_w))
        if not (1 <= max_h <= MAX_SIDE and 1 <= max_w <= MAX_SIDE):
            raise PocoHipError(f"PngDecoder: max_h, max_w must be in 1..{MAX_SIDE}, got {max_h} x {max_w}")
        if not 1 <= max_batch <= 4096:
            raise PocoHipError(f"PngDecoder: max_batch must be in 1..4096, got {max_batch}")
        if not 1 <= max_bytes <= 1 << 30:
            raise PocoHipError(f"PngDecoder: max_bytes must be in 1..2^30, got {max_bytes}")
        self.max_h, self.max_w, self.max_batch, self.max_bytes = max_h, max_w, max_batch, max_bytes
        self._h = C.c_void_p()
        self.device = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        L = lib()
        L.poco_png_decoder_create.argtypes = [C.c_int, C.c_int, C.c_int, C.c_size_t, C.POINTER(C.c_void_p)]
        L.poco_png_decode.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        L.poco_png_decoder_destroy.argtypes = [C.c_void_p]
        L.poco_png_decoder_destroy.restype = None
        with torch.cuda.device(self.device):
            check(L.poco_png_decoder_create(max_h, max_w, max_batch, max_bytes, C.byref(self._h)), "poco_png_decoder_create")

    def close(self) -> None:
        if getattr(self, "_h", None):
            lib().poco_png_decoder_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def decode_into(self, images, outs, status: torch.Tensor = None) -> torch.Tensor:
        """Enqueue the decode of `images` (bytes of .png files or PngInfo, at most max_batch) into `outs` (contiguous uint8
        [H,W,3] device tensors of the files' sizes) on the current stream: one host-to-device copy, no host synchronisation.
        Returns `status`, an int32 [n] device tensor: 0 per decoded image, non-zero for a damaged stream."""
        infos = []
        for im in images:
            info = im if isinstance(im, PngInfo) else parse_png(im)
            if info is None:
                raise PocoHipError("PngDecoder: not a PNG file this decoder takes (parse_png returned None)")
            infos.append(info)
        n = len(infos)
        if not 1 <= n <= self.max_batch:
            raise PocoHipError(f"PngDecoder: {n} images in one call, the decoder was created for 1..{self.max_batch}")
        if len(outs) != n:
            raise PocoHipError(f"PngDecoder: {n} images but {len(outs)} output tensors")
        for info, o in zip(infos, outs):
            if not (torch.is_tensor(o) and o.device == self.device and o.dtype == torch.uint8 and o.is_contiguous()
                    and tuple(o.shape) == (info.height, info.width, 3)):
                raise PocoHipError(f"PngDecoder: an output must be a contiguous uint8 [{info.height},{info.width},3] tensor on "
                                   f"{self.device}")
        if status is None:
            status = torch.empty(n, dtype=torch.int32, device=self.device)
        elif not (torch.is_tensor(status) and status.device == self.device and status.dtype == torch.int32
                  and status.is_contiguous() and status.numel() >= n):
            raise PocoHipError("PngDecoder: status must be a contiguous int32 tensor of at least n elements on the decoder's device")
        arr = (_CPngImage * n)()
        keep = []
        for s, info, o in zip(arr, infos, outs):
            buf = np.frombuffer(info.data, np.uint8)
            idat = np.ascontiguousarray(np.asarray(info.idat, np.uint32).reshape(-1, 2))
            keep += [buf, idat]
            s.data, s.nbytes = buf.ctypes.data, buf.size
            s.idat, s.nidat = idat.ctypes.data, idat.shape[0]
            s.H, s.W, s.colour_type = info.height, info.width, info.colour_type
            C.memmove(s.palette, bytes(info.palette[:768]).ljust(768, b"\0"), 768)
            s.d_rgb = o.data_ptr()
        check(lib().poco_png_decode(self._h, C.cast(arr, C.c_void_p), n, status.data_ptr(),
                                    C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "poco_png_decode")
        return status

    def decode(self, images, return_status: bool = False):
        """The pictures of `images` as new device tensors.  return_status: also the list of status words (this reads them back,
        the call's only host synchronisation)."""
        infos = [im if isinstance(im, PngInfo) else parse_png(im) for im in images]
        if any(i is None for i in infos):
            raise PocoHipError("PngDecoder: not a PNG file this decoder takes (parse_png returned None)")
        outs = [torch.empty(i.height, i.width, 3, dtype=torch.uint8, device=self.device) for i in infos]
        status = self.decode_into(infos, outs)
        return (outs, status.cpu().tolist()) if return_status else outs
