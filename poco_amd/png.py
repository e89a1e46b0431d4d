"""Rendered frames as PNG, filtered and deflated on the GPU where they are (a binding of poco_png_* in include/poco_hip.h,
csrc/png_enc.hip): the lossless pictures the reference writes with cv2.imwrite (pocolib/core/tester.py:350, :572) without the
frame crossing to the host.

    enc = PngEncoder(device, 1080, 1920)
    data = enc.encode(frame_u8_cuda)          # bytes of a .png file: PIL reads back exactly the frame

The bytes are a function of the frame alone (tests/png_np.py restates them in numpy); they are not the bytes PIL or libpng
would write for the same pixels."""
from __future__ import annotations

import ctypes as C

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
