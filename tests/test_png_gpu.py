"""GPU: the PNG encoder (csrc/png_enc.hip) against its numpy restatement (tests/png_np.py) BYTE for byte on the fixture set whose
coverage tests/test_png_cpu.py asserts, on a rendered frame, its guard bands, scratch reuse and determinism."""
import functools
import io

import numpy as np
import pytest
import torch
from PIL import Image

from poco_amd import png, render
from poco_amd._lib import lib
from tests import png_np, render_np

pytestmark = pytest.mark.gpu

POISON = 0xA5


@functools.lru_cache(maxsize=None)
def _fixtures():
    return {name: (img, png_np.encode(img)) for name, img in png_np.fixture_set()}


def _first_difference(a: bytes, b: bytes):
    n = min(len(a), len(b))
    d = np.nonzero(np.frombuffer(a[:n], np.uint8) != np.frombuffer(b[:n], np.uint8))[0]
    return (len(a), len(b), int(d[0]) if d.size else None)


@pytest.mark.parametrize("name", [n for n, _ in png_np.fixture_set()])
def test_bytes_equal_the_restatement(cuda, name):
    img, ref = _fixtures()[name]
    H, W = img.shape[:2]
    got = png.PngEncoder(cuda, H, W).encode(torch.from_numpy(img).to(cuda))
    assert got == ref, (name, _first_difference(got, ref))
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(got)).convert("RGB")), img)


def test_rendered_frame(cuda):
    """The procedural mesh of tests/render_np.py drawn over a seeded background at 120 x 168, encoded from the device frame."""
    H, W = 120, 168
    r = np.random.default_rng(12)
    verts, faces = render_np.deformed_sphere(3, subdiv=3, radius=0.5)
    frame = torch.from_numpy(png_np.photo_like(H, W, seed=12)).to(cuda)
    before = frame.clone()
    R = render.Renderer(faces, verts.shape[0], cuda)
    R.render(frame, torch.from_numpy(verts[None]).to(cuda), [[1.2 * H / W, 1.2, 0.0, 0.0]],
             [render.vertex_color(np.full(24, 0.3, np.float32), "hrnet_w48_cls-cliff")], [render.MATERIAL_UNCERT])
    assert (frame != before).any(), "nothing was drawn"
    got = png.PngEncoder(cuda, H, W).encode(frame)
    host = frame.cpu().numpy()
    ref = png_np.encode(host)
    assert got == ref, _first_difference(got, ref)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(got)).convert("RGB")), host)


def test_guard_band_and_length(cuda):
    """Nothing outside out[0, len) changes: the buffer is poisoned beyond the reported length and in a guard band in front."""
    guard = 64
    for name in ("noise_64x200", "special_24x700", "black_96x160"):          # stored blocks, dynamic blocks, next to nothing
        img, ref = _fixtures()[name]
        H, W = img.shape[:2]
        cap = png.worst_case_bytes(H, W)
        enc = png.PngEncoder(cuda, H, W)
        buf = torch.full((guard + cap + guard,), POISON, dtype=torch.uint8, device=cuda)
        out, n = enc.encode_into(torch.from_numpy(img).to(cuda), buf[guard:guard + cap])
        assert out.data_ptr() == buf.data_ptr() + guard and n.dtype == torch.int32 and n.is_cuda
        host, n = buf.cpu().numpy(), int(n.item())
        assert n == len(ref) and host[guard:guard + n].tobytes() == ref, name
        assert (host[:guard] == POISON).all() and (host[guard + n:] == POISON).all(), name


def test_encoder_reuse_smaller_then_larger(cuda):
    """One encoder codes a smaller and then a larger picture (and a small one again): the bytes of a fresh encoder each time, so
    no stale filtered row, slot, length or Adler sum leaks."""
    enc = png.PngEncoder(cuda, 129, 700)
    for name in ("special_3x7", "special_129x85", "special_24x700", "checker_96x160", "special_1x1"):
        img, ref = _fixtures()[name]
        got = enc.encode(torch.from_numpy(img).to(cuda))
        assert got == ref, (name, _first_difference(got, ref))


def test_two_encodes_are_bitwise_equal(cuda):
    img, ref = _fixtures()["photo_120x168"]
    enc = png.PngEncoder(cuda, 120, 168)
    frame = torch.from_numpy(img).to(cuda)
    a, b = enc.encode(frame), enc.encode(frame)
    assert a == b == ref


def test_argument_errors_leave_the_output_alone(cuda):
    H, W = 32, 48
    enc = png.PngEncoder(cuda, H, W)
    cap = png.worst_case_bytes(H, W)
    frame = torch.zeros(H, W, 3, dtype=torch.uint8, device=cuda)
    out = torch.full((cap,), POISON, dtype=torch.uint8, device=cuda)
    n = torch.full((1,), -7, dtype=torch.int32, device=cuda)
    L = lib()
    f, o, ln, h = frame.data_ptr(), out.data_ptr(), n.data_ptr(), enc._h
    bad = [(h, f, 0, W, o, cap, ln), (h, f, H, 0, o, cap, ln), (h, f, H + 1, W, o, cap, ln), (h, f, H, W + 1, o, cap, ln),
           (None, f, H, W, o, cap, ln), (h, None, H, W, o, cap, ln), (h, f, H, W, None, cap, ln), (h, f, H, W, o, cap, None),
           (h, f, H, W, o, cap - 1, ln)]
    for a in bad:
        assert L.poco_png_encode(*a, None) == 1, a
        assert L.poco_last_error().startswith(b"poco_png_encode")
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == POISON).all() and int(n.item()) == -7
    with pytest.raises(png.PocoHipError, match="uint8"):
        enc.encode(frame.float())
    assert enc.encode(frame) == png_np.encode(np.zeros((H, W, 3), np.uint8))          # the handle still works afterwards
