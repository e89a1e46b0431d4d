"""CPU: the entries whose launch puts a caller-sized count on gridDim.y without chunking it refuse a count above the 65 535 limit
before they launch, with a message that names the limit (DESIGN.md section 37 lists every such launch and the test that holds its
row; poco_op_part_visibility's refusal is in tests/test_visibility_cpu.py, the JPEG decoder's in tests/test_jpegdec_cpu.py).  No GPU:
the argument checks come first.  Also here: tester.crop_normalize refuses tensors that are not on a GPU."""
import ctypes as C

import numpy as np
import pytest
import torch

from poco_amd import _lib

FAKE, NULL = C.c_void_p(4096), C.c_void_p(0)


def msg():
    return _lib.lib().poco_last_error().decode()


def test_part_labels_refuses_more_than_65535_bodies():
    L = _lib.lib()
    f = C.c_float(5000.0)
    call = lambda B: L.poco_op_part_labels(FAKE, B, 10, FAKE, FAKE, 4, FAKE, f, 224, FAKE, FAKE, NULL)      # noqa: E731
    assert call(65536) == 1 and "part_labels" in msg() and "B <= 65535" in msg()
    assert call(1 << 30) == 1 and call(0) == 1


def test_segm_entries_refuse_more_than_65535_crops():
    L = _lib.lib()
    score = lambda B: L.poco_op_segm_score(FAKE, B, 25, 56, 56, FAKE, 224, 224, FAKE, FAKE, NULL)            # noqa: E731
    assert score(65536) == 1 and "segm_score" in msg() and "B <= 65535" in msg()
    argmax = lambda B: L.poco_op_segm_argmax(FAKE, B, 25, 56, 56, 224, 224, FAKE, NULL)                      # noqa: E731
    assert argmax(65536) == 1 and "segm_argmax" in msg() and "B <= 65535" in msg()
    assert score(0) == 1 and argmax(0) == 1


def test_engine_refuses_a_max_batch_above_65535():
    """smpl_skin_kernel runs one block row per 64 crops on gridDim.y; the engine's batch is capped where the operators' is."""
    L = _lib.lib()
    L.poco_create.argtypes = [C.c_char_p, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
    h = C.c_void_p()
    for mb in (65536, 1 << 30):
        assert L.poco_create(b"resnet50-cliff", mb, 6, C.byref(h)) == 1 and "max_batch must be in 1..65535" in msg(), mb
        assert not h.value
    assert L.poco_create(b"resnet50-cliff", 0, 6, C.byref(h)) == 1 and not h.value


def test_crop_normalize_refuses_cpu_tensors():
    from poco_amd.tester import crop_normalize
    frame = torch.zeros(8, 8, 3, dtype=torch.uint8)
    boxes = torch.tensor([[4.0, 4.0, 6.0, 6.0]])
    with pytest.raises(ValueError, match="crop_normalize: the frame"):
        crop_normalize(frame, boxes)
    with pytest.raises(ValueError, match="crop_normalize"):
        crop_normalize(np.zeros((8, 8, 3), np.uint8), boxes)
