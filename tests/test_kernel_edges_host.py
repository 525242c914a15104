"""The frame helpers of tests/gpu_checks.py on the CPU: the guard check can fail, in each of its four bands."""
import pytest
import torch

import gpu_checks as gc


@pytest.mark.parametrize("dtype", [torch.float16, torch.float32])
def test_frame_reports_a_flip_in_each_band(dtype):
    M, C = 5, 12
    buf, view, frame = gc._framed(M, C, dtype, device="cpu")
    rows, cols = frame[0], frame[1]
    assert tuple(view.shape) == (M, C) and view.dtype == dtype and view.stride(1) == 1
    assert view.data_ptr() % 16 == 0 and view.stride(0) % 8 == 0          # what the fast paths test for
    assert torch.isnan(buf.view(dtype)).all()                             # the poison is a NaN, the window included until it is written
    view.copy_(torch.arange(M * C, dtype=torch.float32).view(M, C).to(dtype))
    assert gc._frame_intact(buf, frame)
    bands = {"above": (rows - 1, cols + 3), "below": (rows + M, cols + 3), "left": (rows + 2, cols - 1), "right": (rows + 2, cols + C)}
    for band, (r, c) in bands.items():
        old = int(buf[r, c])
        buf[r, c] = old ^ 1
        assert not gc._frame_intact(buf, frame), band
        buf[r, c] = old
        assert gc._frame_intact(buf, frame), band
    view[M - 1, C - 1] = 3.0                                              # writes inside the window are not the frame's business
    assert gc._frame_intact(buf, frame)


def test_framed_like_keeps_values_shape_and_contiguity():
    t2 = torch.randn(7, 13).half()
    buf, view, frame = gc._framed_like(t2)
    assert torch.equal(view, t2) and view.stride(0) % 8 == 0 and view.stride(0) > 13 and gc._frame_intact(buf, frame)
    for t in (torch.randn(11).half(), torch.randn(3, 5, 4), torch.randn(6, 64).half()):
        buf, view, frame = gc._framed_like(t, flat=True)
        assert torch.equal(view, t) and view.is_contiguous() and view.shape == t.shape and view.data_ptr() % 16 == 0
        flat = buf.view(t.dtype).reshape(-1)
        start = (view.data_ptr() - buf.data_ptr()) // t.element_size()
        assert torch.isnan(flat[start - 1]) and torch.isnan(flat[start + t.numel()])   # poison directly before and after
        buf[1, frame[1] - 1] ^= 1
        assert not gc._frame_intact(buf, frame)


def test_operand_factories_hand_out_same_shapes_and_alignment():
    t = torch.randn(9, 12).half()
    p = gc._ld8(t)
    assert torch.equal(p, t) and p.stride(0) == 16
    buf, view, frame = gc._framed(9, 12, torch.float16, cols=12, device="cpu", aligned=False)   # the deliberately misaligned C view
    assert view.data_ptr() % 16 == 8 and view.stride(0) % 8 == 0
