"""TEST-ONLY torch emulation of ``ops.resample_u8`` on the CPU, beside ``cpu_track_emulation``: the passes ``ops.resample_passes`` plans
(the library's own tables: building them touches no GPU), each one gather and one integer sum over the taps, so that the runner tests stay
quick; ``test_resample_host`` holds it against the spec bit for bit.  Never importable from the product."""
from __future__ import annotations

import torch


def _one_pass(x, dim, table):
    """x: uint8 [F, H, W, C]; resamples ``dim`` (1 or 2) by ``table = (ksize, bounds [out, 2], coeffs [out, ksize])``."""
    ksize, bounds, coeffs = table
    idx = (bounds[:, :1].long() + torch.arange(ksize)[None, :]).clamp(max=x.shape[dim] - 1)       # [out, ksize]; past n the coefficient is 0
    xi = x.movedim(dim, -1).to(torch.int64)                                                       # [..., in]
    acc = (xi[..., idx] * coeffs.to(torch.int64)).sum(dim=-1) + (1 << 21)                         # [..., out]
    return (acc >> 22).clamp(0, 255).to(torch.uint8).movedim(-1, dim).contiguous()


def resample_u8(frames, size, resample="lanczos", box=None, window=None):
    from anyv2v_amd import ops
    if not (isinstance(frames, torch.Tensor) and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[0] >= 1
            and frames.shape[3] in (1, 3)):
        raise ValueError("resample_u8: a contiguous uint8 [F, H, W, C] tensor with C = 1 or 3 expected")
    (wx, wy, ww, wh), row0, rows, h, v = ops.resample_passes(int(frames.shape[1]), int(frames.shape[2]), size, resample, box, window)
    x = frames[:, row0:row0 + rows]
    x = x[:, :, wx:wx + ww].clone() if h is None else _one_pass(x, 2, h)
    return x if v is None else _one_pass(x, 1, v)


def install(monkeypatch=None):
    """``cpu_track_emulation.install`` plus ``ops.resample_u8`` (tests only)."""
    import cpu_track_emulation as temu
    from anyv2v_amd import ops
    temu.install(monkeypatch)
    if monkeypatch is not None:
        monkeypatch.setattr(ops, "resample_u8", resample_u8, raising=False)
    else:
        ops.resample_u8 = resample_u8
