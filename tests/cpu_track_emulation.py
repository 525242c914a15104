"""TEST-ONLY torch emulation of the five tracking ops (``ops.luma_u8``, ``ops.block_match``, ``ops.flow_median``, ``ops.mask_propagate``,
``ops.first_frame_mask``) on the CPU, beside ``cpu_composite_emulation``: each function restates the contract of ``include/anyv2v_hip.h``
in integers, vectorised where ``track_spec`` loops (a row of displacements at a time, the winner by the minimum of a packed key, the chain
walked per pixel) so that the runner tests stay quick; ``test_track_host`` holds it against the spec bit for bit.  Never importable from
the product."""
from __future__ import annotations

import torch
import torch.nn.functional as Fn


def luma_u8(frames):
    assert frames.dtype == torch.uint8 and frames.dim() == 4 and frames.shape[-1] == 3
    f = frames.to(torch.int32)
    return ((77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8).to(torch.uint8)


def block_match(luma, radius=16):
    from anyv2v_amd import _lib
    assert luma.dtype == torch.uint8 and luma.dim() == 3 and luma.shape[1] % 8 == 0 and luma.shape[2] % 8 == 0
    if isinstance(radius, bool) or not 0 <= radius <= _lib.TRACK_MAX_RADIUS or int(radius) != radius:
        raise ValueError(f"radius={radius}: an integer, 0 <= radius <= {_lib.TRACK_MAX_RADIUS} pixels")
    F, H, W = luma.shape
    R = int(radius)
    flow = torch.zeros(F, H // 8, W // 8, 2, dtype=torch.int16)
    pad = Fn.pad(luma[:, None].float(), (R + 4,) * 4, mode="replicate")[:, 0].to(torch.int64)      # [F, H + 8 + 2 R, W + 8 + 2 R]
    dxs = torch.arange(-R, R + 1)
    for k in range(1, F):
        cur = pad[k, R: R + H + 8, R: R + W + 8]
        best = None
        for dy in range(-R, R + 1):
            prev = pad[k - 1, R + dy: R + dy + H + 8].unfold(1, W + 8, 1)                             # [H + 8, 2 R + 1, W + 8]
            cost = (cur[:, None, :] - prev).abs().unfold(0, 16, 8).sum(-1).unfold(2, 16, 8).sum(-1)   # [h, 2 R + 1, w]
            key = (cost << 26) | ((dy * dy + dxs * dxs) << 14)[None, :, None] | ((dy + 32) << 7) | (dxs + 32)[None, :, None]
            key = key.amin(dim=1)
            best = key if best is None else torch.minimum(best, key)
        flow[k, ..., 0], flow[k, ..., 1] = (((best >> 7) & 127) - 32).to(torch.int16), ((best & 127) - 32).to(torch.int16)
    return flow


def flow_median(flow):
    assert flow.dtype == torch.int16 and flow.dim() == 4 and flow.shape[3] == 2
    F, h, w, _ = flow.shape
    p = Fn.pad(flow.permute(0, 3, 1, 2).float(), (1, 1, 1, 1), mode="replicate")
    nine = p.unfold(2, 3, 1).unfold(3, 3, 1).reshape(F, 2, h, w, 9)
    return nine.sort(dim=-1).values[..., 4].permute(0, 2, 3, 1).to(torch.int16).contiguous()


def mask_propagate(mask0, flow):
    assert flow.dtype == torch.int16 and flow.dim() == 4 and mask0.dtype in (torch.bool, torch.uint8)
    F, h, w, _ = flow.shape
    H, W = 8 * h, 8 * w
    assert tuple(mask0.shape) == (H, W)
    k = torch.arange(F)[:, None, None]
    qy = torch.arange(H)[None, :, None].expand(F, H, W).clone()
    qx = torch.arange(W)[None, None, :].expand(F, H, W).clone()
    for j in range(F - 1, 0, -1):                                   # frame k takes the steps j = k .. 1
        d = flow[j].to(torch.int64)[qy // 8, qx // 8]
        go = k >= j
        qy = torch.where(go, (qy + d[..., 0]).clamp(0, H - 1), qy)
        qx = torch.where(go, (qx + d[..., 1]).clamp(0, W - 1), qx)
    return (mask0 != 0)[qy, qx]


def first_frame_mask(source, edited, threshold=24, min_count=8):
    assert source.dtype == torch.uint8 and edited.dtype == torch.uint8 and source.dim() == 3 and source.shape == edited.shape
    if isinstance(threshold, bool) or not 0 <= threshold <= 255 or int(threshold) != threshold:
        raise ValueError(f"threshold={threshold}: an integer, 0 <= threshold <= 255")
    if isinstance(min_count, bool) or not 1 <= min_count <= 64 or int(min_count) != min_count:
        raise ValueError(f"min_count={min_count}: an integer, 1 <= min_count <= 64")
    changed = (edited.to(torch.int16) - source.to(torch.int16)).abs().amax(dim=-1) > threshold
    count = Fn.avg_pool2d(changed[None, None].float(), 8, divisor_override=1)[0, 0]
    return (count >= min_count).repeat_interleave(8, dim=0).repeat_interleave(8, dim=1)[None]


def install(monkeypatch=None):
    """``cpu_composite_emulation.install`` plus the five tracking ops (tests only)."""
    import cpu_composite_emulation as cemu
    from anyv2v_amd import ops
    cemu.install(monkeypatch)
    for name, fn in (("luma_u8", luma_u8), ("block_match", block_match), ("flow_median", flow_median), ("mask_propagate", mask_propagate),
                     ("first_frame_mask", first_frame_mask)):
        if monkeypatch is not None:
            monkeypatch.setattr(ops, name, fn, raising=False)
        else:
            setattr(ops, name, fn)
