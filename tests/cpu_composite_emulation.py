"""TEST-ONLY torch emulation of the three composite ops (``ops.pixel_alpha``, ``ops.composite_stats``, ``ops.composite``) on the CPU, beside
``cpu_masked_edit_emulation``: each function restates the contract of ``include/anyv2v_hip.h`` -- the support and the two dilations exactly,
the feather's two passes in fp32 (a product and a sum where the kernel has one fmaf: the last bit may differ), the statistics as exact
integer sums in ONE record (the kernel spreads them over its blocks; only the fold is defined), the paste through fp64 where fp32 torch has
no fused multiply-add.  Never importable from the product."""
from __future__ import annotations

import torch
import torch.nn.functional as Fn


def _levels(video):
    return torch.nan_to_num(((video + 1.0) * 127.5).round().clamp(0, 255).float(), nan=0.0)


def pixel_alpha(latent_mask, grow_px=0, feather_px=0.0, out=None):
    from anyv2v_amd import _lib, ops
    assert latent_mask.dim() == 3 and latent_mask.dtype == torch.float16
    if isinstance(grow_px, bool) or not 0 <= grow_px <= _lib.COMPOSITE_MAX_GROW or int(grow_px) != grow_px:
        raise ValueError(f"grow_px={grow_px}: an integer, 0 <= grow_px <= {_lib.COMPOSITE_MAX_GROW} pixels")
    taps = torch.tensor(ops.gaussian_taps(feather_px, _lib.COMPOSITE_MAX_RADIUS, "feather_px", "pixels"), dtype=torch.float32)
    R, g = taps.numel() // 2, int(grow_px)
    base = (latent_mask > 0).repeat_interleave(8, dim=1).repeat_interleave(8, dim=2).float()
    grown = lambda r: base if r == 0 else Fn.max_pool2d(base[None], 2 * r + 1, stride=1, padding=r)[0]
    core, a = grown(g) > 0, grown(g + R)
    if R > 0:
        H, W = a.shape[1:]
        xs = (torch.arange(W)[:, None] + torch.arange(-R, R + 1)[None, :]).clamp(0, W - 1)
        ys = (torch.arange(H)[:, None] + torch.arange(-R, R + 1)[None, :]).clamp(0, H - 1)
        rows = torch.zeros_like(a)
        for k in range(2 * R + 1):
            rows = rows + taps[k] * a[:, :, xs[:, k]]
        a = torch.zeros_like(rows)
        for k in range(2 * R + 1):
            a = a + taps[k] * rows[:, ys[:, k], :]
    res = torch.where(core, torch.ones_like(a), a.clamp(max=1.0))
    if out is not None:
        out.copy_(res)
        return out
    return res


def composite_stats(video, source_u8, alpha, out=None):
    from anyv2v_amd import _lib
    _, C_, F, H, W = video.shape
    assert video.dtype == torch.float16 and C_ == 3 and source_u8.dtype == torch.uint8 and tuple(source_u8.shape) == (F, H, W, 3)
    assert alpha.dtype == torch.float32 and alpha.shape[0] in (1, F) and tuple(alpha.shape[1:]) == (H, W)
    e = _levels(video)[0].permute(1, 2, 3, 0).long()
    s = source_u8.long()
    kept = (alpha.expand(F, H, W) == 0)[..., None].expand_as(e).long()
    rec = torch.zeros(_lib.COMPOSITE_STATS_BLOCKS, _lib.COMPOSITE_STATS_RECORD, dtype=torch.int64)
    cols = [kept, kept * e, kept * e * e, kept * s, kept * s * s]
    rec[0, :15] = torch.stack([c.sum(dim=(0, 1, 2)) for c in cols], dim=1).reshape(-1)
    if out is not None:
        out.copy_(rec)
        return out
    return rec


def composite(video, source_u8, alpha, match_color=False, out=None):
    _, C_, F, H, W = video.shape
    rec = composite_stats(video, source_u8, alpha) if match_color else None
    a = alpha.expand(F, H, W)[..., None]
    e = _levels(video)[0].permute(1, 2, 3, 0)
    s = source_u8.float()
    if rec is not None:
        q = rec.sum(dim=0)[:15].view(3, 5).double()
        gain, bias = torch.ones(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
        for c in range(3):
            n = q[c, 0]
            if n < 64:
                continue
            me, ms = q[c, 1] / n, q[c, 3] / n
            ve, vs = (q[c, 2] / n - me * me).clamp(min=0), (q[c, 4] / n - ms * ms).clamp(min=0)
            if ve > 0:
                gain[c] = (vs.sqrt() / ve.sqrt()).clamp(0.5, 2.0)
                bias[c] = ms - gain[c] * me
        e = (gain.float().double() * e.double() + bias.float().double()).float().clamp(0, 255)      # one fp32 rounding: the fmaf
    y = (a.double() * (e - s).double() + s.double()).float().round().clamp(0, 255)
    res = torch.where(a == 0, s, torch.where(a == 1, e.round(), y)).to(torch.uint8)
    if out is not None:
        out.copy_(res)
        return out
    return res


def install(monkeypatch=None):
    """``cpu_auto_mask_emulation.install`` plus the three composite ops (tests only)."""
    import cpu_auto_mask_emulation as aemu
    from anyv2v_amd import ops
    aemu.install(monkeypatch)
    for name, fn in (("pixel_alpha", pixel_alpha), ("composite_stats", composite_stats), ("composite", composite)):
        if monkeypatch is not None:
            monkeypatch.setattr(ops, name, fn, raising=False)
        else:
            setattr(ops, name, fn)
