"""TEST-ONLY torch emulation of the two masked-edit ops (``ops.latent_mask``, ``ops.masked_blend``) on the CPU, beside
``cpu_sampler_emulation``: fp16 storage, fp32 arithmetic where torch has the operation (the window maximum, the feather's two passes),
fp64 where fp32 torch cannot restate the kernel (the exact 64-value sum of the pool, the fused multiply-add of the blend).  Never
importable from the product."""
from __future__ import annotations

import torch
import torch.nn.functional as Fn


def latent_mask(mask, grow=0, sigma=0.0, out=None):
    from anyv2v_amd import ops
    assert mask.dim() == 3 and mask.dtype == torch.float16
    Fm, H, W = mask.shape
    h, w = H // 8, W // 8
    m = (mask.double().clamp(0, 1).view(Fm, h, 8, w, 8).sum(dim=(2, 4)) / 64.0).float()   # exact sum, one rounding to fp32
    if grow > 0:
        m = Fn.max_pool2d(m[None], 2 * grow + 1, stride=1, padding=grow)[0]                # (pads with -inf: outside is ignored)
    taps = torch.tensor(ops.gaussian_taps(sigma), dtype=torch.float32)
    R = taps.numel() // 2
    if R > 0:
        xs = (torch.arange(w)[:, None] + torch.arange(-R, R + 1)[None, :]).clamp(0, w - 1)
        ys = (torch.arange(h)[:, None] + torch.arange(-R, R + 1)[None, :]).clamp(0, h - 1)
        m = (m[:, :, xs] * taps).sum(dim=-1)
        m = (m[:, ys, :] * taps[None, None, :, None]).sum(dim=2)
    res = m.half()
    if out is not None:
        out.copy_(res)
        return out
    return res


def masked_blend(x, src, mask, out=None):
    assert x.dtype == src.dtype == mask.dtype == torch.float16 and x.shape == src.shape and mask.shape[0] in (1, x.shape[2])
    mm = mask[None, None].expand(x.shape)
    d = (x.float() - src.float())
    y = (mm.double() * d.double() + src.double()).float().half()
    res = torch.where(mm == 0, src, torch.where(mm == 1, x, y))
    if out is None:
        return res
    out.copy_(res)
    return out


def install(monkeypatch=None):
    """``cpu_sampler_emulation.install`` plus the two masked-edit ops (tests only)."""
    import cpu_sampler_emulation as semu
    from anyv2v_amd import ops
    semu.install(monkeypatch)
    for name, fn in (("latent_mask", latent_mask), ("masked_blend", masked_blend)):
        if monkeypatch is not None:
            monkeypatch.setattr(ops, name, fn, raising=False)
        else:
            setattr(ops, name, fn)
