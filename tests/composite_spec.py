"""The pixel-space composite of a masked edit, as defined in ``include/anyv2v_hip.h``, in fp64 with torch on the CPU (TEST-ONLY):
``pixel_alpha`` (support, two square dilations, separable Gaussian with replicate padding, the selects), ``stats`` (exact integer sums over
the kept region), ``gain_bias`` and ``composite``.

The paste is exact: ``alpha (e - s) + s`` with a 24-bit alpha and 9-bit integers fits fp64 without rounding; rounded to fp32 and then by
``rint`` it is what an fp32 ``fmaf`` followed by ``rint`` yields, so the expected bytes are exact."""
from __future__ import annotations

import torch
import torch.nn.functional as Fn


def pil_bytes(video):
    """The bytes ``vae.to_pil`` forms from an fp16 tensor, any shape: ``((v + 1.0) * 127.5).round().clamp(0, 255)`` in fp16 arithmetic;
    NaN -> 0 (what the conversion to uint8 makes of it on the CPU), +Inf -> 255, -Inf -> 0."""
    assert video.dtype == torch.float16
    return torch.nan_to_num(((video + 1.0) * 127.5).round().clamp(0, 255).float(), nan=0.0).to(torch.uint8)


def dilate(b, r):
    """Square-window maximum of a bool [Fm, H, W], radius r, positions outside the image ignored."""
    if r == 0:
        return b.clone()
    return Fn.max_pool2d(b.double()[None], 2 * r + 1, stride=1, padding=r)[0] > 0     # (pads with -inf)


def pixel_alpha(lm, grow_px, taps):
    """fp16 latent mask [Fm, h, w], pixel grow, the 2 R + 1 fp32 taps (a list, [] for no feather) -> dict(alpha fp64 [Fm, 8 h, 8 w],
    core bool, reach bool: the support grown by grow_px + 2 R, beyond which alpha is exactly 0)."""
    assert lm.dtype == torch.float16 and lm.dim() == 3
    R = len(taps) // 2
    base = (lm > 0).repeat_interleave(8, dim=1).repeat_interleave(8, dim=2)
    core, wide = dilate(base, grow_px), dilate(base, grow_px + R)
    a = wide.double()
    if R > 0:
        t = torch.tensor(taps, dtype=torch.float32).double()
        H, W = a.shape[1:]
        xs = (torch.arange(W)[:, None] + torch.arange(-R, R + 1)[None, :]).clamp(0, W - 1)
        ys = (torch.arange(H)[:, None] + torch.arange(-R, R + 1)[None, :]).clamp(0, H - 1)
        a = (a[:, :, xs] * t).sum(dim=-1)                          # rows first
        a = (a[:, ys, :] * t[None, None, :, None]).sum(dim=2)      # then columns
    alpha = torch.where(core, torch.ones_like(a), a.clamp(max=1.0))
    return dict(alpha=alpha, core=core, reach=dilate(base, grow_px + 2 * R))


def _expand(alpha, F):
    assert alpha.shape[0] in (1, F)
    return alpha.expand(F, *alpha.shape[1:])


def stats(video, source, alpha):
    """-> int64 [3, 5]: per channel count, sum e, sum e^2, sum s, sum s^2 over the kept pixels (alpha == 0) of the whole clip."""
    _, C, F, H, W = video.shape
    e = pil_bytes(video)[0].permute(1, 2, 3, 0).long()             # [F, H, W, 3]
    s = source.long()
    kept = (_expand(alpha, F) == 0)[..., None].expand_as(e).long()
    return torch.stack([kept.sum(dim=(0, 1, 2)), (kept * e).sum(dim=(0, 1, 2)), (kept * e * e).sum(dim=(0, 1, 2)),
                        (kept * s).sum(dim=(0, 1, 2)), (kept * s * s).sum(dim=(0, 1, 2))], dim=1)


def gain_bias(st):
    """[3, 5] sums -> (gain, bias), each fp32 [3]: gain = clamp(std_s / std_e, 0.5, 2), bias = mean_s - gain mean_e in fp64, rounded to
    fp32; the identity when fewer than 64 kept pixels or a constant edit channel."""
    gain, bias = torch.ones(3, dtype=torch.float64), torch.zeros(3, dtype=torch.float64)
    for c in range(3):
        n, se, se2, ss, ss2 = (float(int(v)) for v in st[c])
        if int(st[c, 0]) < 64:
            continue
        me, ms = se / n, ss / n
        ve, vs = max(se2 / n - me * me, 0.0), max(ss2 / n - ms * ms, 0.0)
        if ve > 0.0:
            gain[c] = min(max(vs ** 0.5 / ve ** 0.5, 0.5), 2.0)
            bias[c] = ms - float(gain[c]) * me
    return gain.float(), bias.float()


def composite(video, source, alpha, match_color=False):
    """video fp16 [1, 3, F, H, W], source uint8 [F, H, W, 3], alpha fp32 (or fp64 holding fp32 values) [Fm, H, W] ->
    dict(out uint8 [F, H, W, 3], real fp64: the value before the final rint)."""
    _, C, F, H, W = video.shape
    assert C == 3 and source.dtype == torch.uint8 and tuple(source.shape) == (F, H, W, 3)
    a = _expand(alpha.float().double(), F)[..., None]
    e = pil_bytes(video)[0].permute(1, 2, 3, 0).double()
    s = source.double()
    if match_color:
        gain, bias = gain_bias(stats(video, source, alpha))
        e = (gain.double() * e + bias.double()).clamp(0, 255)
    real = torch.where(a == 0, s, torch.where(a == 1, e, a * (e - s) + s))
    rounded = real if match_color else torch.where((a == 0) | (a == 1), real, real.float().double())   # (the fp32 rounding of the fmaf)
    return dict(out=rounded.round().clamp(0, 255).to(torch.uint8), real=real)
