"""TEST-ONLY definition of the mask tracking (``anyv2v_amd/csrc/track.hip``), restated in plain integer torch from the text of
``include/anyv2v_hip.h`` -- frame after frame, displacement after displacement, the tie-break as the four comparisons of the tuple
``(cost, dy^2 + dx^2, dy, dx)``.  Not derived from the kernel: no tiles, no packed bytes, no key.  Everything is exact, so the kernels
are compared with ``torch.equal``.  Never importable from the product."""
from __future__ import annotations

import torch


def luma(frames):
    """uint8 [F, H, W, 3] -> uint8 [F, H, W]: Y = (77 R + 150 G + 29 B + 128) >> 8."""
    f = frames.to(torch.int64)
    return ((77 * f[..., 0] + 150 * f[..., 1] + 29 * f[..., 2] + 128) >> 8).to(torch.uint8)


def _clamped(plane, ys, xs):
    H, W = plane.shape
    return plane[ys.clamp(0, H - 1)[:, None], xs.clamp(0, W - 1)[None, :]]


def block_match(y, radius=16):
    """Luma uint8 [F, H, W] -> int16 [F, h, w, 2] (dy, dx); D_0 = 0."""
    F, H, W = y.shape
    assert H % 8 == 0 and W % 8 == 0 and F >= 1 and 0 <= radius <= 32
    h, w, R = H // 8, W // 8, int(radius)
    y = y.to(torch.int64)
    flow = torch.zeros(F, h, w, 2, dtype=torch.int16)
    ys, xs = torch.arange(-4, H + 4), torch.arange(-4, W + 4)      # every pixel some window holds: the frame and 4 pixels around it
    for k in range(1, F):
        cur = _clamped(y[k], ys, xs)
        best = None
        for dy in range(-R, R + 1):
            for dx in range(-R, R + 1):
                diff = (cur - _clamped(y[k - 1], ys + dy, xs + dx)).abs()
                cost = diff.unfold(0, 16, 8).unfold(1, 16, 8).sum(dim=(-1, -2))      # [h, w]: the window of cell c starts at 8 c - 4
                cand = (cost, torch.full_like(cost, dy * dy + dx * dx), torch.full_like(cost, dy), torch.full_like(cost, dx))
                if best is None:
                    best = cand
                    continue
                less = torch.zeros_like(cost, dtype=torch.bool)
                equal = torch.ones_like(cost, dtype=torch.bool)
                for a, b in zip(cand, best):                                             # lexicographic: the first component that differs
                    less |= equal & (a < b)
                    equal &= a == b
                best = tuple(torch.where(less, a, b) for a, b in zip(cand, best))
        flow[k, ..., 0], flow[k, ..., 1] = best[2].to(torch.int16), best[3].to(torch.int16)
    return flow


def flow_median(flow):
    """Every component -> the median of its 3 x 3 cell neighbourhood, replicate border, per frame."""
    F, h, w, _ = flow.shape
    out = torch.empty_like(flow)
    for f in range(F):
        for c in range(2):
            nine = torch.stack([_clamped(flow[f, :, :, c], torch.arange(h) + a, torch.arange(w) + b) for a in (-1, 0, 1) for b in (-1, 0, 1)])
            out[f, :, :, c] = nine.sort(dim=0).values[4]
    return out


def propagate(mask0, flow):
    """The sequential warp: mask_k[p] = mask_{k-1}[clamp(p + D_k[cell(p)])].  bool [H, W], int16 [F, h, w, 2] -> bool [F, H, W]."""
    F, h, w, _ = flow.shape
    H, W = 8 * h, 8 * w
    assert tuple(mask0.shape) == (H, W)
    py, px = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    masks = [mask0 != 0]
    for k in range(1, F):
        d = flow[k].to(torch.int64)[py // 8, px // 8]
        masks.append(masks[-1][(py + d[..., 0]).clamp(0, H - 1), (px + d[..., 1]).clamp(0, W - 1)])
    return torch.stack(masks)


def propagate_chain(mask0, flow):
    """What the kernel does per pixel: q <- clamp(q + D_j[cell(q)]) for j = k .. 1, then mask_0[q].  Equal to ``propagate`` by induction on
    k: mask_k[p] = mask_{k-1}[q_1] with q_1 the first step, and mask_{k-1}[q_1] is, by hypothesis, the chain j = k - 1 .. 1 from q_1."""
    F, h, w, _ = flow.shape
    H, W = 8 * h, 8 * w
    py, px = torch.meshgrid(torch.arange(H), torch.arange(W), indexing="ij")
    m0, out = mask0 != 0, []
    for k in range(F):
        qy, qx = py.clone(), px.clone()
        for j in range(k, 0, -1):
            d = flow[j].to(torch.int64)[qy // 8, qx // 8]
            qy, qx = (qy + d[..., 0]).clamp(0, H - 1), (qx + d[..., 1]).clamp(0, W - 1)
        out.append(m0[qy, qx])
    return torch.stack(out)


def first_frame_mask(source, edited, threshold=24, min_count=8):
    """uint8 [H, W, 3] twice -> bool [1, H, W], constant on cells."""
    H, W, _ = source.shape
    changed = ((edited.to(torch.int64) - source.to(torch.int64)).abs().amax(dim=-1) > threshold).to(torch.int64)
    count = changed.view(H // 8, 8, W // 8, 8).sum(dim=(1, 3))
    return (count >= min_count).repeat_interleave(8, dim=0).repeat_interleave(8, dim=1)[None]


def track(frames, mask0, radius=16, median=True):
    """Frames uint8 [F, H, W, 3], frame-0 mask [H, W] -> (bool [F, H, W], int16 [F, h, w, 2])."""
    flow = block_match(luma(frames), radius)
    if median:
        flow = flow_median(flow)
    return propagate(mask0, flow), flow
