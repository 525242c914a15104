"""TEST-ONLY torch emulation of the two automatic-mask ops (``ops.diff_map_accum``, ``ops.diff_map_finish``) on the CPU, beside
``cpu_masked_edit_emulation``: each function restates the contract of ``include/anyv2v_hip.h`` (the channel sum of absolute differences in
fp32 in channel order; the clip mean folded in fp64, the scale ``ratio / mean`` rounded to fp32, one fp32 product, one rounding to fp16, the
comparison on the rounded map).  Never importable from the product."""
from __future__ import annotations

import torch


def diff_map_accum(vtok, C_, F, HW, acc, first):
    n = F * HW
    assert vtok.dtype == torch.float16 and vtok.shape[0] >= 2 * n and vtok.shape[1] >= C_ and acc.dtype == torch.float32 and acc.numel() == n
    d = (vtok[n:2 * n, :C_].float() - vtok[:n, :C_].float()).abs()
    s = torch.zeros(n, dtype=torch.float32)
    for c in range(C_):
        s = s + d[:, c]
    if torch.is_tensor(first):
        first = bool(int(first.reshape(-1)[0]))
    flat = acc.view(-1)
    flat.copy_(s if first else flat + s)
    return acc


def diff_map_finish(acc, F, h, w, ratio, threshold, out=None):
    assert acc.dtype == torch.float32 and acc.numel() == F * h * w
    if not (ratio > 0 and ratio < float("inf")) or not 0.0 < threshold < 1.0:
        raise ValueError("diff_map_finish: ratio must be finite and > 0, threshold in (0, 1)")
    a = acc.reshape(F, h, w)
    mean = a.double().sum() / a.numel()
    scale = torch.tensor(float(ratio) / float(mean) if float(mean) > 0.0 else 0.0, dtype=torch.float32)
    m = torch.nan_to_num(a * scale, nan=0.0).clamp(0.0, 1.0).half()
    mask = m > torch.tensor(float(threshold)).half()
    pm = mask.repeat_interleave(8, dim=1).repeat_interleave(8, dim=2)
    if out is not None:
        out[0].copy_(m)
        out[1].copy_(pm)
        return out
    return m, pm


def install(monkeypatch=None):
    """``cpu_masked_edit_emulation.install`` plus the two automatic-mask ops (tests only)."""
    import cpu_masked_edit_emulation as memu
    from anyv2v_amd import ops
    memu.install(monkeypatch)
    for name, fn in (("diff_map_accum", diff_map_accum), ("diff_map_finish", diff_map_finish)):
        if monkeypatch is not None:
            monkeypatch.setattr(ops, name, fn, raising=False)
        else:
            setattr(ops, name, fn)
