"""TEST-ONLY torch emulation of ``ops.detail_gate_u8`` and ``ops.restore_detail_u8`` on the CPU, beside ``cpu_restore_emulation``: the gate
the way the kernels form it (row sums that must fit a uint16, then column sums and the ramp), and the passes ``ops.restore_passes`` plans
followed by what ``anyv2v_restore_detail_u8`` does.  ``test_restore_detail_host`` holds both against ``tests/detail_spec.py`` bit for bit on
the GPU test's shapes.  Never importable from the product."""
from __future__ import annotations

import torch

from cpu_resample_emulation import _one_pass


def _frames(t, nd, last=None):
    return isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.dim() == nd and t.shape[0] >= 1 and (last is None or t.shape[-1] == last)


def detail_gate_u8(edit_u8, prepared_u8, lo=8, hi=32, radius=2):
    from anyv2v_amd import ops
    if not (_frames(edit_u8, 4, 3) and _frames(prepared_u8, 4, 3) and edit_u8.shape == prepared_u8.shape):
        raise ValueError("detail_gate_u8: two uint8 [F, h, w, 3] tensors of one shape expected")
    lo, hi, radius = ops.detail_parameters(lo, hi, radius, "detail_gate_u8: ")
    c = (edit_u8.to(torch.int64) - prepared_u8.to(torch.int64)).abs().amax(dim=3)                      # [F, h, w]
    h, w = int(c.shape[1]), int(c.shape[2])
    taps = torch.arange(-radius, radius + 1)
    xs = (torch.arange(w)[:, None] + taps[None, :]).clamp(0, w - 1)                                    # [w, 2r + 1]
    rows = c[:, :, xs].sum(dim=-1)
    assert int(rows.max()) < 65536                                                                     # the kernels' intermediate is uint16
    ys = (torch.arange(h)[:, None] + taps[None, :]).clamp(0, h - 1)
    b = rows[:, ys, :].sum(dim=2)                                                                      # [F, h, 2r + 1, w] -> [F, h, w]
    n = (2 * radius + 1) ** 2
    mean = (b + n // 2) // n
    ramp = (255 * (hi - mean) + (hi - lo) // 2) // (hi - lo)
    return torch.where(mean <= lo, 255, torch.where(mean >= hi, 0, ramp)).to(torch.uint8)


def restore_detail_u8(edited_u8, prepared_u8, gate_u8, source_u8, dest, box, resample="lanczos", alpha_u8=None):
    from anyv2v_amd import ops
    if not (_frames(edited_u8, 4, 3) and _frames(source_u8, 4, 3) and _frames(prepared_u8, 4, 3) and prepared_u8.shape == edited_u8.shape
            and source_u8.shape[0] == edited_u8.shape[0]):
        raise ValueError("restore_detail_u8: uint8 [F, h, w, 3] (twice) and [F, sh, sw, 3] tensors expected")
    F, h, w, _ = (int(v) for v in edited_u8.shape)
    for name, t in (("gate_u8", gate_u8),) + (() if alpha_u8 is None else (("alpha_u8", alpha_u8),)):
        if not (_frames(t, 3) and t.shape[0] in (1, F) and tuple(t.shape[1:]) == (h, w)):
            raise ValueError(f"restore_detail_u8: {name}: a uint8 [1 or {F}, {h}, {w}] tensor expected")
    dx0, dy0, dx1, dy1 = ops._dest(dest, int(source_u8.shape[1]), int(source_u8.shape[2]), "restore_detail_u8")
    pe, pa = ops.restore_passes(h, w, (dx0, dy0, dx1, dy1), box, resample)

    def resized(x, p):
        row0, rows, hp, vp = p
        x = x[:, row0:row0 + rows]
        return _one_pass(x if hp is None else _one_pass(x, 2, hp), 1, vp).to(torch.int64)
    e, p, g = resized(edited_u8, pe), resized(prepared_u8, pe), resized(gate_u8[..., None], pa)
    m = torch.full_like(g[:1], 255) if alpha_u8 is None else resized(alpha_u8[..., None], pa)
    out = source_u8.clone()
    d = out[:, dy0:dy1, dx0:dx1].to(torch.int64)
    add = ((d - p) * (g + (g >> 7)) + 128) >> 8
    e2 = (e + add).clamp(0, 255)
    t = d * (255 - m) + e2 * m + 128
    out[:, dy0:dy1, dx0:dx1] = (((t >> 8) + t) >> 8).to(torch.uint8)
    return out


def install(monkeypatch=None):
    """``cpu_restore_emulation.install`` plus the two ops above (tests only)."""
    import cpu_restore_emulation as remu
    from anyv2v_amd import ops
    remu.install(monkeypatch)
    for name, fn in (("detail_gate_u8", detail_gate_u8), ("restore_detail_u8", restore_detail_u8)):
        if monkeypatch is not None:
            monkeypatch.setattr(ops, name, fn, raising=False)
        else:
            setattr(ops, name, fn)
