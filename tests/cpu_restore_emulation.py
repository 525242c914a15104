"""TEST-ONLY torch emulation of ``ops.restore_u8`` on the CPU, beside ``cpu_resample_emulation``: the passes ``ops.restore_passes`` plans
(the library's own tables: building them touches no GPU) -- the horizontal passes, then what ``anyv2v_restore_paste_u8`` does: the vertical
table walk of the edit and of alpha and the paste formula against the source byte, bytes outside ``dest`` copied.  ``test_restore_host``
holds it against Pillow bit for bit on the GPU test's shapes.  Never importable from the product."""
from __future__ import annotations

import torch

from cpu_resample_emulation import _one_pass


def restore_u8(edited_u8, source_u8, dest, box, resample="lanczos", alpha_u8=None):
    from anyv2v_amd import ops
    ok = lambda t, nd: isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.dim() == nd and t.shape[0] >= 1
    if not (ok(edited_u8, 4) and ok(source_u8, 4) and edited_u8.shape[3] == 3 and source_u8.shape[3] == 3 and source_u8.shape[0] == edited_u8.shape[0]):
        raise ValueError("restore_u8: uint8 [F, h, w, 3] and [F, sh, sw, 3] tensors expected")
    F, h, w, _ = (int(v) for v in edited_u8.shape)
    if alpha_u8 is not None and not (ok(alpha_u8, 3) and alpha_u8.shape[0] in (1, F) and tuple(alpha_u8.shape[1:]) == (h, w)):
        raise ValueError(f"restore_u8: alpha_u8: a uint8 [1 or {F}, {h}, {w}] tensor expected")
    dx0, dy0, dx1, dy1 = ops._dest(dest, int(source_u8.shape[1]), int(source_u8.shape[2]), "restore_u8")
    pe, pa = ops.restore_passes(h, w, (dx0, dy0, dx1, dy1), box, resample)

    def resized(x, p):
        row0, rows, hp, vp = p
        x = x[:, row0:row0 + rows]
        return _one_pass(x if hp is None else _one_pass(x, 2, hp), 1, vp)        # (the identity table where Pillow skips the vertical pass)
    e = resized(edited_u8, pe).to(torch.int64)
    m = torch.full((1, dy1 - dy0, dx1 - dx0, 1), 255, dtype=torch.int64) if alpha_u8 is None else resized(alpha_u8[..., None], pa).to(torch.int64)
    out = source_u8.clone()
    d = out[:, dy0:dy1, dx0:dx1].to(torch.int64)
    t = d * (255 - m) + e * m + 128
    out[:, dy0:dy1, dx0:dx1] = (((t >> 8) + t) >> 8).to(torch.uint8)
    return out


def install(monkeypatch=None):
    """``cpu_resample_emulation.install`` plus ``ops.restore_u8`` (tests only)."""
    import cpu_resample_emulation as remu
    from anyv2v_amd import ops
    remu.install(monkeypatch)
    if monkeypatch is not None:
        monkeypatch.setattr(ops, "restore_u8", restore_u8, raising=False)
    else:
        ops.restore_u8 = restore_u8
