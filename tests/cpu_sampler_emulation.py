"""TEST-ONLY torch emulation of the two sampler-option ops (``ops.guidance_stats``, ``ops.cfg_ddim_step_ex``) on the CPU, beside
``cpu_ops_emulation``: each function restates the contract of ``include/anyv2v_hip.h`` (fp16 guided prediction, sums about the first
element as pivot in fp32 records, fold in fp64, the factor in fp32, one rounding of the result).  Never importable from the product."""
from __future__ import annotations

import torch

BLOCKS, RECORD = 64, 8   # ANYV2V_GUIDANCE_STATS_BLOCKS / _RECORD


def _h(t):
    return t.half().float()


def _planar(vtok, b, C, Fr, H, W):
    n = Fr * H * W
    return vtok[b * n:(b + 1) * n, :C].float().view(Fr, H, W, C).permute(3, 0, 1, 2)


def _guided(vu, v, g):
    return _h(vu + _h(g * _h(v - vu)))


def guidance_stats(vtok, b_unc, b_cond, guidance, lat_shape, out=None):
    _, C, Fr, H, W = lat_shape
    assert b_unc >= 0
    txt = _planar(vtok, b_cond, C, Fr, H, W)
    cfg = _guided(_planar(vtok, b_unc, C, Fr, H, W), txt, guidance)
    kt, kg = txt.reshape(-1)[0], cfg.reshape(-1)[0]          # (pixel 0, channel 0)
    if out is None:
        out = torch.empty(BLOCKS * RECORD, dtype=torch.float32)
    out.zero_()
    rec = out[:BLOCKS * RECORD].view(BLOCKS, RECORD)
    rec[:, 4], rec[:, 5] = kt, kg
    # (the kernel spreads the pixels over the blocks; any split folds to the same sums up to fp32 rounding -- all in record 0 here)
    rec[0, 0], rec[0, 1] = (txt - kt).sum(), ((txt - kt) ** 2).sum()
    rec[0, 2], rec[0, 3] = (cfg - kg).sum(), ((cfg - kg) ** 2).sum()
    return out


def cfg_ddim_step_ex(vtok, b_unc, b_cond, guidance, row, lat, out, *, prediction=0, stats=None, phi=0.0, noise=None):
    _, C, Fr, H, W = lat.shape
    sa_t, sb_t, c_x0, c_eps, sigma, phi_row, n = (float(c) for c in row[:7])
    assert 0.0 <= phi <= 1.0 and (phi == 0.0 or abs(phi - phi_row) < 1e-6)   # (the host's copy of row[5])
    v = _planar(vtok, b_cond, C, Fr, H, W)
    if b_unc >= 0:
        v = _guided(_planar(vtok, b_unc, C, Fr, H, W), v, guidance)
        if stats is not None and phi_row > 0:
            assert n >= 2
            rec = stats[:BLOCKS * RECORD].view(BLOCKS, RECORD).double()
            st, qt, sg, qg = (rec[:, i].sum() for i in range(4))
            std_t = (((qt - st * st / n).clamp_min(0) / (n - 1)).sqrt()).float()
            std_g = (((qg - sg * sg / n).clamp_min(0) / (n - 1)).sqrt()).float()
            s = torch.tensor(phi_row) * (std_t / std_g) + (1.0 - torch.tensor(phi_row))
            v = _h(v * s)
    x = lat.float()[0]
    if prediction == 0:
        x0, eps = sa_t * x - sb_t * v, sa_t * v + sb_t * x
    elif prediction == 1:
        x0, eps = (x - sb_t * v) / sa_t, v
    else:
        x0, eps = v, (x - sa_t * v) / sb_t
    y = c_x0 * x0 + c_eps * eps
    if noise is not None:
        y = y + sigma * noise.float().reshape(x.shape)
    out[0] = y.half()
    return out


def install(monkeypatch=None):
    """``cpu_ops_emulation.install`` plus the two sampler-option ops (tests only)."""
    import cpu_ops_emulation as emu
    from anyv2v_amd import ops
    emu.install(monkeypatch)
    for name, fn in (("guidance_stats", guidance_stats), ("cfg_ddim_step_ex", cfg_ddim_step_ex)):
        if monkeypatch is not None:
            monkeypatch.setattr(ops, name, fn, raising=False)
        else:
            setattr(ops, name, fn)
