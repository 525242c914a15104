"""TEST-ONLY definition of the masked PnP edit, restated in torch fp64.  Nothing in the reference implements it (the technique is the
latent blending of Blended Latent Diffusion, arXiv 2206.02779, and of diffusers' inpaint loop ``latents = (1 - mask) * init_latents_proper
+ mask * latents``, with the inverted latent of the source in the place of the re-noised one), so this file IS the contract the kernels
of ``anyv2v_amd/csrc/mask.hip`` are tested against:

* latent mask -- pixel mask [Fm, H, W] fp16 in [0, 1]: (1) mean over each 8 x 8 block, (2) maximum over the (2 r + 1)^2 window with
  positions outside the image ignored, (3) separable Gaussian of radius ceil(3 sigma) with replicate padding; stages in fp32, one rounding
  to fp16 at the end.  "In fp32" is stated here as: the pooled value is the EXACT mean rounded to fp32 once (the ideal fp32 result; sums
  of 64 fp16 values in [0, 1] are exact in fp64), the maximum is exact, and the feather is evaluated in fp64 on those fp32 values with
  the fp32 taps -- the kernel's fp32 accumulation may differ from it by far less than half an fp16 ulp, so only ties can move;
* blend -- ``m == 0 -> s``, ``m == 1 -> x`` (selects), else ``fp16(fmaf(m, x - s, s))``: the difference rounded to fp32, the fma
  rounded to fp32, then to fp16;
* the edit loop -- after the step at ``ts[i]`` the edit latent is blended against the source at level ``ts[i + 1]`` (the trajectory's
  entry), after the last step against the clean source latent."""
from __future__ import annotations

import math
import types

import torch

import sampler_options_spec as sspec


def gaussian_taps(sigma: float) -> torch.Tensor:
    """exp(-k^2 / (2 sigma^2)) / sum for k = -R .. R, R = ceil(3 sigma): fp64, rounded to fp32 -> float32 [2 R + 1] (empty: no feather)."""
    R = int(math.ceil(3.0 * float(sigma)))
    if R == 0:
        return torch.zeros(0, dtype=torch.float32)
    k = torch.arange(-R, R + 1, dtype=torch.float64)
    raw = torch.exp(-(k * k) / (2.0 * float(sigma) ** 2))
    return (raw / raw.sum()).float()


def latent_mask(mask: torch.Tensor, grow: int = 0, sigma: float = 0.0) -> torch.Tensor:
    """-> fp64 [Fm, H / 8, W / 8], NOT yet rounded to fp16 (``.half()`` is the one rounding)."""
    assert mask.dim() == 3 and mask.dtype == torch.float16
    Fm, H, W = mask.shape
    h, w = H // 8, W // 8
    m = mask.double().clamp(0.0, 1.0).view(Fm, h, 8, w, 8).sum(dim=(2, 4)) / 64.0     # exact in fp64
    m = m.float().double()                                                             # the stage's result is an fp32 value
    r = int(grow)
    if r > 0:
        big = torch.full((Fm, h + 2 * r, w + 2 * r), -1.0, dtype=torch.float64)        # outside the image: ignored (every value is >= 0)
        big[:, r:r + h, r:r + w] = m
        m = torch.stack([big[:, dy:dy + h, dx:dx + w] for dy in range(2 * r + 1) for dx in range(2 * r + 1)]).amax(dim=0)
    taps = gaussian_taps(sigma).double()
    R = taps.numel() // 2
    if R > 0:
        ys = (torch.arange(h)[:, None] + torch.arange(-R, R + 1)[None, :]).clamp(0, h - 1)   # replicate padding: clamped indices
        xs = (torch.arange(w)[:, None] + torch.arange(-R, R + 1)[None, :]).clamp(0, w - 1)
        m = (m[:, :, xs] * taps).sum(dim=-1)                     # along w: [Fm, h, w]
        m = (m[:, ys, :] * taps[None, None, :, None]).sum(dim=2)   # along h
    return m


def blend(x: torch.Tensor, s: torch.Tensor, m: torch.Tensor) -> torch.Tensor:
    """x / s [1, C, F, h, w] fp16, m [Fm, h, w] fp16 (Fm 1 or F) -> fp16.  The fp32 fma is formed in fp64: m (x - s) is exact there
    (11 x 24 bits), and the sum with s is checked to be exact too (two-sum error term) wherever it is finite -- a correctly rounded fma."""
    assert x.dtype == s.dtype == m.dtype == torch.float16 and x.shape == s.shape and m.shape[0] in (1, x.shape[2])
    mm = m[None, None].expand(x.shape).double()
    xd, sd = x.double(), s.double()
    d = (xd - sd).float().double()
    p = mm * d
    t = p + sd
    bv = t - p
    err = (p - (t - bv)) + (sd - bv)
    sel = (mm != 0) & (mm != 1) & torch.isfinite(t)
    assert bool((err[sel] == 0).all()), "the fp64 restatement of the fp32 fma is not exact for these operands"
    y = t.float().half()
    return torch.where(mm == 0, s, torch.where(mm == 1, x, y))


def partners(ts, traj, source_latents):
    """The partner of step i: the source at the level the edit latent arrives at -- ``traj[ts[i + 1]]``, the clean latent after the last."""
    return [traj[ts[i + 1]] if i + 1 < len(ts) else source_latents for i in range(len(ts))]


def masked_edit_loop(c, steps, lat_mask, source_latents, register, eta=0.0, phi=0.0, seed=0, guidance=9.0):
    """The PnP edit loop by the definitions (the spec loop of tests/test_sampler_options_host.py: the native UNet's prediction of every
    branch, fp16 guidance, fp64 rescale and step, fp16 latents between the steps) with the blend behind every step.  ``c``: the clip
    namespace of those tests (native, traj, T, ehs, ie, il); ``register(holder)`` registers the injection schedules and returns the
    scheduler.  -> (final latent, {t: latent after the step at t})."""
    from anyv2v_amd import pnp_utils
    holder = types.SimpleNamespace(unet=c.native, register_modules=lambda **kw: None)
    sched = register(holder)
    sched.set_timesteps(steps)
    gen = torch.Generator().manual_seed(seed)
    lat = c.traj[c.T].clone()
    kw = dict(fps=torch.tensor([8] * 3, device=lat.device), encoder_hidden_states=c.ehs,
              image_embeddings=torch.cat([c.ie[:1], torch.zeros_like(c.ie[:1]), c.ie[2:3]]),
              image_latents=torch.cat([c.il[:1], c.il[2:3], c.il[2:3]]))
    ts = [int(t) for t in sched.timesteps]
    trace = {}
    try:
        for t, partner in zip(ts, partners(ts, c.traj, source_latents)):
            pnp_utils.register_time(holder, t)
            v = c.native(torch.cat([c.traj[t], lat, lat]), t, **kw)[0]
            e_unc, e_txt = v[-2:-1].half(), v[-1:].half()
            g = sspec.guided_fp16(e_unc, e_txt, guidance)
            if phi > 0:
                g = sspec.rescale_noise_cfg(g, e_txt, phi)
            noise = torch.randn(lat.shape, generator=gen, dtype=torch.float32).half().to(lat.device) if eta > 0 else None
            a_t, a_p = float(sched.alphas_cumprod[t]), sched._abar(t - sched._ratio())
            lat = sspec.ddim_eta_step(g, lat, sspec.eta_row(a_t, a_p, eta), noise).half()
            lat = blend(lat.cpu(), partner.cpu(), lat_mask.cpu()).to(lat.device)
            trace[t] = lat.clone()
    finally:
        pnp_utils.clear_time(holder)
    return lat, trace
