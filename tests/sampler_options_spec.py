"""TEST-ONLY definitions of the two sampler options of the I2VGen-XL step engines, restated in fp64:

* guidance rescale -- ``rescale_noise_cfg`` of ``consisti2v/consisti2v/pipelines/pipeline_video_editing.py:50-61`` (Lin et al., "Common
  Diffusion Noise Schedules and Sample Steps are Flawed", 3.4);
* stochastic DDIM -- ``GaussianDiffusion.ddim_sample`` with ``eta`` of ``seine/diffusion/gaussian_diffusion.py:547-600`` (Song et al.
  eq. 12 / 16), the in-tree statement of diffusers' ``DDIMScheduler.step(eta=, generator=)``.

``tests/golden/sampler_options_ref.pt`` (written by ``tests/golden/make_sampler_golden.py`` from the reference's own code) pins both.
What is NOT restated in fp64 is the classifier-free-guidance combine: the reference forms it on fp16 tensors
(``pipeline_i2vgen_xl.py:1160-1162``), the kernels round the same three operations to fp16, and ``guided_fp16`` is that arithmetic."""
from __future__ import annotations

import math

import torch

PRED_V, PRED_EPSILON, PRED_SAMPLE = 0, 1, 2


def guided_fp16(e_unc: torch.Tensor, e_txt: torch.Tensor, guidance: float) -> torch.Tensor:
    """``neg + g * (text - neg)`` on fp16 tensors: torch rounds each of the three operations to fp16, as the reference's loop does."""
    assert e_unc.dtype == e_txt.dtype == torch.float16
    return e_unc + guidance * (e_txt - e_unc)


def rescale_noise_cfg(noise_cfg: torch.Tensor, noise_pred_text: torch.Tensor, guidance_rescale: float) -> torch.Tensor:
    """fp64; statistics per batch element over every other dimension, unbiased (``torch.std``)."""
    cfg, txt = noise_cfg.double(), noise_pred_text.double()
    dims = list(range(1, txt.ndim))
    std_text = txt.std(dim=dims, keepdim=True)
    std_cfg = cfg.std(dim=dims, keepdim=True)
    rescaled = cfg * (std_text / std_cfg)
    return guidance_rescale * rescaled + (1 - guidance_rescale) * cfg


def eta_sigma(a_t: float, a_p: float, eta: float) -> float:
    """``gaussian_diffusion.py:585-589``."""
    return eta * math.sqrt((1 - a_p) / (1 - a_t)) * math.sqrt(1 - a_t / a_p)


def eta_row(a_t: float, a_p: float, eta: float, phi: float = 0.0, n: int = 0):
    """The 8 coefficients of one step {sa_t, sb_t, c_x0, c_eps, sigma, phi, n, 0} in fp64 (``:583-595``)."""
    sigma = eta_sigma(a_t, a_p, eta)
    return (math.sqrt(a_t), math.sqrt(1 - a_t), math.sqrt(a_p), math.sqrt(max(1 - a_p - sigma ** 2, 0.0)), sigma, float(phi), float(n), 0.0)


def x0_eps(e: torch.Tensor, x: torch.Tensor, sa_t: float, sb_t: float, prediction: int):
    e, x = e.double(), x.double()
    if prediction == PRED_V:
        return sa_t * x - sb_t * e, sa_t * e + sb_t * x
    if prediction == PRED_EPSILON:
        return (x - sb_t * e) / sa_t, e
    return e, (x - sa_t * e) / sb_t


def ddim_eta_step(e: torch.Tensor, x: torch.Tensor, row, noise=None, prediction: int = PRED_V) -> torch.Tensor:
    """``:592-599`` in fp64: sqrt(a_p) x0 + sqrt(1 - a_p - sigma^2) eps + sigma noise, coefficients from ``row`` (``eta_row``)."""
    sa_t, sb_t, c_x0, c_eps, sigma = (float(c) for c in row[:5])
    x0, eps = x0_eps(e, x, sa_t, sb_t, prediction)
    y = c_x0 * x0 + c_eps * eps
    return y if noise is None else y + sigma * noise.double()


def branch_planar(vtok: torch.Tensor, b: int, C: int, F: int, H: int, W: int) -> torch.Tensor:
    """Branch ``b`` of the channels-last token matrix [(nb F) H W, ld] -> planar [1, C, F, H, W]."""
    n = F * H * W
    return vtok[b * n:(b + 1) * n, :C].reshape(F, H, W, C).permute(3, 0, 1, 2).unsqueeze(0).contiguous()


def fused_step(vtok: torch.Tensor, b_unc: int, b_cond: int, guidance: float, row, lat: torch.Tensor, noise=None, prediction: int = PRED_V):
    """What ``ops.guidance_stats`` + ``ops.cfg_ddim_step_ex`` compute, by the definitions: the fp16 guided prediction, the rescale with
    ``phi = row[5]`` (skipped without guidance, ``pipeline_video_editing.py:685``), the step -- fp64 [1, C, F, H, W], not rounded."""
    _, C, F, H, W = lat.shape
    txt = branch_planar(vtok, b_cond, C, F, H, W)
    g = txt
    if b_unc >= 0:
        g = guided_fp16(branch_planar(vtok, b_unc, C, F, H, W), txt, guidance)
        if float(row[5]) > 0:
            g = rescale_noise_cfg(g, txt, float(row[5]))
    return ddim_eta_step(g, lat, row, noise, prediction)


def ulp_distance_fp16(a: torch.Tensor, b: torch.Tensor) -> int:
    """Largest distance between two fp16 tensors counted in representable fp16 values."""
    def key(t):
        i = t.contiguous().view(torch.int16).to(torch.int32)
        return torch.where(i < 0, -(i & 0x7FFF), i)
    return int((key(a.half()) - key(b.half())).abs().max())
