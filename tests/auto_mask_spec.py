"""TEST-ONLY definition of the automatic edit mask, restated in torch fp64.  Nothing in the reference implements it; the method is
DiffEdit's (Couairon et al., arXiv 2210.11427; diffusers' ``StableDiffusionDiffEditPipeline.generate_mask``) with one mean over the whole
clip, so this file IS the contract the kernels of ``anyv2v_amd/csrc/automask.hip`` and ``I2VGenXLPipeline.generate_edit_mask`` are tested
against:

* per map k: ``x_t = scheduler.add_noise(x0, noise_k, t)`` rounded to fp16, the UNet's raw outputs ``v_src``, ``v_tgt`` on the batch
  [source, edit] of the same ``x_t`` (no classifier-free guidance), ``acc[f, y, x] += sum_c |v_tgt - v_src|``: the difference of two fp16
  values and its absolute value are exact in fp32, channels are added in the order 0 .. C - 1 in fp32, maps in the order 0 .. N - 1 in fp32;
* ``mean = sum(acc) / (F h w)``, ONE mean over the clip; ``map = clamp(ratio * acc / mean, 0, 1)`` rounded once to fp16; ``mean == 0`` gives
  ``map = 0``; ``mask = map_fp16 > fp16(threshold)``, at the pixel size with each latent pixel replicated over its 8 x 8 block;
* the timestep: with ``num_inference_steps`` set on the forward DDIM scheduler, ``init = min(int(steps * strength), steps)`` and
  ``t = timesteps[steps - init]`` (diffusers' ``get_timesteps``), the index clamped to the last timestep."""
from __future__ import annotations

import torch


def accumulate(v_src: torch.Tensor, v_tgt: torch.Tensor, acc=None) -> torch.Tensor:
    """v_src / v_tgt fp16 [C, F, h, w] (or [C, n]) -> fp32 accumulator of the trailing shape: ``acc + sum_c |v_tgt - v_src|`` in the stated
    order, ``acc`` None for the first map."""
    assert v_src.dtype == v_tgt.dtype == torch.float16 and v_src.shape == v_tgt.shape
    d = (v_tgt.float() - v_src.float()).abs()
    s = torch.zeros_like(d[0])
    for c in range(d.shape[0]):
        s = s + d[c]
    return s if acc is None else acc + s


def finish(acc: torch.Tensor, ratio: float, threshold: float):
    """fp32 accumulator [F, h, w] -> (map fp64 NOT yet rounded, map fp16, mask bool [F, h, w])."""
    a = acc.double()
    mean = a.sum() / a.numel()
    m = (float(ratio) * a / mean).clamp(0.0, 1.0) if float(mean) != 0.0 else torch.zeros_like(a)
    m16 = m.half()
    thr = torch.tensor(float(threshold), dtype=torch.float64).half()
    return m, m16, m16 > thr


def pixel_mask(mask: torch.Tensor) -> torch.Tensor:
    """bool [F, h, w] -> bool [F, 8 h, 8 w]: each latent pixel replicated over its 8 x 8 block."""
    return mask.repeat_interleave(8, dim=1).repeat_interleave(8, dim=2)


def generate(v_pairs, ratio: float, threshold: float):
    """``v_pairs``: one (v_src, v_tgt) per map, fp16 [C, F, h, w] -> (map fp16 [F, h, w], pixel mask bool [F, 8 h, 8 w], accumulator)."""
    acc = None
    for v_src, v_tgt in v_pairs:
        acc = accumulate(v_src, v_tgt, acc)
    _, m16, mask = finish(acc, ratio, threshold)
    return m16, pixel_mask(mask), acc


def timestep(timesteps, steps: int, strength: float) -> int:
    init = min(int(steps * strength), steps)
    return int(timesteps[min(steps - init, steps - 1)])


def near_threshold(map64: torch.Tensor, threshold: float) -> torch.Tensor:
    """Elements whose exact map lies within 1 fp16 ulp of fp16(threshold): where a kernel whose map is within 1 ulp of the rounded
    definition may decide the other way.  (The ulp is that of the threshold's binade: 2^-11 for a threshold in [0.5, 1).)"""
    import math
    thr = float(torch.tensor(float(threshold), dtype=torch.float64).half())
    ulp = 2.0 ** (math.floor(math.log2(thr)) - 10)
    return (map64 - thr).abs() <= ulp


def fixture(F: int, h: int, w: int, N: int, seed: int, C: int = 4, special: bool = True):
    """The kernels' test inputs, shared by the GPU tests and the host test that checks the share of near-threshold elements: N maps of
    (v_src, v_tgt) fp16 [C, F h w].  The edit differs from the source by a smooth per-pixel amplitude (so the map is spread over [0, 1]
    and beyond the clamp) plus noise; with ``special`` a few elements hold +-65504, subnormals and equal values."""
    g = torch.Generator().manual_seed(seed)
    n = F * h * w
    amp = torch.rand(n, generator=g) ** 2 * 3.0
    pairs = []
    for _ in range(N):
        vs = torch.randn(C, n, generator=g)
        vt = vs + amp[None] * torch.randn(C, n, generator=g) * 0.5
        vs, vt = vs.half(), vt.half()
        if special and n >= 8:
            vs[0, 0], vt[0, 0] = 65504.0, -65504.0            # the largest difference: 131008 is exact in fp32
            vs[1, 1], vt[1, 1] = 6e-8, -6e-8                  # subnormals
            vs[2, 2], vt[2, 2] = 5.96e-8, 1.0
            vt[:, 3] = vs[:, 3]                               # equal values: a zero
            vs[3, 4], vt[3, 4] = -65504.0, -65504.0
        pairs.append((vs, vt))
    return pairs
