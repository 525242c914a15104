"""Writes ``tests/golden/sampler_options_ref.pt`` by running the REFERENCE's own code on the CPU (needs the reference tree):

* ``rescale_noise_cfg`` of ``consisti2v/consisti2v/pipelines/pipeline_video_editing.py:50-61`` -- the file imported verbatim the way
  ``oracle/ref_consisti2v_pipeline.py`` imports it -- on fp64 and on fp16 tensors;
* ``GaussianDiffusion.ddim_sample`` with ``eta`` of ``seine/diffusion/gaussian_diffusion.py:547-600`` on ``respace.SpacedDiffusion`` with the
  I2VGen-XL betas (cosine, zero terminal SNR) respaced to the 50 sampling timesteps, the v-prediction handed over in its x0 form.

The file holds data only: the inputs and what the reference returned.  ``python tests/golden/make_sampler_golden.py [out.pt]``;
``tests/test_sampler_options_host.py`` re-runs ``build()`` live against the committed file when the reference tree is present."""
from __future__ import annotations

import importlib.util
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

OUT = os.path.join(ROOT, "tests", "golden", "sampler_options_ref.pt")
GUIDANCE = 9.0
PHIS = (0.0, 0.7, 1.0)
ETA = 0.5
STEP_INDICES = (0, 1, 10, 30, 49)     # into the ascending 50 sampling timesteps 1, 21, ..., 981
SHAPES = ((1, 4, 2, 8, 8), (2, 4, 3, 5, 7))


def _seine_diffusion():
    from oracle import ref_stubs
    root = os.path.join(ref_stubs.REFERENCE_ROOT, "seine", "diffusion")
    name = "_ref_seine_diffusion_sampler_golden"
    spec = importlib.util.spec_from_file_location(name, os.path.join(root, "__init__.py"), submodule_search_locations=[root])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return name, mod, sys.modules[name + ".gaussian_diffusion"]


def build() -> dict:
    from anyv2v_amd.schedulers import DDIMScheduler
    from oracle import ref_consisti2v_pipeline as rcp
    pm = rcp.load_reference_consisti2v_pipeline()[0]
    out = {"guidance": GUIDANCE, "eta": ETA, "rescale": [], "ddim": []}
    for k, shape in enumerate(SHAPES):
        g = torch.Generator().manual_seed(100 + k)
        e_unc = (torch.randn(shape, generator=g) + 0.25).half()
        e_txt = (torch.randn(shape, generator=g) + 0.25).half()
        cfg16 = e_unc + GUIDANCE * (e_txt - e_unc)            # the reference's fp16 guidance (pipeline_video_editing.py:679-683)
        for phi in PHIS:
            out["rescale"].append(dict(noise_pred_uncond=e_unc, noise_cfg=cfg16, noise_pred_text=e_txt, guidance_rescale=phi,
                                       out_fp64=pm.rescale_noise_cfg(cfg16.double(), e_txt.double(), guidance_rescale=phi),
                                       out_fp16=pm.rescale_noise_cfg(cfg16, e_txt, guidance_rescale=phi)))
    name, mod, gd = _seine_diffusion()
    try:
        sched = DDIMScheduler()
        sched.set_timesteps(50)
        ts = sorted(int(t) for t in sched.timesteps)
        diff = mod.SpacedDiffusion(use_timesteps=ts, betas=sched.betas.double().numpy(), model_mean_type=gd.ModelMeanType.START_X,
                                   model_var_type=gd.ModelVarType.FIXED_SMALL, loss_type=gd.LossType.MSE)
        g = torch.Generator().manual_seed(7)
        x = torch.randn(2, 4, 3, 5, 5, generator=g, dtype=torch.float64)
        v = torch.randn(2, 4, 3, 5, 5, generator=g, dtype=torch.float64)
        for i in STEP_INDICES:
            t = ts[i]
            a_t = float(sched.alphas_cumprod[t])
            a_p = float(sched.alphas_cumprod[ts[i - 1]]) if i else 1.0
            x0 = a_t ** 0.5 * x - (1 - a_t) ** 0.5 * v       # v-prediction -> x0 (consisti2v/ddim_inverse_scheduler.py:350-352)
            torch.manual_seed(40 + i)                         # ddim_sample draws ``randn_like(x)`` from the global generator
            ref = diff.ddim_sample(lambda xx, tt: x0, x, torch.tensor([i, i]), clip_denoised=False, eta=ETA)["sample"]
            torch.manual_seed(40 + i)
            noise = torch.randn_like(x)
            out["ddim"].append(dict(index=i, timestep=t, alpha_t=a_t, alpha_prev=a_p, x=x, v=v, noise=noise, nonzero=bool(i), sample=ref))
    finally:
        for k in [k for k in sys.modules if k.startswith(name)]:
            del sys.modules[k]
    return out


if __name__ == "__main__":
    torch.save(build(), sys.argv[1] if len(sys.argv) > 1 else OUT)
