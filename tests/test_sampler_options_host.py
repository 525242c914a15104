"""Stochastic DDIM (``eta``) and guidance rescale in the I2VGen-XL step engines, without a GPU: the fp64 definitions against what the
reference's own code returned (tests/sampler_options_spec.py, tests/golden/sampler_options_ref.pt), the coefficient rows, the refusals,
the C ABI's host-side validation, and the mini pipeline under the CPU op emulation (tests/cpu_sampler_emulation.py) against the spec loop."""
import ctypes
import math
import os
import re
import types

import pytest
import torch

import cpu_sampler_emulation as semu
import gpu_checks as gc
import sampler_options_spec as spec
from oracle import ref_stubs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "sampler_options_ref.pt")
ETA, PHI = 0.5, 0.7
FR, HW_, STEPS = 2, 8, 4


@pytest.fixture()
def cpu_ops(monkeypatch):
    semu.install(monkeypatch)
    monkeypatch.setattr(gc, "DEV", "cpu")
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "1")
    yield


# ------------------------------------------------------------------------------------------------ definitions vs the reference
def test_spec_against_the_references_own_results():
    """rescale_noise_cfg: the fp64 restatement equals the reference's fp64 result to 1e-12 (relative to the largest value), and the
    reference's own fp16 result lies within the kernels' KTOL of it; ddim_sample(eta = 0.5): within rtol 2e-4 / atol 2e-5, the bound of
    the other tests pinned to that file (its ``_extract_into_tensor`` rounds every coefficient to fp32, and ``_predict_eps_from_xstart``
    divides by sqrt(1 / abar - 1), 7e-3 at t = 1)."""
    fx = torch.load(GOLDEN)
    assert fx["eta"] == ETA and len(fx["rescale"]) == 6 and len(fx["ddim"]) == 5
    for r in fx["rescale"]:
        got = spec.rescale_noise_cfg(r["noise_cfg"], r["noise_pred_text"], r["guidance_rescale"])
        scale = float(r["out_fp64"].abs().max())
        assert float((got - r["out_fp64"]).abs().max()) <= 1e-12 * scale
        d16 = float((r["out_fp16"].double() - got).abs().max()) / scale
        ulps = spec.ulp_distance_fp16(r["out_fp16"], got.half())
        print(f"[sampler] rescale phi={r['guidance_rescale']} {tuple(got.shape)}: reference fp16 vs fp64 definition {d16:.2e} of max, {ulps} fp16 ulp")
        assert d16 <= gc.KTOL
        if r["guidance_rescale"] == 0.0:
            assert torch.equal(got, r["noise_cfg"].double())
    for d in fx["ddim"]:
        row = spec.eta_row(d["alpha_t"], d["alpha_prev"], fx["eta"])
        got = spec.ddim_eta_step(d["v"], d["x"], row, d["noise"] if d["nonzero"] else None, spec.PRED_V)
        assert torch.allclose(got, d["sample"], rtol=2e-4, atol=2e-5), d["timestep"]
        assert row[4] > 0 or d["alpha_prev"] == 1.0
        moved = float((got - spec.ddim_eta_step(d["v"], d["x"], spec.eta_row(d["alpha_t"], d["alpha_prev"], 0.0))).abs().max())
        assert moved > 1e-2 or not d["nonzero"] or row[4] < 1e-3, "eta does not move this step: the comparison would say nothing"


@pytest.mark.skipif(not ref_stubs.reference_available(), reason="needs the reference tree")
def test_fixture_is_what_the_reference_returns_today():
    """Re-runs tests/golden/make_sampler_golden.py live: the committed file is bit for bit what the reference's code returns."""
    import importlib.util
    s = importlib.util.spec_from_file_location("make_sampler_golden", os.path.join(ROOT, "tests", "golden", "make_sampler_golden.py"))
    mod = importlib.util.module_from_spec(s)
    s.loader.exec_module(mod)
    live, fx = mod.build(), torch.load(GOLDEN)
    assert live.keys() == fx.keys() and live["eta"] == fx["eta"] and live["guidance"] == fx["guidance"]
    for name in ("rescale", "ddim"):
        assert len(live[name]) == len(fx[name])
        for a, b in zip(live[name], fx[name]):
            assert a.keys() == b.keys()
            for k in a:
                assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], (name, k)


# ------------------------------------------------------------------------------------------------ coefficient rows
def test_coefficient_rows():
    from anyv2v_amd.schedulers import DDIMInverseScheduler, DDIMScheduler
    sched = DDIMScheduler()
    sched.set_timesteps(50)
    ts = [int(t) for t in sched.timesteps]
    base = sched.coefficient_table(ts, "cpu")
    assert tuple(base.shape) == (50, 4)
    assert torch.equal(base, torch.tensor([sched.coefficients(t) for t in ts], dtype=torch.float32))      # today's table
    for off in (dict(), dict(eta=None), dict(eta=0.0), dict(eta=0, phi=0.0, n=123)):
        assert torch.equal(sched.coefficient_table(ts, "cpu", **off), base), off
    n = 4 * 16 * 64 * 64
    tab = sched.coefficient_table(ts, "cpu", eta=ETA, phi=PHI, n=n)
    assert tuple(tab.shape) == (50, 8) and tab.dtype == torch.float32
    for i, t in enumerate(ts):
        a_t, a_p = float(sched.alphas_cumprod[t]), (float(sched.alphas_cumprod[t - 20]) if t - 20 >= 0 else 1.0)
        want = torch.tensor(spec.eta_row(a_t, a_p, ETA, PHI, n), dtype=torch.float64)
        assert float((tab[i].double() - want)[:6].abs().max()) <= 1e-6, t      # (fp32 rows of fp64 coefficients <= 1)
        assert float(tab[i, 6]) == n and float(tab[i, 7]) == 0.0
    assert float(tab[-1, 4]) == 0.0                       # the last step's alpha_prev is 1: no noise is added
    # rescale alone: the deterministic coefficients, bit for bit, in columns 0-3
    only_phi = sched.coefficient_table(ts, "cpu", phi=PHI, n=n)
    assert torch.equal(only_phi[:, :4], base) and float(only_phi[:, 4].abs().max()) == 0.0
    # the first timestep under zero terminal SNR: a_t = 0 exactly -> finite row, sa_t = 0, sb_t = 1
    assert float(sched.alphas_cumprod[999]) == 0.0
    row = sched.coefficient_table([999], "cpu", eta=ETA, phi=PHI, n=n)[0]
    assert torch.isfinite(row).all() and float(row[0]) == 0.0 and float(row[1]) == 1.0 and float(row[4]) > 0
    want = spec.eta_row(0.0, float(sched.alphas_cumprod[979]), ETA, PHI, n)
    assert float((row.double() - torch.tensor(want, dtype=torch.float64))[:5].abs().max()) <= 1e-6
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="0 <= eta <= 1"):
            sched.coefficient_table(ts, "cpu", eta=bad)
        with pytest.raises(ValueError, match="guidance_rescale"):
            sched.coefficient_table(ts, "cpu", phi=bad, n=n)
    with pytest.raises(ValueError, match="n >= 2"):
        sched.coefficient_table(ts, "cpu", phi=PHI, n=1)
    eps_sched = DDIMScheduler(prediction_type="epsilon")
    eps_sched.set_timesteps(50)
    with pytest.raises(ValueError, match="singular"):
        eps_sched.coefficient_table([999], "cpu", eta=ETA)
    inv = DDIMInverseScheduler()
    inv.set_timesteps(50)
    with pytest.raises(NotImplementedError, match="forward DDIM"):
        inv.coefficient_table([1, 21], "cpu", eta=ETA)
    assert tuple(inv.coefficient_table([1, 21], "cpu").shape) == (2, 4)


# ------------------------------------------------------------------------------------------------ refusals
def test_every_refused_option_raises_with_its_message():
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMInverseScheduler, DDIMScheduler
    from anyv2v_amd.unet import I2VGenXLUNet, I2VGenXLUNetConfig
    with torch.device("meta"):
        unet = I2VGenXLUNet(I2VGenXLUNetConfig.mini())
    pipe = I2VGenXLPipeline(unet=unet, scheduler=DDIMScheduler())
    assert pipe._sampler_options(None, None) == (False, 0.0, 0.0) and pipe._sampler_options(0.0, {}) == (False, 0.0, 0.0)
    assert pipe._sampler_options(ETA, None) == (True, ETA, 0.0)
    for bad in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="0 <= eta <= 1"):
            pipe._sampler_options(bad, None)
        with pytest.raises(ValueError, match="0 <= guidance_rescale <= 1"):
            pipe.enable_guidance_rescale(bad)
    with pytest.raises(ValueError, match="cross_attention_kwargs"):
        pipe._sampler_options(ETA, {"scale": 0.5})
    pipe.enable_guidance_rescale(PHI)
    assert pipe._sampler_options(ETA, None) == (True, ETA, PHI) and pipe._sampler_options(0.0, None) == (False, 0.0, PHI)
    assert pipe.sibling()._guidance_rescale == PHI
    # frame-parallel clips: both options refused, as FreeU is
    unet.frame_parallel = object()
    with pytest.raises(NotImplementedError, match="frame-parallel"):
        pipe._sampler_options(0.0, None)               # (the rescale is still on)
    pipe.disable_guidance_rescale()
    assert pipe._sampler_options(0.0, None) == (False, 0.0, 0.0)
    with pytest.raises(NotImplementedError, match="frame-parallel"):
        pipe._sampler_options(ETA, None)
    with pytest.raises(NotImplementedError, match="frame-parallel"):
        pipe.enable_guidance_rescale(PHI)
    pipe.enable_guidance_rescale(0.0)
    unet.frame_parallel = None
    # the inverse scheduler's step takes no eta: dropped, as in the reference; it has no rescale path
    pipe.scheduler = DDIMInverseScheduler()
    assert pipe._sampler_options(ETA, None) == (False, 0.0, 0.0)
    pipe.enable_guidance_rescale(PHI)
    with pytest.raises(NotImplementedError, match="forward DDIM"):
        pipe._sampler_options(0.0, None)
    # a stochastic engine that is not handed this step's noise refuses to replay the last draw
    from anyv2v_amd.pipeline import _StepEngine
    eng = _StepEngine.__new__(_StepEngine)
    eng.stochastic, eng.ctx, eng.coef = True, types.SimpleNamespace(t_buf=torch.zeros(1)), torch.zeros(8)
    with pytest.raises(ValueError, match="variance noise"):
        eng._step(torch.zeros(1), torch.zeros(8), ("k",))


def test_abi_validation_without_gpu():
    """Host-side validation returns ANYV2V_EINVAL (-1) with a message before anything touches a device."""
    from anyv2v_amd import _lib
    lib = _lib.load()
    P = 4096   # any 16-byte-aligned non-null address: nothing is dereferenced before the checks
    good = dict(V=P, ldv=8, b_unc=0, b_cond=1, g=9.0, rec=2 * P, C=4, F=2, HW=64)

    def stats(**over):
        a = dict(good, **over)
        return lib.anyv2v_guidance_stats_f16(a["V"], a["ldv"], a["b_unc"], a["b_cond"], a["g"], a["rec"], a["C"], a["F"], a["HW"], None)

    for name in ("V", "rec"):
        assert stats(**{name: None}) == -1 and b"null pointer" in lib.anyv2v_last_error()
    for over in (dict(b_unc=-1), dict(b_cond=-1), dict(C=0), dict(F=0), dict(HW=0), dict(ldv=3)):
        assert stats(**over) == -1 and b"bad arguments" in lib.anyv2v_last_error(), over
    assert stats(C=1, F=1, HW=1) == -1 and b"n >= 2" in lib.anyv2v_last_error()
    assert stats(rec=2 * P + 4) == -1 and b"16-byte" in lib.anyv2v_last_error()
    assert stats(F=1 << 16, HW=1 << 16) == -1 and b"fit an int" in lib.anyv2v_last_error()
    good2 = dict(V=P, ldv=8, b_unc=0, b_cond=1, g=9.0, pred=0, row=2 * P, rec=3 * P, phi=0.7, noise=4 * P, lat=5 * P, out=5 * P, C=4, F=2, HW=64)

    def step(**over):
        a = dict(good2, **over)
        return lib.anyv2v_cfg_ddim_step_ex_f16(a["V"], a["ldv"], a["b_unc"], a["b_cond"], a["g"], a["pred"], a["row"], a["rec"], a["phi"],
                                               a["noise"], a["lat"], a["out"], a["C"], a["F"], a["HW"], None)

    for name in ("V", "row", "lat", "out", "rec"):
        assert step(**{name: None}) == -1 and b"null pointer" in lib.anyv2v_last_error(), name
    for phi in (-0.1, 1.5, float("nan")):
        assert step(phi=phi) == -1 and b"[0, 1]" in lib.anyv2v_last_error(), phi
    assert step(C=1, F=1, HW=1) == -1 and b"n >= 2" in lib.anyv2v_last_error()
    for over in (dict(pred=3), dict(pred=-1), dict(b_cond=-1), dict(ldv=3), dict(C=0)):
        assert step(**over) == -1 and b"bad arguments" in lib.anyv2v_last_error(), over
    assert step(rec=3 * P + 4) == -1 and b"16-byte" in lib.anyv2v_last_error()


def test_header_binding_and_abi_version():
    """Both entry points are declared with the reference lines they replace, bound and exported; the grid constants agree; the ABI
    version did not move (no structure changed)."""
    from anyv2v_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "anyv2v_hip.h")).read()
    for sym, nargs in (("anyv2v_guidance_stats_f16", 10), ("anyv2v_cfg_ddim_step_ex_f16", 16)):
        assert re.search(r"\b%s\s*\(" % sym, hdr)
        assert sym in _lib.SYMBOLS and len(_lib.SYMBOLS[sym][1]) == nargs
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), sym)
    assert "pipeline_video_editing.py:50-61" in hdr and "gaussian_diffusion.py:583-599" in hdr and "pipeline_i2vgen_xl.py:868,1173" in hdr
    consts = {k: int(v) for k, v in re.findall(r"#define ANYV2V_GUIDANCE_STATS_(\w+) (\d+)", hdr)}
    assert consts == dict(BLOCKS=_lib.GUIDANCE_STATS_BLOCKS, THREADS=_lib.GUIDANCE_STATS_THREADS, RECORD=_lib.GUIDANCE_STATS_RECORD)
    assert ops.GUIDANCE_STATS_FLOATS == consts["BLOCKS"] * consts["RECORD"] == semu.BLOCKS * semu.RECORD
    assert _lib.ABI_VERSION == 105 and "#define ANYV2V_ABI_VERSION 105" in hdr


# ------------------------------------------------------------------------------------------------ emulation vs the definition
@pytest.mark.parametrize("pred", [0, 1, 2])
def test_emulated_ops_against_the_definition(pred):
    """The torch emulation the pipeline tests below run on, against the fp64 definition: KTOL, as the kernels."""
    shape = (1, 4, 3, 5, 7)
    g = torch.Generator().manual_seed(3 + pred)
    n = shape[2] * shape[3] * shape[4]
    vtok = (torch.randn(3 * n, 8, generator=g) + 0.25).half()
    lat, noise = torch.randn(shape, generator=g).half(), torch.randn(shape, generator=g).half()
    row = torch.tensor((0.8, 0.6, 0.9, 0.3, 0.25, PHI, 4 * n, 0.0), dtype=torch.float32)
    for b_unc, phi in ((1, PHI), (1, 0.0), (-1, PHI)):
        row[5] = phi
        stats = semu.guidance_stats(vtok, b_unc, 2, 9.0, shape) if (phi > 0 and b_unc >= 0) else None
        out = torch.empty(shape, dtype=torch.float16)
        semu.cfg_ddim_step_ex(vtok, b_unc, 2, 9.0, row, lat, out, prediction=pred, stats=stats, phi=phi if stats is not None else 0.0, noise=noise)
        ref = spec.fused_step(vtok, b_unc, 2, 9.0, [float(c) for c in row], lat, noise, pred)
        r = gc._res(f"emulated step pred {pred} b_unc {b_unc} phi {phi}", out, ref, gc.KTOL)
        assert r["ok"], r


# ------------------------------------------------------------------------------------------------ mini pipeline on the CPU
def _clip():
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMInverseScheduler
    native, _, ocfg = gc.build_pair("mini", 1234)
    inp = gc.config1_inputs(ocfg, 3, FR, HW_)
    h = lambda x: x.half()
    c = types.SimpleNamespace(native=native, lat0=h(inp["sample"][:1]), ehs=h(inp["encoder_hidden_states"]), ie=h(inp["image_embeddings"]),
                              il=h(inp["image_latents"]))
    pipe = I2VGenXLPipeline(unet=native, scheduler=DDIMInverseScheduler())
    c.traj = pipe.invert(prompt_embeds=c.ehs[:1], image_embeddings=c.ie[:1], image_latents=c.il[:1], height=HW_ * 8, width=HW_ * 8,
                         num_frames=FR, num_inference_steps=STEPS, guidance_scale=1.0, target_fps=8, latents=c.lat0, return_trajectory=True)
    c.T = max(c.traj.keys())
    return c


def _pipe(c):
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMScheduler
    return I2VGenXLPipeline(unet=c.native, scheduler=DDIMScheduler())


def _sample(pipe, c, eta=0.0, seed=0):
    return pipe(prompt_embeds=c.ehs[2:3], negative_prompt_embeds=c.ehs[1:2], image_embeddings=c.ie[2:3], image_latents=c.il[2:3],
                height=HW_ * 8, width=HW_ * 8, num_frames=FR, num_inference_steps=STEPS, guidance_scale=9.0, target_fps=8, eta=eta,
                generator=torch.Generator().manual_seed(seed), latents=c.traj[c.T].clone(), output_type="latent",
                ddim_init_latents_t_idx=0).frames.clone()


def _register(pipe, ratios=(0.5, 0.75, 1.0)):
    from anyv2v_amd import pnp_utils
    from anyv2v_amd.schedulers import DDIMScheduler
    sched = DDIMScheduler()
    sched.set_timesteps(STEPS)
    pipe.register_modules(scheduler=sched)
    k = lambda r: sched.timesteps[: int(STEPS * r)]
    pnp_utils.register_conv_injection(pipe, k(ratios[0]))
    pnp_utils.register_spatial_attention_pnp(pipe, k(ratios[1]))
    pnp_utils.register_temp_attention_pnp(pipe, k(ratios[2]))
    return sched


def _edit(pipe, c, eta=0.0, seed=0):
    from anyv2v_amd import pnp_utils
    _register(pipe)
    try:
        return pipe.sample_with_pnp(prompt_embeds=c.ehs[2:3], negative_prompt_embeds=c.ehs[1:2], image_embeddings=c.ie[2:3],
                                    image_latents=c.il[2:3], height=HW_ * 8, width=HW_ * 8, num_frames=FR, num_inference_steps=STEPS,
                                    guidance_scale=9.0, target_fps=8, eta=eta, generator=torch.Generator().manual_seed(seed),
                                    latents=c.traj[c.T].clone(), output_type="latent", ddim_init_latents_t_idx=0, ddim_inv_latents_path=c.traj,
                                    ddim_inv_prompt_embeds=c.ehs[:1], ddim_inv_image_embeddings=c.ie[:1],
                                    ddim_inv_image_latents=c.il[:1]).frames.clone()
    finally:
        pnp_utils.clear_time(pipe)


def _spec_loop(c, eta, phi, seed, pnp):
    """The loop by the definitions: the native UNet's prediction of every branch (whole batch, no step engine), the fp16 guidance, the
    fp64 rescale and step, the noise drawn as ``randn_tensor`` draws it from a CPU generator (fp32, then cast), fp16 latents between
    the steps as in the reference's loop."""
    from anyv2v_amd import pnp_utils
    from anyv2v_amd.schedulers import DDIMScheduler
    holder = types.SimpleNamespace(unet=c.native, register_modules=lambda **kw: None)
    sched = _register(holder) if pnp else DDIMScheduler()
    sched.set_timesteps(STEPS)
    gen = torch.Generator().manual_seed(seed)
    lat = c.traj[c.T].clone()
    b0 = 0 if pnp else 1
    kw = dict(fps=torch.tensor([8] * (3 - b0)), encoder_hidden_states=c.ehs[b0:],
              image_embeddings=torch.cat([c.ie[:1]] * (1 - b0) + [torch.zeros_like(c.ie[:1]), c.ie[2:3]]),
              image_latents=torch.cat([c.il[:1]] * (1 - b0) + [c.il[2:3], c.il[2:3]]))
    try:
        for t in [int(t) for t in sched.timesteps]:
            if pnp:
                pnp_utils.register_time(holder, t)
            smp = torch.cat(([c.traj[t]] if pnp else []) + [lat, lat])
            v = c.native(smp, t, **kw)[0]
            e_unc, e_txt = v[-2:-1].half(), v[-1:].half()
            g = spec.guided_fp16(e_unc, e_txt, 9.0)
            if phi > 0:
                g = spec.rescale_noise_cfg(g, e_txt, phi)
            noise = torch.randn(lat.shape, generator=gen, dtype=torch.float32).half() if eta > 0 else None
            a_t, a_p = float(sched.alphas_cumprod[t]), sched._abar(t - sched._ratio())
            lat = spec.ddim_eta_step(g, lat, spec.eta_row(a_t, a_p, eta), noise).half()
    finally:
        if pnp:
            pnp_utils.clear_time(holder)
    return lat


LOOP_TOL = 1e-2   # the emulated step computes in fp32 what the definition computes in fp64: an fp16 rounding of a latent may flip
                  # (2^-10 of the value), and three more UNet forwards see it; both loops run the same UNet on the same op emulation


@pytest.mark.parametrize("loop", ["__call__", "sample_with_pnp"])
def test_mini_pipeline_with_eta_and_rescale_against_the_spec_loop(cpu_ops, loop):
    """``eta = 0.5`` after ``enable_guidance_rescale(0.7)``: against the spec loop; the same seed twice gives the same bits, another
    seed other bits; each option alone and both together move the sample by far more than the bound; both off afterwards is bit-equal
    to never on, on an engine with today's cache key."""
    run = _sample if loop == "__call__" else _edit
    c = _clip()
    pipe = _pipe(c)
    off = run(pipe, c)
    key_off = [k for k in pipe._engines if k[0] in ("cfg", "pnp", "pnp-droptail")]
    pipe.enable_guidance_rescale(PHI)
    on = run(pipe, c, eta=ETA, seed=11)
    key_on = [k for k in pipe._engines if k[0] in ("cfg", "pnp", "pnp-droptail")]
    assert len(key_off) == len(key_on) == 1 and key_on[0][:-1] == key_off[0] and key_on[0][-1] == ("sampler", True, PHI)
    assert not any(isinstance(x, tuple) and x and x[0] == "sampler" for x in key_off[0])        # today's key
    ref = _spec_loop(c, ETA, PHI, 11, pnp=loop != "__call__")
    r = gc._res(f"{loop} eta {ETA} rescale {PHI} vs the spec loop", on, ref, LOOP_TOL)
    moved = gc._rel(on, off.float())
    print(f"[sampler] {loop}: vs spec loop max {r['err']:.3e} l2 {r['l2']:.3e} (tol {LOOP_TOL}); options on vs off max {moved[0]:.3e} l2 {moved[1]:.3e}")
    assert r["ok"], r
    assert moved[0] > 10 * LOOP_TOL and moved[1] > 10 * LOOP_TOL, "the options do not move the sample: the comparison above would be vacuous"
    assert torch.equal(run(pipe, c, eta=ETA, seed=11), on), "same seed, other bits"
    other = run(pipe, c, eta=ETA, seed=12)
    assert not torch.equal(other, on) and gc._rel(other, on.float())[1] > 10 * LOOP_TOL, "another seed, the same sample"
    only_phi = run(pipe, c)
    r_phi = gc._res(f"{loop} rescale alone vs the spec loop", only_phi, _spec_loop(c, 0.0, PHI, 0, pnp=loop != "__call__"), LOOP_TOL)
    assert r_phi["ok"], r_phi
    assert gc._rel(only_phi, off.float())[1] > 10 * LOOP_TOL and gc._rel(only_phi, on.float())[1] > 10 * LOOP_TOL
    pipe.disable_guidance_rescale()
    assert torch.equal(run(pipe, c), off), "both options off again: not bit-equal to never on"
    assert [k for k in pipe._engines if k[0] in ("cfg", "pnp", "pnp-droptail")] == key_off


def test_variance_noise_is_drawn_once_per_step_outside_the_engine(cpu_ops, monkeypatch):
    """One draw per step from the caller's generator, with the shape and dtype of the guided prediction; consecutive steps get
    different noise (a buffer filled once would replay the first); eta = 0 draws nothing; ``invert`` drops eta."""
    from anyv2v_amd.schedulers import DDIMScheduler
    c = _clip()
    pipe = _pipe(c)
    draws = []
    inner = DDIMScheduler.draw_noise
    monkeypatch.setattr(DDIMScheduler, "draw_noise", lambda self, like, generator=None: (draws.append(inner(self, like, generator)), draws[-1])[1])
    _sample(pipe, c, eta=0.0)
    _edit(pipe, c, eta=0.0)
    assert draws == []
    gen_state = torch.Generator().manual_seed(5)
    want = [torch.randn(c.lat0.shape, generator=gen_state, dtype=torch.float32).half() for _ in range(STEPS)]
    for run in (_sample, _edit):
        draws.clear()
        run(pipe, c, eta=ETA, seed=5)
        assert len(draws) == STEPS and all(d.shape == c.lat0.shape and d.dtype == torch.float16 for d in draws)
        assert all(torch.equal(d, w) for d, w in zip(draws, want)) and not torch.equal(draws[0], draws[1])


def test_source_cache_stays_valid_under_both_options(cpu_ops):
    """Multi-edit job: what the cache records is the source branch's features, fed from the trajectory -- the same whatever the edit's
    eta / rescale.  Recorded by a default edit, replayed by an edit with both options on; and recorded under the options: the same
    features, bit for bit.  The recording (three-branch) edit is bit-equal to the uncached one; a REPLAYED edit is bit-equal on the GPU
    only (tests/test_sampler_options_gpu.py) -- torch's CPU matmul picks its summation order by shape, so here it agrees to the "fp16
    drift" bound of ``gpu_checks.check_source_cache`` (0.12; a wrong or stale feature at any site is an O(1) error)."""
    c = _clip()
    want_off = _edit(_pipe(c), c)
    fresh = _pipe(c)
    fresh.enable_guidance_rescale(PHI)
    fresh_cache = fresh.enable_source_cache(True)
    want_on = _edit(fresh, c, eta=ETA, seed=3)               # records under both options
    plain = _pipe(c)
    plain.enable_guidance_rescale(PHI)
    assert torch.equal(want_on, _edit(plain, c, eta=ETA, seed=3)), "recording edit under eta + rescale differs from the uncached one"
    pipe = _pipe(c)
    cache = pipe.enable_source_cache(True)
    assert torch.equal(_edit(pipe, c), want_off) and cache.recorded_steps > 0 and cache.replayed_steps == 0
    recorded = {k: {n: v.clone() for n, v in d.items()} for k, d in cache.steps.items()}
    assert recorded.keys() == fresh_cache.steps.keys()
    assert all(torch.equal(fresh_cache.steps[k][n], v) for k, d in recorded.items() for n, v in d.items()), "the source features depend on the options"
    pipe.enable_guidance_rescale(PHI)
    got = _edit(pipe, c, eta=ETA, seed=3)
    assert cache.replayed_steps > 0 and cache.signature is not None, "the options dropped the cache"
    r = gc._res("replayed edit under eta + rescale vs the uncached one (CPU emulation: fp16 drift)", got, want_on.float(), 0.12)
    print(f"[sampler] source cache replay under both options: max {r['err']:.3e} l2 {r['l2']:.3e}")
    assert r["ok"], r
    assert cache.steps.keys() == recorded.keys() and all(torch.equal(cache.steps[k][n], v) for k, d in recorded.items() for n, v in d.items())


# ------------------------------------------------------------------------------------------------ configuration keys
def test_config_keys_reach_the_call(tmp_path, monkeypatch):
    """``eta`` / ``guidance_rescale`` in the template or the JSON entry reach ``sample_with_pnp`` / ``enable_guidance_rescale`` through
    ``Stage2``; absent, the call and the output directory are the ones of a job without the keys."""
    import logging

    import numpy as np
    from PIL import Image

    from anyv2v_amd.config import OmegaConf, sampler_options
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.run_group_pnp_edit import Stage2, output_suffix
    from anyv2v_amd.schedulers import DDIMScheduler
    from anyv2v_amd.unet import I2VGenXLUNet, I2VGenXLUNetConfig
    from anyv2v_amd.utils import LatentTrajectory
    tmpl = OmegaConf.load(os.path.join(ROOT, "configs", "group_pnp_edit", "template.yaml"))
    assert "eta" not in tmpl and "guidance_rescale" not in tmpl and sampler_options(tmpl) == (0.0, 0.0)
    entry = {"active": True, "task_name": "T", "video_name": "clip", "edited_first_frame_path": "demo/clip/e.png", "editing_prompt": "a robot",
             "edited_video_name": "robot"}
    plain = OmegaConf.merge(tmpl, OmegaConf.create(entry))
    assert output_suffix(plain, 1) == "ddim_init_latents_t_idx_1_nsteps_50_cfg_9.0_pnpf0.2_pnps0.2_pnpt0.5"
    both = OmegaConf.merge(tmpl, OmegaConf.create(dict(entry, eta=ETA, guidance_rescale=PHI)))
    assert sampler_options(both) == (ETA, PHI) and output_suffix(both, 1).endswith("_pnpt0.5_eta0.5_rescale0.7")
    for bad in (dict(eta=1.5), dict(guidance_rescale=-0.2)):
        with pytest.raises(ValueError, match="0 <="):
            sampler_options(OmegaConf.merge(tmpl, OmegaConf.create(bad)))
    # through the runner: frames on disk, a trajectory in memory, the pipeline's call recorded and stopped
    clip = tmp_path / "demo" / "clip"
    clip.mkdir(parents=True)
    for i in range(2):
        Image.fromarray(np.full((64, 64, 3), 40 * i, dtype=np.uint8)).save(clip / f"{i:05d}.png")
    Image.fromarray(np.full((64, 64, 3), 99, dtype=np.uint8)).save(clip / "e.png")
    tmpl.data_dir, tmpl.device, tmpl.image_size, tmpl.n_frames, tmpl.n_steps = str(tmp_path), "cpu", [64, 64], 2, 4
    with torch.device("meta"):
        unet = I2VGenXLUNet(I2VGenXLUNetConfig.mini())
    pipe = I2VGenXLPipeline(unet=unet, scheduler=DDIMScheduler())
    seen = []

    class Stop(Exception):
        pass

    def fake(**kw):
        seen.append((kw.get("eta"), pipe._guidance_rescale))
        raise Stop
    monkeypatch.setattr(pipe, "sample_with_pnp", fake)
    monkeypatch.setattr(pipe, "auto_vae_tiling", lambda *a: None)
    sched = DDIMScheduler()
    sched.set_timesteps(4)
    traj = LatentTrajectory()
    for t in sched.timesteps.tolist():
        traj[int(t)] = torch.zeros(1, 4, 2, 8, 8, dtype=torch.float16)
    lat_dir = os.path.abspath(str(OmegaConf.merge(tmpl, OmegaConf.create(entry)).ddim_latents_path))
    entries = [dict(entry), dict(entry, eta=ETA, guidance_rescale=PHI), dict(entry, eta=0.25), dict(entry)]
    stage = Stage2(tmpl, entries, torch.device("cpu"), logging.getLogger("sampler-options"), pipe=pipe, trajectories={lat_dir: traj})
    for e in entries:
        with pytest.raises(Stop):
            stage.run_entry(e)
    assert seen == [(0.0, 0.0), (ETA, PHI), (0.25, 0.0), (0.0, 0.0)]
