"""Masked PnP editing without a GPU: the torch emulation of the two ops (tests/cpu_masked_edit_emulation.py) against the fp64 definition
(tests/masked_edit_spec.py), the feather's tap table, every refusal, the C ABI's host-side validation, the bindings, the mini pipeline
under the op emulation against the spec loop, the partner of every step, and the configuration keys through the runner."""
import ctypes
import os
import re
import types

import pytest
import torch

import cpu_masked_edit_emulation as memu
import gpu_checks as gc
import masked_edit_spec as spec
from sampler_options_spec import ulp_distance_fp16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FR, HW_, STEPS = 2, 8, 4
PARAMS = [(0, 0.0), (1, 0.0), (8, 0.0), (0, 0.5), (2, 1.5), (0, 8.0)]


@pytest.fixture()
def cpu_ops(monkeypatch):
    memu.install(monkeypatch)
    monkeypatch.setattr(gc, "DEV", "cpu")
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "1")
    yield


def _masks(Fm, H, W, seed=0):
    """A binary mask aligned to the 8 x 8 blocks, a binary mask that is not, a random soft mask: fp16 [Fm, H, W]."""
    g = torch.Generator().manual_seed(100 * Fm + H + W + seed)
    aligned = torch.zeros(Fm, H, W)
    aligned[:, : max(8, H // 16 * 8), : max(8, W // 16 * 8)] = 1.0
    ragged = torch.zeros(Fm, H, W)
    for f in range(Fm):
        ragged[f, 1 + f: max(3, H // 2 + 3), 2: max(5, W // 2 + 5 - f)] = 1.0
    soft = torch.rand(Fm, H, W, generator=g)
    return {"aligned": aligned.half(), "ragged": ragged.half(), "soft": soft.half()}


# ------------------------------------------------------------------------------------------------ emulation vs the definition
@pytest.mark.parametrize("grow,sigma", PARAMS)
def test_emulated_latent_mask_against_the_definition(grow, sigma):
    for Fm, H, W in ((1, 8, 8), (3, 40, 24)):
        for name, m in _masks(Fm, H, W).items():
            want = spec.latent_mask(m, grow, sigma).half()
            got = memu.latent_mask(m, grow, sigma)
            assert got.dtype == torch.float16 and tuple(got.shape) == (Fm, H // 8, W // 8)
            if sigma == 0:
                assert torch.equal(got, want), (name, Fm, H, W)
            else:
                assert ulp_distance_fp16(got, want) <= 1, (name, Fm, H, W)
            assert float(got.min()) >= 0.0 and float(got.max()) <= 1.0
    # a binary mask pools to k / 64 exactly; an all-ones / all-zeros mask stays exactly 1 / 0 through every stage (the taps sum to 1
    # within fp32 rounding, so the feather of a constant 1 is checked to the last fp16 bit)
    m = _masks(1, 16, 16)["ragged"]
    k = m.float().view(1, 2, 8, 2, 8).sum(dim=(2, 4))
    assert torch.equal(spec.latent_mask(m).half(), (k / 64).half())
    for const in (0.0, 1.0):
        c = torch.full((1, 16, 24), const).half()
        assert torch.equal(spec.latent_mask(c, grow, sigma).half(), torch.full((1, 2, 3), const).half())
        assert torch.equal(memu.latent_mask(c, grow, sigma), torch.full((1, 2, 3), const).half())


def test_emulated_blend_against_the_definition_and_the_selects():
    g = torch.Generator().manual_seed(7)
    for F, Fm, h, w in ((1, 1, 5, 5), (3, 3, 8, 8), (3, 1, 3, 16), (3, 3, 9, 7)):
        x, s = torch.randn(1, 4, F, h, w, generator=g).half(), torch.randn(1, 4, F, h, w, generator=g).half()
        m = torch.rand(Fm, h, w, generator=g).half()
        m.view(-1)[::3], m.view(-1)[1::3] = 0.0, 1.0
        want = spec.blend(x, s, m)
        assert torch.equal(memu.masked_blend(x, s, m), want)
        mm = m[None, None].expand(x.shape)
        assert torch.equal(want[mm == 0], s[mm == 0]) and torch.equal(want[mm == 1], x[mm == 1])
        # the dropped operand may hold anything: Inf / NaN in x where m == 0, in s where m == 1
        xp, sp = x.clone(), s.clone()
        xp[mm == 0] = torch.tensor([float("inf"), float("nan")]).half().repeat(int((mm == 0).sum() + 1) // 2)[: int((mm == 0).sum())]
        sp[mm == 1] = float("nan")
        for fn in (spec.blend, memu.masked_blend):
            got = fn(xp, sp, m)
            assert torch.equal(got.view(torch.int16), want.view(torch.int16)), fn
        inplace = x.clone()
        assert memu.masked_blend(inplace, s, m, out=inplace) is inplace and torch.equal(inplace, want)


def test_tap_table():
    from anyv2v_amd import _lib, ops
    assert ops.gaussian_taps(0.0) == []
    for sigma in (0.1, 0.5, 1.0, 1.5, 2.7, 8.0):
        taps = ops.gaussian_taps(sigma)
        R = len(taps) // 2
        assert len(taps) == 2 * R + 1 and R == -(-3 * sigma // 1) and R <= _lib.MASK_MAX_RADIUS
        assert all(ctypes.c_float(t).value == t for t in taps), "not fp32 values"
        assert abs(sum(torch.tensor(taps, dtype=torch.float64)) - 1.0) <= 1e-7
        assert taps == taps[::-1] and taps[R] == max(taps)
        assert torch.equal(torch.tensor(taps, dtype=torch.float32), spec.gaussian_taps(sigma))
    for bad in (-0.5, 8.5, float("nan")):
        with pytest.raises(ValueError, match="0 <= feather <= 8"):
            ops.gaussian_taps(bad)


# ------------------------------------------------------------------------------------------------ refusals
def _meta_pipe():
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMScheduler
    from anyv2v_amd.unet import I2VGenXLUNet, I2VGenXLUNetConfig
    with torch.device("meta"):
        unet = I2VGenXLUNet(I2VGenXLUNetConfig.mini())
    return I2VGenXLPipeline(unet=unet, scheduler=DDIMScheduler()), unet


def test_every_refusal_raises_with_its_message():
    pipe, unet = _meta_pipe()
    mask, src = torch.ones(64, 64, dtype=torch.bool), torch.zeros(1, 4, 2, 8, 8, dtype=torch.float16)
    assert pipe._masked_edit is None and pipe._masked_edit_buffers(64, 64, 2, src) is None
    # accepted forms: [H, W] and [Fm, H, W]; bool, uint8 (255 = edit), float
    pipe.enable_masked_edit(mask, src)
    assert tuple(pipe._masked_edit["mask"].shape) == (1, 64, 64) and pipe._masked_edit["mask"].dtype == torch.float16
    assert float(pipe._masked_edit["mask"].min()) == 1.0 and (pipe._masked_edit["grow"], pipe._masked_edit["feather"]) == (0, 0.0)
    pipe.enable_masked_edit(torch.full((2, 64, 64), 255, dtype=torch.uint8), src, grow=8, feather=8.0)
    assert float(pipe._masked_edit["mask"].min()) == 1.0 and tuple(pipe._masked_edit["mask"].shape) == (2, 64, 64)
    pipe.enable_masked_edit(torch.rand(1, 64, 64), src, grow=2, feather=1.5)
    assert (pipe._masked_edit["grow"], pipe._masked_edit["feather"]) == (2, 1.5)
    assert pipe.sibling()._masked_edit is None, "the mask belongs to the clip: a sibling pipeline does not inherit it"
    # a mask set when __call__ / invert run
    for loop in (pipe, pipe.invert):
        with pytest.raises(ValueError, match="an edit mask is set"):
            loop(prompt_embeds=torch.zeros(1, 77, 8), height=64, width=64)
    with pytest.raises(ValueError, match="an edit mask is set"):
        pipe.invert_clips([], height=64, width=64)
    # a mask that does not match the call: H x W, Fm; source_latents that do not
    lat = torch.zeros(1, 4, 2, 8, 8, dtype=torch.float16)
    with pytest.raises(ValueError, match="does not match the call"):
        pipe._masked_edit_buffers(64, 128, 2, lat)
    pipe.enable_masked_edit(torch.ones(2, 64, 64), src)
    with pytest.raises(ValueError, match="does not match the call"):
        pipe._masked_edit_buffers(64, 64, 3, torch.zeros(1, 4, 3, 8, 8, dtype=torch.float16))
    pipe.enable_masked_edit(torch.ones(1, 64, 64), src)
    with pytest.raises(ValueError, match="source_latents .* do not match"):
        pipe._masked_edit_buffers(64, 64, 3, torch.zeros(1, 4, 3, 8, 8, dtype=torch.float16))
    pipe.disable_masked_edit()
    assert pipe._masked_edit is None
    # the setter's own checks; a refused call leaves the setting as it was (off)
    for bad_mask, msg in ((torch.ones(64), "tensor expected"), (torch.ones(1, 1, 64, 64), "tensor expected"), ([[1]], "tensor expected"),
                          (torch.ones(64, 64, dtype=torch.int32), "bool, uint8 or float"), (torch.full((64, 64), 1.5), r"\[0, 1\]"),
                          (torch.full((64, 64), float("nan")), r"\[0, 1\]"), (torch.ones(60, 64), "multiples of 8")):
        with pytest.raises(ValueError, match=msg):
            pipe.enable_masked_edit(bad_mask, src)
    for bad_src in (torch.zeros(1, 4, 2, 8, 4), torch.zeros(2, 4, 2, 8, 8), torch.zeros(1, 3, 2, 8, 8), torch.zeros(4, 2, 8, 8), None):
        with pytest.raises(ValueError, match="source_latents"):
            pipe.enable_masked_edit(mask, bad_src)
    with pytest.raises(ValueError, match="source_latents"):
        pipe.enable_masked_edit(torch.ones(3, 64, 64), src)       # Fm = 3 against F = 2
    for bad in (-1, 9, 1.5, float("nan"), True):
        with pytest.raises(ValueError, match="0 <= grow <= 8"):
            pipe.enable_masked_edit(mask, src, grow=bad)
    for bad in (-0.1, 8.5, float("nan")):
        with pytest.raises(ValueError, match="0 <= feather <= 8"):
            pipe.enable_masked_edit(mask, src, feather=bad)
    assert pipe._masked_edit is None
    # a frame-parallel clip: refused by the setter, and by the call when the clip became frame-parallel afterwards
    pipe.enable_masked_edit(mask, src)
    unet.frame_parallel = object()
    with pytest.raises(NotImplementedError, match="frame-parallel"):
        pipe._masked_edit_buffers(64, 64, 2, lat)
    with pytest.raises(NotImplementedError, match="frame-parallel"):
        pipe.enable_masked_edit(mask, src)
    unet.frame_parallel = None
    # a masked engine that is not handed this step's partner refuses to blend against the last one
    from anyv2v_amd.pipeline import _StepEngine
    eng = _StepEngine.__new__(_StepEngine)
    eng.stochastic, eng.ctx, eng.coef, eng.blend = False, types.SimpleNamespace(t_buf=torch.zeros(1)), torch.zeros(4), (lat.clone(), None)
    with pytest.raises(ValueError, match="partner latent"):
        eng._step(torch.zeros(1), torch.zeros(4), ("k",))


def test_abi_validation_without_gpu():
    """Host-side validation returns ANYV2V_EINVAL (-1) with a message before anything touches a device."""
    from anyv2v_amd import _lib
    lib = _lib.load()
    P = 4096   # any 16-byte-aligned non-null address: nothing on the device is dereferenced before the checks
    taps = (ctypes.c_float * 3)(0.25, 0.5, 0.25)
    good = dict(mask=P, Fm=1, H=64, W=64, grow=1, taps=taps, R=1, ws=2 * P, out=3 * P)

    def lm(**over):
        a = dict(good, **over)
        return lib.anyv2v_latent_mask_f16(a["mask"], a["Fm"], a["H"], a["W"], a["grow"], a["taps"], a["R"], a["ws"], a["out"], None)

    for name in ("mask", "ws", "out", "taps"):
        assert lm(**{name: None}) == -1 and b"null pointer" in lib.anyv2v_last_error(), name
    for over in (dict(H=60), dict(W=4), dict(H=0), dict(W=-8), dict(Fm=0)):
        assert lm(**over) == -1 and b"multiples of 8" in lib.anyv2v_last_error(), over
    for grow in (-1, 9):
        assert lm(grow=grow) == -1 and b"grow" in lib.anyv2v_last_error()
    for R in (-1, 25):
        assert lm(R=R) == -1 and b"R =" in lib.anyv2v_last_error()
    assert lm(Fm=1 << 10, H=1 << 11, W=1 << 11) == -1 and b"fit an int" in lib.anyv2v_last_error()
    for bad in (float("nan"), -0.5, 2.0, float("inf")):
        assert lm(taps=(ctypes.c_float * 3)(0.25, bad, 0.25)) == -1 and b"tap 1" in lib.anyv2v_last_error(), bad
    good2 = dict(x=P, src=2 * P, mask=3 * P, Fm=1, out=P, C=4, F=2, HW=64)

    def bl(**over):
        a = dict(good2, **over)
        return lib.anyv2v_masked_blend_f16(a["x"], a["src"], a["mask"], a["Fm"], a["out"], a["C"], a["F"], a["HW"], None)

    for name in ("x", "src", "mask", "out"):
        assert bl(**{name: None}) == -1 and b"null pointer" in lib.anyv2v_last_error(), name
    for over in (dict(C=0), dict(F=0), dict(HW=0), dict(HW=-8)):
        assert bl(**over) == -1 and b"bad arguments" in lib.anyv2v_last_error(), over
    for Fm in (0, 3, -1):
        assert bl(Fm=Fm) == -1 and b"must be 1 or F" in lib.anyv2v_last_error()
    assert bl(C=4, F=1 << 15, HW=1 << 15) == -1 and b"fit an int" in lib.anyv2v_last_error()
    assert bl(out=2 * P) == -1 and b"alias x only" in lib.anyv2v_last_error()


def test_header_binding_and_abi_version():
    from anyv2v_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "anyv2v_hip.h")).read()
    for sym, nargs in (("anyv2v_latent_mask_f16", 10), ("anyv2v_masked_blend_f16", 9)):
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % sym, hdr)
        assert decl and len(decl.group(1).split(",")) == nargs
        assert sym in _lib.SYMBOLS and len(_lib.SYMBOLS[sym][1]) == nargs
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), sym)
    assert "init_latents_proper" in hdr and "2206.02779" in hdr               # the call the entry points replace, cited
    consts = {k: int(v) for k, v in re.findall(r"#define ANYV2V_MASK_MAX_(\w+) (\d+)", hdr)}
    assert consts == dict(GROW=_lib.MASK_MAX_GROW, RADIUS=_lib.MASK_MAX_RADIUS) and consts["RADIUS"] == 3 * 8
    assert callable(ops.latent_mask) and callable(ops.masked_blend) and callable(ops.gaussian_taps)
    assert _lib.ABI_VERSION == 105 and "#define ANYV2V_ABI_VERSION 105" in hdr
    mk = open(os.path.join(ROOT, "anyv2v_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bmask\.hip\b", mk, re.M)


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


def _edit(pipe, c, eta=0.0, seed=0, trace=None, ratios=(0.5, 0.75, 1.0)):
    from anyv2v_amd import pnp_utils
    _register(pipe, ratios)
    try:
        return pipe.sample_with_pnp(prompt_embeds=c.ehs[2:3], negative_prompt_embeds=c.ehs[1:2], image_embeddings=c.ie[2:3],
                                    image_latents=c.il[2:3], height=HW_ * 8, width=HW_ * 8, num_frames=FR, num_inference_steps=STEPS,
                                    guidance_scale=9.0, target_fps=8, eta=eta, generator=torch.Generator().manual_seed(seed),
                                    latents=c.traj[c.T].clone(), output_type="latent", ddim_init_latents_t_idx=0, ddim_inv_latents_path=c.traj,
                                    ddim_inv_prompt_embeds=c.ehs[:1], ddim_inv_image_embeddings=c.ie[:1],
                                    ddim_inv_image_latents=c.il[:1], latents_trace=trace).frames.clone()
    finally:
        pnp_utils.clear_time(pipe)


def _half_plane(Fm=1):
    m = torch.zeros(Fm, HW_ * 8, HW_ * 8)
    m[:, :, : HW_ * 4] = 1.0          # the left half is edited, the right half keeps the source
    return m


LOOP_TOL = 1e-2   # as tests/test_sampler_options_host.py: the emulated step computes in fp32 what the definition computes in fp64, an fp16
                  # rounding of a latent may flip (2^-10 of the value) and three more UNet forwards see it; same UNet, same op emulation


def test_mini_pipeline_against_the_spec_loop(cpu_ops):
    """Half-plane mask, grown by 1 and feathered (sigma 0.5), with eta and the rescale on: every traced step against the spec loop; the kept
    half far from the feather is the source, bit for bit; mask off afterwards is bit-equal to never on, on an engine with today's key."""
    c = _clip()
    pipe = _pipe(c)
    off = _edit(pipe, c)
    key_off = [k for k in pipe._engines if k[0] in ("pnp", "pnp-droptail")]
    pipe.enable_guidance_rescale(0.7)
    pipe.enable_masked_edit(_half_plane(), c.lat0, grow=1, feather=0.5)
    trace = {}
    on = _edit(pipe, c, eta=0.5, seed=11, trace=trace)
    key_on = [k for k in pipe._engines if k[0] in ("pnp", "pnp-droptail")]
    assert len(key_off) == len(key_on) == 1 and key_on[0][:-2] == key_off[0] and key_on[0][-1] == ("blend", (1, HW_, HW_))
    assert not any(isinstance(x, tuple) and x and x[0] == "blend" for x in key_off[0])        # today's key
    lm = memu.latent_mask(_half_plane().half(), 1, 0.5)
    assert ulp_distance_fp16(lm, spec.latent_mask(_half_plane().half(), 1, 0.5).half()) <= 1
    assert float(lm[0, :, -1].max()) == 0.0 and float(lm[0, :, 0].min()) == 1.0, "the test's mask has no exact 0 / 1 columns"
    ref, ref_trace = spec.masked_edit_loop(c, STEPS, lm, c.lat0, _register, eta=0.5, phi=0.7, seed=11)
    assert list(trace) == list(ref_trace) and len(trace) == STEPS
    for t in trace:
        r = gc._res(f"masked edit after t = {t} vs the spec loop", trace[t], ref_trace[t].float(), LOOP_TOL)
        print(f"[masked-edit] t {t}: vs spec loop max {r['err']:.3e} l2 {r['l2']:.3e} (tol {LOOP_TOL})")
        assert r["ok"], r
    assert torch.equal(on, trace[min(trace)])
    kept = lm[0] == 0
    assert torch.equal(on[0, :, :, kept], c.lat0[0, :, :, kept]), "outside the mask the result is not the source's bits"
    edited = lm[0] == 1
    assert gc._rel(on[0, :, :, edited], c.lat0[0, :, :, edited].float())[1] > 10 * LOOP_TOL, "inside the mask nothing was edited"
    pipe.disable_masked_edit()
    pipe.disable_guidance_rescale()
    assert torch.equal(_edit(pipe, c), off), "mask off again: not bit-equal to never on"
    assert [k for k in pipe._engines if k[0] in ("pnp", "pnp-droptail")] == key_off


@pytest.mark.parametrize("ratios", [(0.5, 0.75, 1.0), (0.25, 0.25, 0.5)], ids=["three-branch", "with-source-free-steps"])
def test_partner_of_every_step(cpu_ops, monkeypatch, ratios):
    """What the blend of step i reads is ``traj[ts[i + 1]]``, after the last step ``source_latents`` -- recorded from the engines' static
    buffer right after each step was enqueued, whichever engine ran it (three-branch or [negative, editing] only); the all-zeros mask
    turns that into the latents themselves, the all-ones mask into the unmasked edit."""
    from anyv2v_amd.pipeline import _StepEngine
    from anyv2v_amd.schedulers import DDIMScheduler
    c = _clip()
    seen, engines = [], []
    inner = _StepEngine._step

    def spy(self, t_row, coef_row, key, noise=None, partner=None):
        inner(self, t_row, coef_row, key, noise, partner)
        if self.blend is not None:
            seen.append((key, self.blend[0].clone(), self.blend[0].data_ptr()))
            engines.append(self)
    monkeypatch.setattr(_StepEngine, "_step", spy)
    sched = DDIMScheduler()
    sched.set_timesteps(STEPS)
    ts = [int(t) for t in sched.timesteps]
    src = c.lat0 + 0.5                                  # (not the trajectory's start: the last partner is what the caller supplied)
    want = spec.partners(ts, c.traj, src)
    assert [torch.equal(w, c.traj[t]) for w, t in zip(want[:-1], ts[1:])] == [True] * (STEPS - 1) and want[-1] is src
    plain = _edit(_pipe(c), c, ratios=ratios)
    assert seen == []
    pipe = _pipe(c)
    pipe.enable_masked_edit(torch.zeros(HW_ * 8, HW_ * 8), src)
    trace = {}
    out = _edit(pipe, c, trace=trace, ratios=ratios)
    assert len(seen) == STEPS and all(torch.equal(s[1], w) for s, w in zip(seen, want)), "a step blended against another level"
    assert len({s[2] for s in seen}) == 1, "the engines of one edit do not share the partner buffer"
    assert all("blend" in s[0] for s in seen), "the graph key does not carry the option"
    if ratios[2] < 1.0:
        assert len(set(map(id, engines))) == 2, "the source-free steps did not run on the [negative, editing] engine"
    assert all(torch.equal(trace[t], w) for t, w in zip(ts, want)) and torch.equal(out, src)
    seen.clear()
    pipe.enable_masked_edit(torch.ones(FR, HW_ * 8, HW_ * 8, dtype=torch.bool), src)
    assert torch.equal(_edit(pipe, c, ratios=ratios), plain) and len(seen) == STEPS


# ------------------------------------------------------------------------------------------------ configuration keys
def test_config_keys_reach_the_setter(tmp_path, monkeypatch):
    """``edit_mask_path`` / ``_grow`` / ``_feather`` in the template or the JSON entry reach ``enable_masked_edit`` through ``Stage2`` with
    the mask file's pixels and the encoded source frames; the setter is cleared after the entry; absent, the call, the suffix and the
    pipeline are those of a job without the keys."""
    import logging

    import numpy as np
    from PIL import Image

    from anyv2v_amd.config import OmegaConf, masked_edit_options
    from anyv2v_amd.run_group_pnp_edit import Stage2, output_suffix
    from anyv2v_amd.utils import LatentTrajectory, load_edit_mask
    from anyv2v_amd.schedulers import DDIMScheduler
    tmpl = OmegaConf.load(os.path.join(ROOT, "configs", "group_pnp_edit", "template.yaml"))
    assert not any(k.startswith("edit_mask") for k in tmpl) and masked_edit_options(tmpl) is None
    entry = {"active": True, "task_name": "T", "video_name": "clip", "edited_first_frame_path": "demo/clip/e.png", "editing_prompt": "a robot",
             "edited_video_name": "robot"}
    plain = OmegaConf.merge(tmpl, OmegaConf.create(entry))
    assert output_suffix(plain, 1) == "ddim_init_latents_t_idx_1_nsteps_50_cfg_9.0_pnpf0.2_pnps0.2_pnpt0.5"
    full = OmegaConf.merge(tmpl, OmegaConf.create(dict(entry, edit_mask_path="demo/clip/hat.png", edit_mask_grow=2, edit_mask_feather=1.5)))
    assert masked_edit_options(full) == ("demo/clip/hat.png", 2, 1.5)
    assert output_suffix(full, 1) == output_suffix(plain, 1) + "_mask-hat_grow2_feather1.5"
    only = OmegaConf.merge(tmpl, OmegaConf.create(dict(entry, edit_mask_path="demo/clip/masks/")))
    assert masked_edit_options(only) == ("demo/clip/masks/", 0, 0.0) and output_suffix(only, 1) == output_suffix(plain, 1) + "_mask-masks"
    for bad, msg in ((dict(edit_mask_path="m.png", edit_mask_grow=9), "edit_mask_grow"), (dict(edit_mask_path="m.png", edit_mask_grow=1.5), "edit_mask_grow"),
                     (dict(edit_mask_path="m.png", edit_mask_feather=-1), "edit_mask_feather"),
                     (dict(edit_mask_path="m.png", edit_mask_feather=float("nan")), "edit_mask_feather"), (dict(edit_mask_grow=1), "without edit_mask_path")):
        with pytest.raises(ValueError, match=msg):
            masked_edit_options(OmegaConf.merge(tmpl, OmegaConf.create(bad)))
    # files: frames, the edited first frame, one mask PNG, a directory of per-frame masks, a mask of another size
    clip = tmp_path / "demo" / "clip"
    (clip / "masks").mkdir(parents=True)
    for i in range(2):
        Image.fromarray(np.full((64, 64, 3), 40 * i, dtype=np.uint8)).save(clip / f"{i:05d}.png")
        per = np.zeros((64, 64), dtype=np.uint8)
        per[: 16 * (i + 1)] = 255
        Image.fromarray(per).save(clip / "masks" / f"{i:05d}.png")
    Image.fromarray(np.full((64, 64, 3), 99, dtype=np.uint8)).save(clip / "e.png")
    hat = np.zeros((64, 64), dtype=np.uint8)
    hat[:24, 8:40] = 255
    Image.fromarray(hat).save(clip / "hat.png")
    Image.fromarray(np.zeros((32, 64), dtype=np.uint8)).save(clip / "small.png")
    m1 = load_edit_mask(str(clip / "hat.png"), 2, (64, 64))
    assert m1.dtype == torch.uint8 and tuple(m1.shape) == (1, 64, 64) and torch.equal(m1[0], torch.from_numpy(hat))
    m2 = load_edit_mask(str(clip / "masks"), 2, (64, 64))
    assert tuple(m2.shape) == (2, 64, 64) and int(m2[0].sum()) == 255 * 16 * 64 and int(m2[1].sum()) == 255 * 32 * 64
    with pytest.raises(ValueError, match="does not match config.image_size"):
        load_edit_mask(str(clip / "small.png"), 2, (64, 64))
    with pytest.raises(ValueError, match="not found"):
        load_edit_mask(str(clip / "masks"), 3, (64, 64))
    # through the runner: the pipeline's call recorded and stopped
    tmpl.data_dir, tmpl.device, tmpl.image_size, tmpl.n_frames, tmpl.n_steps = str(tmp_path), "cpu", [64, 64], 2, 4
    pipe, _unet = _meta_pipe()
    seen, encoded = [], []

    class Stop(Exception):
        pass

    def fake(**kw):
        me = pipe._masked_edit
        seen.append(None if me is None else (me["mask"].clone(), me["source_latents"], me["grow"], me["feather"]))
        raise Stop

    def fake_encode(frames, device=None, height=None, width=None):
        encoded.append((len(frames), height, width))
        return torch.full((1, 4, len(frames), height // 8, width // 8), float(len(encoded)), dtype=torch.float16)
    monkeypatch.setattr(pipe, "sample_with_pnp", fake)
    monkeypatch.setattr(pipe, "encode_vae_video", fake_encode)
    monkeypatch.setattr(pipe, "auto_vae_tiling", lambda *a: None)
    sched = DDIMScheduler()
    sched.set_timesteps(4)
    traj = LatentTrajectory()
    for t in sched.timesteps.tolist():
        traj[int(t)] = torch.zeros(1, 4, 2, 8, 8, dtype=torch.float16)
    lat_dir = os.path.abspath(str(OmegaConf.merge(tmpl, OmegaConf.create(entry)).ddim_latents_path))
    entries = [dict(entry), dict(entry, edit_mask_path="demo/clip/hat.png", edit_mask_grow=2, edit_mask_feather=1.5),
               dict(entry, edit_mask_path="demo/clip/masks"), dict(entry), dict(entry, edit_mask_path="demo/clip/small.png")]
    stage = Stage2(tmpl, entries, torch.device("cpu"), logging.getLogger("masked-edit"), pipe=pipe, trajectories={lat_dir: traj})
    for e in entries[:4]:
        with pytest.raises(Stop):
            stage.run_entry(e)
        assert pipe._masked_edit is None, "the setter was not cleared after the entry"
    assert seen[0] is None and seen[3] is None and encoded == [(2, 64, 64), (2, 64, 64)], "an entry without the keys touched the masked edit"
    mask, src, grow, feather = seen[1]
    assert torch.equal(mask, (torch.from_numpy(hat).float() / 255).half()[None]) and (grow, feather) == (2, 1.5) and float(src.max()) == 1.0
    mask, src, grow, feather = seen[2]
    assert tuple(mask.shape) == (2, 64, 64) and (grow, feather) == (0, 0.0) and float(src.max()) == 2.0
    with pytest.raises(ValueError, match="does not match config.image_size"):
        stage.run_entry(entries[4])
    assert pipe._masked_edit is None and len(seen) == 4
