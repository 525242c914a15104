"""Automatic edit masks without a GPU: the fp64 definition (tests/auto_mask_spec.py) against itself and against diffusers' expression,
the timestep choice, every refusal, the C ABI's host-side validation, the mini pipeline under the op emulation
(tests/cpu_auto_mask_emulation.py) against a spec loop on the same UNet forward, the generator discipline, the hand-over to the masked
edit, the configuration keys through the runner, and the share of near-threshold elements of the GPU tests' inputs."""
import ctypes
import logging
import os
import re
import types

import pytest
import torch

import auto_mask_spec as spec
import cpu_auto_mask_emulation as aemu
import gpu_checks as gc
from sampler_options_spec import ulp_distance_fp16

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FR, HW_, STEPS = 2, 8, 4
# the kernels' shapes (tests/test_auto_mask_gpu.py) and the seed of each shape's inputs: chosen so that the definition alone leaves at most
# 1 % of the map within 1 fp16 ulp of the threshold -- asserted below, on the CPU
GPU_SHAPES = [(1, 1, 1), (3, 5, 5), (1, 8, 8), (3, 3, 16), (2, 9, 7), (5, 64, 64)]
GPU_SEEDS = {s: 11 + i for i, s in enumerate(GPU_SHAPES)}


@pytest.fixture()
def cpu_ops(monkeypatch):
    aemu.install(monkeypatch)
    monkeypatch.setattr(gc, "DEV", "cpu")
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "1")
    yield


# ------------------------------------------------------------------------------------------------ the definition
def _rectangle(F=4, h=6, w=7, C=4, offset=0.5):
    g = torch.Generator().manual_seed(3)
    vs = torch.randn(C, F, h, w, generator=g).half()
    vt = vs.clone()
    inside = torch.zeros(F, h, w, dtype=torch.bool)
    inside[1:3, 2:5, 1:4] = True                     # a rectangle of frames 1 and 2; frames 0 and 3 do not change
    vt[:, inside] = (vs[:, inside].float() + offset).half()
    return vs, vt, inside


def test_spec_against_itself():
    vs, vt, inside = _rectangle()
    m16, pm, acc = spec.generate([(vs, vt)] * 3, 3.0, 0.5)
    assert torch.equal(pm, spec.pixel_mask(inside)) and tuple(pm.shape) == (4, 48, 56) and pm.dtype == torch.bool
    assert float(m16[0].max()) == 0.0 and float(m16[3].max()) == 0.0, "a frame in which nothing changes must come out empty"
    # identical predictions: an all-false mask and a map without NaN
    m0, pm0, acc0 = spec.generate([(vs, vs)], 3.0, 0.5)
    assert float(acc0.abs().max()) == 0.0 and not bool(torch.isnan(m0).any()) and float(m0.max()) == 0.0 and not bool(pm0.any())
    # scaling both predictions by 2 leaves the map unchanged (|2 a - 2 b| = 2 |a - b| exactly, the mean doubles with it)
    m2, pm2, _ = spec.generate([((vs.float() * 2).half(), (vt.float() * 2).half())] * 3, 3.0, 0.5)
    assert torch.equal(m2, m16) and torch.equal(pm2, pm)
    # maps are added in order, in fp32
    g = torch.Generator().manual_seed(4)
    pairs = [(torch.randn(4, 2, 3, 3, generator=g).half(), torch.randn(4, 2, 3, 3, generator=g).half()) for _ in range(3)]
    want = None
    for a, b in pairs:
        s = sum((b[c].float() - a[c].float()).abs() for c in range(4))
        want = s if want is None else want + s
    assert torch.equal(spec.generate(pairs, 3.0, 0.5)[2], want)


def test_spec_against_diffusers_expression():
    """The expression of diffusers' ``StableDiffusionDiffEditPipeline.generate_mask`` as this project states it, restated in fp64 on one
    frame, where the clip mean and the frame mean coincide:
        map = abs(noise_pred_target - noise_pred_source).reshape(1, N, C, h, w).mean([1, 2])
        map = clamp(map / map.mean() * mask_thresholding_ratio, 0, 1)
        mask = where(map <= threshold, 0, 1)
    The definition accumulates sums where this takes means: the factor 1 / (N C) cancels in ``map / map.mean()``."""
    N, C, h, w = 3, 4, 9, 7
    pairs = [(p[0].view(C, 1, h, w), p[1].view(C, 1, h, w)) for p in spec.fixture(1, h, w, N, 5, special=False)]
    tgt = torch.stack([p[1][:, 0] for p in pairs]).double()         # [N, C, h, w]
    src = torch.stack([p[0][:, 0] for p in pairs]).double()
    for ratio, thr in ((3.0, 0.5), (1.0, 0.3), (0.5, 0.75)):
        m = (tgt - src).abs().reshape(1, N, C, h, w).mean([1, 2])
        m = (m / m.mean() * ratio).clamp(0, 1)
        want = torch.where(m <= thr, 0, 1)[0]
        acc = None
        for a, b in pairs:
            acc = spec.accumulate(a, b, acc)
        m64, m16, mask = spec.finish(acc, ratio, thr)
        assert float((m64[0] - m[0]).abs().max()) < 1e-6      # (the accumulator is fp32, the restatement fp64 throughout)
        clear = ~spec.near_threshold(m64, thr)[0] & ((m[0] - thr).abs() > 1e-3)
        assert int(clear.sum()) > 0.9 * clear.numel() and torch.equal(mask[0][clear], want[clear].bool())


def test_timestep_choice():
    from anyv2v_amd.pipeline import edit_mask_timestep
    from anyv2v_amd.schedulers import DDIMScheduler
    # leading spacing with steps_offset 1: timesteps[i] = (steps - 1 - i) * (1000 // steps) + 1
    for steps, strength, want in ((50, 0.5, 481),    # init 25 -> timesteps[25] = 24 * 20 + 1
                                  (50, 1.0, 981),    # init 50 -> timesteps[0]
                                  (10, 0.05, 1),     # init 0 -> index 10 clamps to the last timestep, timesteps[9] = 1
                                  (3, 0.5, 1),       # init 1 -> timesteps[2] = 0 * 333 + 1
                                  (50, 0.2, 181)):   # init 10 -> timesteps[40] = 9 * 20 + 1
        sched = DDIMScheduler()
        sched.set_timesteps(steps)
        assert edit_mask_timestep(sched.timesteps, steps, strength) == want == spec.timestep(sched.timesteps, steps, strength)


# ------------------------------------------------------------------------------------------------ refusals
def _meta_pipe():
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMScheduler
    from anyv2v_amd.unet import I2VGenXLUNet, I2VGenXLUNetConfig
    with torch.device("meta"):
        unet = I2VGenXLUNet(I2VGenXLUNetConfig.mini())
    return I2VGenXLPipeline(unet=unet, scheduler=DDIMScheduler()), unet


def test_every_refusal_raises_with_its_message():
    from anyv2v_amd import pnp_utils
    from anyv2v_amd.schedulers import DDIMInverseScheduler, DDIMScheduler
    from anyv2v_amd.utils import LatentTrajectory
    pipe, unet = _meta_pipe()
    src = torch.zeros(1, 4, 2, 8, 8, dtype=torch.float16)
    emb = dict(prompt_embeds=torch.zeros(1, 77, 8), image_embeddings=torch.zeros(1, 1, 8), image_latents=src.clone(),
               ddim_inv_prompt_embeds=torch.zeros(1, 77, 8), ddim_inv_image_embeddings=torch.zeros(1, 1, 8), ddim_inv_image_latents=src.clone())
    ok = dict(emb, source_latents=src, height=64, width=64, num_frames=2, target_fps=8, num_inference_steps=4)
    call = lambda **over: pipe.generate_edit_mask(**dict(ok, **over))
    traj = LatentTrajectory()
    traj[501] = src.clone()
    unet.frame_parallel = object()
    with pytest.raises(NotImplementedError, match="frame-parallel"):
        call()
    unet.frame_parallel = None
    # PnP injection left registered for the current timestep; inert again after clear_time
    pnp_utils.register_temp_attention_pnp(pipe, [1, 501])
    pnp_utils.register_time(pipe, 501)
    with pytest.raises(ValueError, match="PnP injection is left registered"):
        call()
    pnp_utils.clear_time(pipe)
    # a foreign hook on seam B1
    site = unet.up_blocks[1].attentions[1].transformer_blocks[0].attn1
    native = site.processor
    site.processor = object()
    with pytest.raises(ValueError, match="foreign hooks"):
        call()
    site.processor = native
    with pytest.raises(ValueError, match="exactly one of"):
        call(ddim_inv_latents_path=traj)
    with pytest.raises(ValueError, match="exactly one of"):
        call(source_latents=None)
    for bad in (torch.zeros(1, 4, 3, 8, 8), torch.zeros(1, 4, 2, 8, 4), torch.zeros(4, 2, 8, 8), [1.0]):
        with pytest.raises(ValueError, match="source_latents"):
            call(source_latents=bad)
    with pytest.raises(ValueError, match="trajectory's latents .* do not match the call"):
        call(source_latents=None, ddim_inv_latents_path=traj, num_frames=3)
    with pytest.raises(ValueError, match="no inverted latents"):
        call(source_latents=None, ddim_inv_latents_path=LatentTrajectory())
    with pytest.raises(ValueError, match="divisible by 8"):
        call(height=60)
    for bad in (0, -1, 1.5, True, float("nan")):
        with pytest.raises(ValueError, match="num_maps_per_mask"):
            call(num_maps_per_mask=bad)
    for bad in (0.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="mask_encode_strength"):
            call(mask_encode_strength=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="mask_thresholding_ratio"):
            call(mask_thresholding_ratio=bad)
    for bad in (0.0, 1.0, -0.1, 2.0, float("nan")):
        with pytest.raises(ValueError, match="threshold="):
            call(threshold=bad)
    for over in (dict(prompt=["a", "b"], prompt_embeds=None), dict(ddim_inv_prompt=["a"])):
        with pytest.raises(ValueError, match="list of prompts"):
            call(**over)
    with pytest.raises(ValueError, match="batch of 2 prompts"):
        call(prompt_embeds=torch.zeros(2, 77, 8))
    with pytest.raises(ValueError, match="image latents .* do not match|do not match the edit's"):
        call(image_latents=torch.zeros(1, 4, 3, 8, 8, dtype=torch.float16))
    pipe.register_modules(scheduler=DDIMInverseScheduler())
    with pytest.raises(ValueError, match="forward DDIMScheduler"):
        call()
    pipe.register_modules(scheduler=DDIMScheduler())
    assert pipe._masked_edit is None


def test_config_refusals_and_defaults():
    from anyv2v_amd.config import OmegaConf, auto_mask_options, masked_edit_options
    tmpl = OmegaConf.load(os.path.join(ROOT, "configs", "group_pnp_edit", "template.yaml"))
    assert not any(k.startswith("edit_mask") for k in tmpl) and auto_mask_options(tmpl) is None
    mk = lambda **kw: OmegaConf.merge(tmpl, OmegaConf.create(kw))
    assert auto_mask_options(mk(edit_mask_auto=False)) is None and masked_edit_options(mk(edit_mask_auto=True)) is None
    assert auto_mask_options(mk(edit_mask_auto=True)) == dict(maps=10, strength=0.5, ratio=3.0, threshold=0.5, grow=0, feather=0.0)
    assert auto_mask_options(mk(edit_mask_auto=True, edit_mask_auto_maps=3, edit_mask_auto_strength=1, edit_mask_auto_ratio=2,
                                edit_mask_auto_threshold=0.25, edit_mask_grow=2, edit_mask_feather=1.5)) == \
        dict(maps=3, strength=1.0, ratio=2.0, threshold=0.25, grow=2, feather=1.5)
    assert masked_edit_options(mk(edit_mask_auto=True, edit_mask_grow=2)) is None
    for bad, msg in ((dict(edit_mask_auto=True, edit_mask_path="m.png"), "edit_mask_auto together with edit_mask_path"),
                     (dict(edit_mask_auto="yes"), "true or false"), (dict(edit_mask_auto=1), "true or false"),
                     (dict(edit_mask_auto_maps=3), "edit_mask_auto_maps without edit_mask_auto"),
                     (dict(edit_mask_auto=False, edit_mask_auto_ratio=2.0), "edit_mask_auto_ratio without edit_mask_auto"),
                     (dict(edit_mask_auto=True, edit_mask_auto_maps=0), "edit_mask_auto_maps"),
                     (dict(edit_mask_auto=True, edit_mask_auto_maps=2.5), "edit_mask_auto_maps"),
                     (dict(edit_mask_auto=True, edit_mask_auto_maps=float("nan")), "edit_mask_auto_maps"),
                     (dict(edit_mask_auto=True, edit_mask_auto_maps=True), "edit_mask_auto_maps"),
                     (dict(edit_mask_auto=True, edit_mask_auto_strength=0), "edit_mask_auto_strength"),
                     (dict(edit_mask_auto=True, edit_mask_auto_strength=1.5), "edit_mask_auto_strength"),
                     (dict(edit_mask_auto=True, edit_mask_auto_strength=float("nan")), "edit_mask_auto_strength"),
                     (dict(edit_mask_auto=True, edit_mask_auto_ratio=0), "edit_mask_auto_ratio"),
                     (dict(edit_mask_auto=True, edit_mask_auto_ratio=float("inf")), "edit_mask_auto_ratio"),
                     (dict(edit_mask_auto=True, edit_mask_auto_ratio=float("nan")), "edit_mask_auto_ratio"),
                     (dict(edit_mask_auto=True, edit_mask_auto_threshold=0), "edit_mask_auto_threshold"),
                     (dict(edit_mask_auto=True, edit_mask_auto_threshold=1), "edit_mask_auto_threshold"),
                     (dict(edit_mask_auto=True, edit_mask_auto_threshold=float("nan")), "edit_mask_auto_threshold"),
                     (dict(edit_mask_auto=True, edit_mask_grow=9), "edit_mask_grow"),
                     (dict(edit_mask_auto=True, edit_mask_feather=-1), "edit_mask_feather")):
        with pytest.raises(ValueError, match=msg):
            auto_mask_options(mk(**bad))
    with pytest.raises(ValueError, match="edit_mask_auto together with edit_mask_path"):
        masked_edit_options(mk(edit_mask_auto=True, edit_mask_path="m.png"))
    with pytest.raises(ValueError, match="without edit_mask_path"):       # as before the automatic mask existed
        masked_edit_options(mk(edit_mask_grow=1))
    with pytest.raises(ValueError, match="without edit_mask_path"):
        masked_edit_options(mk(edit_mask_grow=1, edit_mask_auto=False))


# ------------------------------------------------------------------------------------------------ ABI
def _lib_or_skip():
    from anyv2v_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.skip("libanyv2v_hip.so is not built")
    return _lib.load()


def test_abi_validation_without_gpu():
    """Host-side validation returns ANYV2V_EINVAL (-1) with a message before anything touches a device."""
    lib = _lib_or_skip()
    P = 4096   # any 16-byte-aligned non-null address: nothing on the device is dereferenced before the checks
    good = dict(V=P, ldv=8, C=4, F=2, HW=64, acc=2 * P, first=1, flag=None)

    def ac(**over):
        a = dict(good, **over)
        return lib.anyv2v_diff_map_accum_f16(a["V"], a["ldv"], a["C"], a["F"], a["HW"], a["acc"], a["first"], a["flag"], None)

    for name in ("V", "acc"):
        assert ac(**{name: None}) == -1 and b"null pointer" in lib.anyv2v_last_error(), name
    for over in (dict(C=0), dict(F=0), dict(HW=0), dict(HW=-4), dict(ldv=3), dict(C=9)):
        assert ac(**over) == -1 and b"bad arguments" in lib.anyv2v_last_error(), over
    assert ac(F=1 << 15, HW=1 << 15) == -1 and b"fit an int" in lib.anyv2v_last_error()
    for first in (2, -1):
        assert ac(first=first) == -1 and b"first" in lib.anyv2v_last_error()
    good2 = dict(acc=P, F=2, h=8, w=8, ratio=3.0, thr=0.5, rec=2 * P, map=3 * P, pm=4 * P)

    def fi(**over):
        a = dict(good2, **over)
        return lib.anyv2v_diff_map_finish_f16(a["acc"], a["F"], a["h"], a["w"], a["ratio"], a["thr"], a["rec"], a["map"], a["pm"], None)

    for name in ("acc", "rec", "map", "pm"):
        assert fi(**{name: None}) == -1 and b"null pointer" in lib.anyv2v_last_error(), name
    for over in (dict(F=0), dict(h=0), dict(w=-1)):
        assert fi(**over) == -1 and b"bad arguments" in lib.anyv2v_last_error(), over
    assert fi(F=1 << 9, h=1 << 8, w=1 << 8) == -1 and b"fit an int" in lib.anyv2v_last_error()
    for ratio in (0.0, -1.0, float("inf"), float("nan")):
        assert fi(ratio=ratio) == -1 and b"ratio" in lib.anyv2v_last_error(), ratio
    for thr in (0.0, 1.0, -0.5, 1.5, float("nan"), float("inf")):
        assert fi(thr=thr) == -1 and b"threshold" in lib.anyv2v_last_error(), thr


def test_header_binding_and_abi_version():
    from anyv2v_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "anyv2v_hip.h")).read()
    for sym, nargs in (("anyv2v_diff_map_accum_f16", 9), ("anyv2v_diff_map_finish_f16", 10)):
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % sym, hdr)
        assert decl and len(decl.group(1).split(",")) == nargs
        assert sym in _lib.SYMBOLS and len(_lib.SYMBOLS[sym][1]) == nargs
    assert "2210.11427" in hdr and "mask_guidance_map" in hdr                    # the call the entry points replace, cited
    consts = {k: int(v) for k, v in re.findall(r"#define ANYV2V_DIFF_MAP_(\w+) (\d+)", hdr)}
    assert consts == dict(BLOCKS=_lib.DIFF_MAP_BLOCKS, THREADS=_lib.DIFF_MAP_THREADS)
    assert callable(ops.diff_map_accum) and callable(ops.diff_map_finish)
    assert _lib.ABI_VERSION == 105 and "#define ANYV2V_ABI_VERSION 105" in hdr
    mk = open(os.path.join(ROOT, "anyv2v_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bautomask\.hip\b", mk, re.M)
    if os.path.isfile(_lib.LIB_PATH):
        assert all(hasattr(ctypes.CDLL(_lib.LIB_PATH), s) for s in ("anyv2v_diff_map_accum_f16", "anyv2v_diff_map_finish_f16"))


# ------------------------------------------------------------------------------------------------ emulation and GPU inputs vs the definition
@pytest.mark.parametrize("shape", GPU_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_gpu_inputs_share_near_the_threshold_and_emulation(shape):
    """The inputs of the GPU tests, evaluated by the definition on the CPU: at most 1 % of the map lies within 1 fp16 ulp of the threshold
    (the elements the GPU test leaves out of its mask comparison) -- a condition on the seeds, not a measurement.  The op emulation on the
    same inputs: accumulator bit-equal, map within 1 fp16 ulp, mask the exact function of its map."""
    F, h, w = shape
    n = F * h * w
    pairs = spec.fixture(F, h, w, 3, GPU_SEEDS[shape], special=False)
    acc = None
    got = torch.full((n,), float("nan"))
    for k, (a, b) in enumerate(pairs):
        acc = spec.accumulate(a, b, acc)
        vtok = torch.full((2 * n, 8), float("nan"), dtype=torch.float16)
        vtok[:n, :4], vtok[n:, :4] = a.t(), b.t()
        aemu.diff_map_accum(vtok, 4, F, h * w, got, k == 0)
    assert torch.equal(got, acc)
    for ratio, thr in ((3.0, 0.5), (1.0, 0.3)):
        m64, m16, mask = spec.finish(acc.view(F, h, w), ratio, thr)
        near = spec.near_threshold(m64, thr)
        assert int(near.sum()) <= 0.01 * n, f"{int(near.sum())} of {n} elements within 1 fp16 ulp of the threshold: choose another seed"
        em, epm = aemu.diff_map_finish(got, F, h, w, ratio, thr)
        assert ulp_distance_fp16(em, m16) <= 1
        assert torch.equal(epm, spec.pixel_mask(em > torch.tensor(thr).half())) and torch.equal((em > torch.tensor(thr).half())[~near], mask[~near])


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


def _generate(pipe, c, same=False, **kw):
    e = 0 if same else 2
    return pipe.generate_edit_mask(prompt_embeds=c.ehs[e:e + 1], image_embeddings=c.ie[e:e + 1], image_latents=c.il[e:e + 1],
                                   ddim_inv_prompt_embeds=c.ehs[:1], ddim_inv_image_embeddings=c.ie[:1], ddim_inv_image_latents=c.il[:1],
                                   height=HW_ * 8, width=HW_ * 8, num_frames=FR, target_fps=8, num_inference_steps=STEPS, **kw)


def _spec_loop(c, x_ts, t, ratio, thr):
    """The definition on the same UNet forward: one [source, edit] evaluation per x_t."""
    kw = dict(fps=torch.tensor([8] * 2), encoder_hidden_states=torch.cat([c.ehs[:1], c.ehs[2:3]]),
              image_embeddings=torch.cat([c.ie[:1], c.ie[2:3]]), image_latents=torch.cat([c.il[:1], c.il[2:3]]))
    pairs = []
    for x in x_ts:
        v = c.native(torch.cat([x, x]), t, **kw)[0].half()
        pairs.append((v[0], v[1]))
    acc = None
    for a, b in pairs:
        acc = spec.accumulate(a, b, acc)
    return acc, spec.finish(acc, ratio, thr)


@pytest.mark.parametrize("N", [1, 3])
def test_mini_pipeline_against_the_spec_loop(cpu_ops, N):
    """Noise-draw variant: the traced accumulator equals the spec loop's bit for bit (the same forward, the stated order), the map is within
    1 fp16 ulp of the definition on it, the mask is the exact function of the returned map and the 8 x 8 replication of it (Fm = F); the
    generator ends where N draws of ``scheduler.draw_noise`` end; the result feeds ``enable_masked_edit``."""
    from anyv2v_amd import ops
    from anyv2v_amd.schedulers import DDIMScheduler
    c = _clip()
    pipe = _pipe(c)
    trace = {}
    gen = torch.Generator().manual_seed(5)
    pm = _generate(pipe, c, source_latents=c.lat0, num_maps_per_mask=N, generator=gen, trace=trace, mask_thresholding_ratio=1.0)
    assert pm.dtype == torch.bool and tuple(pm.shape) == (FR, HW_ * 8, HW_ * 8) and pipe._masked_edit is None
    sched = DDIMScheduler()
    sched.set_timesteps(STEPS)
    t = spec.timestep(sched.timesteps, STEPS, 0.5)
    assert trace["timestep"] == t == 251 and len(trace["x_t"]) == N
    ref = torch.Generator().manual_seed(5)
    x_ts = [sched.add_noise(c.lat0, sched.draw_noise(c.lat0, ref), torch.tensor([t])) for _ in range(N)]
    assert torch.equal(gen.get_state(), ref.get_state()), "the generator is not where N draws of scheduler.draw_noise leave it"
    assert all(x.dtype == torch.float16 and torch.equal(x, y) for x, y in zip(x_ts, trace["x_t"]))
    acc, (m64, m16, mask) = _spec_loop(c, x_ts, t, 1.0, 0.5)
    assert torch.equal(trace["acc"], acc) and float(acc.min()) > 0.0
    assert ulp_distance_fp16(trace["map"], m16) <= 1
    got = trace["map"] > torch.tensor(0.5).half()
    assert torch.equal(pm, spec.pixel_mask(got))
    near = spec.near_threshold(m64, 0.5)
    assert torch.equal(got[~near], mask[~near]) and 0 < int(got.sum()) < got.numel(), "the test's mask is empty or full"
    # the result is what enable_masked_edit takes, and its pooling gives the latent-size mask back bit for bit
    pipe.enable_masked_edit(pm, c.lat0)
    assert torch.equal(ops.latent_mask(pipe._masked_edit["mask"]), got.half())
    pipe.disable_masked_edit()


def test_mini_pipeline_trajectory_variant_and_identical_conditioning(cpu_ops):
    """Deterministic variant: x_t is the trajectory's entry nearest to the chosen timestep, one map whatever ``num_maps_per_mask`` says, no
    draw from the generator.  Identical source and edit conditioning: an empty mask, a zero map, no NaN."""
    c = _clip()
    pipe = _pipe(c)
    trace = {}
    gen = torch.Generator().manual_seed(9)
    before = gen.get_state()
    pm = _generate(pipe, c, ddim_inv_latents_path=c.traj, generator=gen, trace=trace, mask_thresholding_ratio=1.0)
    assert torch.equal(gen.get_state(), before)
    t = trace["timestep"]
    assert t == 251 and t in c.traj.keys() and len(trace["x_t"]) == 1 and torch.equal(trace["x_t"][0], c.traj[t])
    acc, (m64, m16, mask) = _spec_loop(c, [c.traj[t]], t, 1.0, 0.5)
    assert torch.equal(trace["acc"], acc) and ulp_distance_fp16(trace["map"], m16) <= 1
    assert torch.equal(pm, spec.pixel_mask(trace["map"] > torch.tensor(0.5).half()))
    # a strength whose timestep is no entry: the nearest scheduled one (1.0 -> t 751, an entry; 0.3 -> init 1 -> timesteps[3] = 1)
    tr2 = {}
    _generate(pipe, c, ddim_inv_latents_path=c.traj, mask_encode_strength=0.3, trace=tr2)
    assert tr2["timestep"] == 1
    sparse = type(c.traj)()
    sparse[751], sparse[1] = c.traj[751], c.traj[1]
    tr3 = {}
    _generate(pipe, c, ddim_inv_latents_path=sparse, trace=tr3)          # t = 251: 1 is nearer than 751
    assert tr3["timestep"] == 1 and torch.equal(tr3["x_t"][0], c.traj[1])
    # the directory form of the trajectory
    tr4 = {}
    same = _generate(pipe, c, same=True, source_latents=c.lat0, num_maps_per_mask=2, generator=gen, trace=tr4)
    assert not bool(same.any()) and float(tr4["map"].abs().max()) == 0.0 and float(tr4["acc"].abs().max()) == 0.0
    assert not bool(torch.isnan(tr4["map"]).any())


def test_trajectory_directory(cpu_ops, tmp_path):
    c = _clip()
    c.traj.save(str(tmp_path / "ddim_latents"))
    a, b = {}, {}
    pm_a = _generate(_pipe(c), c, ddim_inv_latents_path=c.traj, trace=a)
    pm_b = _generate(_pipe(c), c, ddim_inv_latents_path=str(tmp_path / "ddim_latents"), trace=b)
    assert torch.equal(pm_a, pm_b) and torch.equal(a["map"], b["map"]) and a["timestep"] == b["timestep"]


# ------------------------------------------------------------------------------------------------ configuration keys
def test_config_keys_through_the_runner(tmp_path, monkeypatch):
    """``edit_mask_auto`` and its tuning keys reach ``generate_edit_mask`` through ``Stage2``, the result reaches ``enable_masked_edit`` with
    grow / feather, the mask frames are written as ``mask_%05d.png`` beside the video and reload equal; an entry without the keys calls
    nothing new and writes the file set and suffix it wrote before."""
    import numpy as np
    from PIL import Image

    from anyv2v_amd.config import OmegaConf
    from anyv2v_amd.run_group_pnp_edit import Stage2, output_suffix
    from anyv2v_amd.schedulers import DDIMScheduler
    from anyv2v_amd.utils import LatentTrajectory, load_edit_mask
    tmpl = OmegaConf.load(os.path.join(ROOT, "configs", "group_pnp_edit", "template.yaml"))
    entry = {"active": True, "task_name": "T", "video_name": "clip", "edited_first_frame_path": "demo/clip/e.png", "editing_prompt": "a robot",
             "edited_video_name": "robot"}
    plain = OmegaConf.merge(tmpl, OmegaConf.create(entry))
    base = "ddim_init_latents_t_idx_1_nsteps_50_cfg_9.0_pnpf0.2_pnps0.2_pnpt0.5"     # (pinned by tests/test_masked_edit_host.py)
    assert output_suffix(plain, 1) == base
    mk = lambda **kw: OmegaConf.merge(tmpl, OmegaConf.create(dict(entry, **kw)))
    assert output_suffix(mk(edit_mask_auto=True), 1) == base + "_mask-auto"
    assert output_suffix(mk(edit_mask_auto=False), 1) == base
    assert output_suffix(mk(edit_mask_auto=True, edit_mask_auto_maps=3, edit_mask_auto_threshold=0.25, edit_mask_grow=2, edit_mask_feather=1.5), 1) \
        == base + "_mask-auto_maps3_threshold0.25_grow2_feather1.5"
    assert output_suffix(mk(edit_mask_auto=True, edit_mask_auto_strength=0.8, edit_mask_auto_ratio=2), 1) == base + "_mask-auto_strength0.8_ratio2.0"
    clip = tmp_path / "demo" / "clip"
    clip.mkdir(parents=True)
    for i in range(2):
        Image.fromarray(np.full((64, 64, 3), 40 * i, dtype=np.uint8)).save(clip / f"{i:05d}.png")
    Image.fromarray(np.full((64, 64, 3), 99, dtype=np.uint8)).save(clip / "e.png")
    tmpl.data_dir, tmpl.device, tmpl.image_size, tmpl.n_frames, tmpl.n_steps = str(tmp_path), "cpu", [64, 64], 2, 4
    pipe, _unet = _meta_pipe()
    gen_calls, edits, encoded = [], [], []
    auto_mask = torch.zeros(2, 64, 64, dtype=torch.bool)
    auto_mask[0, :16, 8:40], auto_mask[1, 8:24, 16:48] = True, True

    def fake_generate(**kw):
        gen_calls.append(kw)
        assert pipe._masked_edit is None
        return auto_mask.clone()

    def fake_edit(**kw):
        me = pipe._masked_edit
        edits.append(None if me is None else (me["mask"].clone(), me["source_latents"], me["grow"], me["feather"]))
        return types.SimpleNamespace(frames=torch.zeros(1, 4, 2, 8, 8, dtype=torch.float16))

    def fake_encode(frames, device=None, height=None, width=None):
        encoded.append((len(frames), height, width))
        return torch.full((1, 4, len(frames), height // 8, width // 8), float(len(encoded)), dtype=torch.float16)
    monkeypatch.setattr(pipe, "generate_edit_mask", fake_generate)
    monkeypatch.setattr(pipe, "sample_with_pnp", fake_edit)
    monkeypatch.setattr(pipe, "encode_vae_video", fake_encode)
    monkeypatch.setattr(pipe, "auto_vae_tiling", lambda *a: None)
    monkeypatch.setattr(pipe, "decode_latents", lambda lat, decode_chunk_size=None: torch.zeros(1, 3, 2, 64, 64))
    pipe.vae = types.SimpleNamespace(to_pil=lambda video: [Image.fromarray(np.zeros((64, 64, 3), dtype=np.uint8)) for _ in range(video.shape[2])])
    sched = DDIMScheduler()
    sched.set_timesteps(4)
    traj = LatentTrajectory()
    for t in sched.timesteps.tolist():
        traj[int(t)] = torch.zeros(1, 4, 2, 8, 8, dtype=torch.float16)
    lat_dir = os.path.abspath(str(OmegaConf.merge(tmpl, OmegaConf.create(entry)).ddim_latents_path))
    tuned = dict(entry, edit_mask_auto=True, edit_mask_auto_maps=3, edit_mask_auto_strength=0.75, edit_mask_auto_ratio=2.0,
                 edit_mask_auto_threshold=0.25, edit_mask_grow=2, edit_mask_feather=1.5, edited_video_name="tuned")
    entries = [dict(entry), dict(entry, edit_mask_auto=True, edited_video_name="auto"), tuned]
    files = lambda e: sorted(os.listdir(os.path.join(str(OmegaConf.merge(tmpl, OmegaConf.create(e)).output_dir),
                                                     output_suffix(OmegaConf.merge(tmpl, OmegaConf.create(e)), 1))))
    # the trajectory handed over in HBM (run_group_anyv2v): the deterministic variant
    stage = Stage2(tmpl, entries, torch.device("cpu"), logging.getLogger("auto-mask"), pipe=pipe, trajectories={lat_dir: traj})
    for e in entries:
        stage.run_entry(e)
        assert pipe._masked_edit is None, "the setter was not cleared after the entry"
    parent_files = ["edited_latents.pt", "video.gif", "video.mp4", "video_00000.png", "video_00001.png"]
    assert files(entries[0]) == parent_files and edits[0] is None and len(gen_calls) == 2 and encoded == [(2, 64, 64)] * 2
    assert files(entries[1]) == sorted(parent_files + ["mask_00000.png", "mask_00001.png"]) == files(entries[2])
    kw = gen_calls[0]
    assert kw["ddim_inv_latents_path"] is traj and "source_latents" not in kw and kw["prompt"] == "a robot" and kw["ddim_inv_prompt"] == ""
    assert (kw["height"], kw["width"], kw["num_frames"], kw["num_inference_steps"], kw["target_fps"]) == (64, 64, 2, 4, 8)
    assert (kw["num_maps_per_mask"], kw["mask_encode_strength"], kw["mask_thresholding_ratio"], kw["threshold"]) == (10, 0.5, 3.0, 0.5)
    kw = gen_calls[1]
    assert (kw["num_maps_per_mask"], kw["mask_encode_strength"], kw["mask_thresholding_ratio"], kw["threshold"]) == (3, 0.75, 2.0, 0.25)
    mask, src, grow, feather = edits[1]
    assert torch.equal(mask, auto_mask.half()) and (grow, feather) == (0, 0.0) and float(src.max()) == 1.0
    assert edits[2][2:] == (2, 1.5)
    cfg1 = OmegaConf.merge(tmpl, OmegaConf.create(entries[1]))
    out = os.path.join(str(cfg1.output_dir), output_suffix(cfg1, 1))
    assert out.endswith("_mask-auto")
    for i in range(2):
        back = load_edit_mask(os.path.join(out, f"mask_{i:05d}.png"), 2, (64, 64))
        assert torch.equal(back[0], auto_mask[i].to(torch.uint8) * 255)
    # read from files (no hand-over): noise draws on the encoded source latents
    traj.save(lat_dir)
    gen_calls.clear()
    stage = Stage2(tmpl, entries, torch.device("cpu"), logging.getLogger("auto-mask"), pipe=pipe)
    stage.run_entry(entries[1])
    kw = gen_calls[0]
    assert "ddim_inv_latents_path" not in kw and float(kw["source_latents"].max()) == 3.0 and kw["generator"] is not None
