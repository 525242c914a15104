"""Masked PnP editing on the GPU, the kernels through the C ABI: the latent mask and the blend against the fp64 definition
(tests/masked_edit_spec.py) on the same fp16 inputs, both inside NaN-poisoned frames (aligned, and offset so that the scalar path runs),
and the mini pipeline (all-ones / all-zeros / half-plane masks, HIP graphs against ANYV2V_NO_GRAPH=1, the parent path with the setter
off, the multi-edit source-feature cache, eta and the guidance rescale together with a mask).

Bounds: pool and grow alone, and the blend, bit-equal to the definition; with the feather 1 fp16 ulp (the fp32 error of <= 49 x 49 taps
is far below half an fp16 ulp, so only ties can move).  Measured on an MI355X (printed by the tests): 0 fp16 ulp on every case."""
import ctypes
import os
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = [(0, 0.0), (1, 0.0), (8, 0.0), (0, 0.5), (2, 1.5), (0, 8.0)]
POISON16, POISON32 = 0x7E5A, 0x7FC5A5A5      # NaN bit patterns no kernel computes (tests/gpu_checks.py)


def _masks(Fm, H, W, seed=0):
    """A binary mask aligned to the 8 x 8 blocks, a binary mask that is not, a random soft mask: fp16 [Fm, H, W] on the host."""
    g = torch.Generator().manual_seed(100 * Fm + H + W + seed)
    aligned = torch.zeros(Fm, H, W)
    aligned[:, : max(8, H // 16 * 8), : max(8, W // 16 * 8)] = 1.0
    ragged = torch.zeros(Fm, H, W)
    for f in range(Fm):
        ragged[f, 1 + f: max(3, H // 2 + 3), 2: max(5, W // 2 + 5 - f)] = 1.0
    soft = torch.rand(Fm, H, W, generator=g)
    return {"aligned": aligned.half(), "ragged": ragged.half(), "soft": soft.half()}


def _c_latent_mask(mask, grow, sigma, ws, out):
    """``anyv2v_latent_mask_f16`` on caller-owned operands (``ops.latent_mask`` allocates the workspace itself)."""
    from anyv2v_amd import _lib, ops
    taps = ops.gaussian_taps(sigma)
    arr = (ctypes.c_float * len(taps))(*taps) if taps else None
    Fm, H, W = mask.shape
    _lib.check(_lib.load().anyv2v_latent_mask_f16(mask.data_ptr(), Fm, H, W, grow, arr, len(taps) // 2, ws.data_ptr(), out.data_ptr(),
                                                 torch.cuda.current_stream().cuda_stream), "anyv2v_latent_mask_f16")
    return out


def _c_blend(x, s, m, out):
    from anyv2v_amd import _lib
    _, C, F, h, w = x.shape
    _lib.check(_lib.load().anyv2v_masked_blend_f16(x.data_ptr(), s.data_ptr(), m.data_ptr(), m.shape[0], out.data_ptr(), C, F, h * w,
                                                  torch.cuda.current_stream().cuda_stream), "anyv2v_masked_blend_f16")
    return out


# ------------------------------------------------------------------------------------------------ latent mask
@pytest.mark.parametrize("Fm", [1, 3])
@pytest.mark.parametrize("H,W", [(8, 8), (40, 24), (64, 64)])
def test_latent_mask_against_the_definition(Fm, H, W):
    """Pool and grow alone (sigma = 0): bit-equal to the definition rounded to fp16 -- the pooled sum is exact, the maximum is exact.
    With the feather: at most 1 fp16 ulp.  (8, 8) is one latent pixel: every window and every radius is wider than the image."""
    import masked_edit_spec as spec
    from anyv2v_amd import ops
    from sampler_options_spec import ulp_distance_fp16
    worst = 0
    for name, m in _masks(Fm, H, W).items():
        dm = m.cuda()
        for grow, sigma in PARAMS:
            want = spec.latent_mask(m, grow, sigma).half()
            got = ops.latent_mask(dm, grow, sigma).cpu()
            assert tuple(got.shape) == (Fm, H // 8, W // 8)
            if sigma == 0:
                assert torch.equal(got, want), (name, grow)
            else:
                d = ulp_distance_fp16(got, want)
                worst = max(worst, d)
                assert d <= 1, (name, grow, sigma, d)
    print(f"[masked-edit] latent mask Fm {Fm} {H} x {W}: with the feather at most {worst} fp16 ulp from the rounded definition")


# ------------------------------------------------------------------------------------------------ blend
@pytest.mark.parametrize("h,w", [(5, 5), (8, 8), (3, 16), (9, 7)])
def test_blend_against_the_definition(h, w):
    """Bit-equal to the definition's fp16(fma), in place and out of place; where m == 0 the output is s, where m == 1 it is x -- with Inf
    and NaN planted in the dropped operand at those positions.  (8, 8) and (3, 16) take the 16-byte path, (5, 5) and (9, 7) the scalar."""
    import masked_edit_spec as spec
    g = torch.Generator().manual_seed(10 * h + w)
    for F in (1, 3):
        for Fm in sorted({1, F}):
            x, s = torch.randn(1, 4, F, h, w, generator=g).half(), torch.randn(1, 4, F, h, w, generator=g).half()
            m = torch.rand(Fm, h, w, generator=g).half()
            m.view(-1)[::3], m.view(-1)[1::3] = 0.0, 1.0
            mm = m[None, None].expand(x.shape)
            want = spec.blend(x, s, m)
            n0, n1 = int((mm == 0).sum()), int((mm == 1).sum())
            x[mm == 0] = torch.tensor([float("inf"), float("nan"), float("-inf")]).half().repeat(n0 // 3 + 1)[:n0]
            s[mm == 1] = torch.tensor([float("nan"), float("inf")]).half().repeat(n1 // 2 + 1)[:n1]
            assert torch.equal(spec.blend(x, s, m).view(torch.int16), want.view(torch.int16))
            dx, ds, dm = x.cuda(), s.cuda(), m.cuda()
            out = _c_blend(dx, ds, dm, torch.empty_like(dx))
            assert torch.equal(out.cpu().view(torch.int16), want.view(torch.int16)), ("out of place", F, Fm)
            assert torch.equal(out.cpu()[mm == 0].view(torch.int16), s[mm == 0].view(torch.int16))
            assert torch.equal(out.cpu()[mm == 1].view(torch.int16), x[mm == 1].view(torch.int16))
            assert torch.equal(dx.cpu().view(torch.int16), x.view(torch.int16)), "an input changed"
            _c_blend(dx, ds, dm, dx)
            assert torch.equal(dx.cpu().view(torch.int16), want.view(torch.int16)), ("in place", F, Fm)


# ------------------------------------------------------------------------------------------------ edges
def _window(t, shift=0, pad=64):
    """``t`` copied into a contiguous window of a NaN-poisoned allocation, ``shift`` elements behind a 16-byte boundary (0: aligned;
    1: no 16-byte access can be aligned) -> (buffer, view, check) with ``check()`` true while everything outside the window is intact."""
    item = t.element_size()
    idt, bits = (torch.int16, POISON16) if item == 2 else (torch.int32, POISON32)
    n, lo = t.numel(), pad + shift
    buf = torch.full((lo + n + pad,), bits, dtype=idt, device="cuda")
    assert buf.data_ptr() % 16 == 0 and (pad * item) % 16 == 0
    view = buf.view(t.dtype)[lo:lo + n].view(t.shape)
    view.copy_(t)
    return buf, view, lambda: bool((buf[:lo] == bits).all() and (buf[lo + n:] == bits).all())


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "offset-scalar-path"])
def test_operands_inside_nan_poisoned_frames(shift):
    """Every operand of both kernels a window of a NaN-filled allocation: the bits of the plain launch, every frame intact -- nothing is
    read outside the operands (a poison NaN would reach the result) and nothing written outside the outputs.  With the windows one
    element behind a 16-byte boundary the blend runs its scalar kernel on a shape that otherwise takes the 16-byte one."""
    from anyv2v_amd import ops
    g = torch.Generator().manual_seed(5 + shift)
    # latent mask: 3 frames of 40 x 24 (h x w = 5 x 3), grown and feathered (all three launches)
    m = _masks(3, 40, 24, seed=1)["soft"].cuda()
    plain = ops.latent_mask(m, 2, 1.5)
    fm, vm, ok_m = _window(m, shift)
    fw, vw, ok_w = _window(torch.zeros(2 * plain.numel(), dtype=torch.float32, device="cuda"), shift)
    fo, vo, ok_o = _window(torch.zeros_like(plain), shift)
    _c_latent_mask(vm, 2, 1.5, vw, vo)
    torch.cuda.synchronize()
    assert torch.equal(vo, plain), "latent mask differs inside frames"
    assert ok_m() and ok_w() and ok_o() and torch.equal(vm, m), "latent mask: a frame or the input changed"
    # blend: 3 frames of 8 x 8 (HW % 8 == 0: the 16-byte kernel when aligned), per-frame mask, out of place and in place
    x, s = torch.randn(1, 4, 3, 8, 8, generator=g).half().cuda(), torch.randn(1, 4, 3, 8, 8, generator=g).half().cuda()
    lm = torch.rand(3, 8, 8, generator=g).half()
    lm.view(-1)[::3], lm.view(-1)[1::3] = 0.0, 1.0
    lm = lm.cuda()
    want = ops.masked_blend(x, s, lm)
    fx, vx, ok_x = _window(x, shift)
    fs, vs, ok_s = _window(s, shift)
    fl, vl, ok_l = _window(lm, shift)
    fy, vy, ok_y = _window(torch.zeros_like(x), shift)
    assert (vx.data_ptr() % 16 == 0) == (shift == 0)
    _c_blend(vx, vs, vl, vy)
    torch.cuda.synchronize()
    assert torch.equal(vy, want), "blend differs inside frames"
    assert ok_x() and ok_s() and ok_l() and ok_y() and torch.equal(vx, x) and torch.equal(vs, s) and torch.equal(vl, lm)
    _c_blend(vx, vs, vl, vx)
    torch.cuda.synchronize()
    assert torch.equal(vx, want) and ok_x() and ok_s() and ok_l(), "in place inside frames"


# ------------------------------------------------------------------------------------------------ mini pipeline, 4 steps
FR, HW_, STEPS, G = 4, 8, 4, 9.0
ETA, PHI = 0.5, 0.7


@pytest.fixture(scope="module")
def clip():
    """One mini model, one clip, its inversion, the unmasked edits -- shared, unchanged, by the pipeline tests below."""
    import gpu_checks as gc
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMInverseScheduler
    native, _, ocfg = gc.build_pair("mini", 1234)
    inp = gc.config1_inputs(ocfg, 3, FR, HW_)
    g = lambda x: x.half().cuda()
    c = types.SimpleNamespace(native=native, lat0=g(inp["sample"][:1]), ehs=g(inp["encoder_hidden_states"]), ie=g(inp["image_embeddings"]),
                              il=g(inp["image_latents"]))
    pipe = I2VGenXLPipeline(unet=native, scheduler=DDIMInverseScheduler())
    pipe._device = torch.device("cuda")
    c.traj = pipe.invert(prompt_embeds=c.ehs[:1], image_embeddings=c.ie[:1], image_latents=c.il[:1], height=HW_ * 8, width=HW_ * 8,
                         num_frames=FR, num_inference_steps=STEPS, guidance_scale=1.0, target_fps=8, latents=c.lat0, return_trajectory=True)
    c.T = max(c.traj.keys())
    c.ts = sorted(c.traj.keys(), reverse=True)
    c.src = (c.lat0 + 0.5).contiguous()     # the caller's clean latent (not a trajectory entry: the last partner is told apart)
    os.environ["ANYV2V_NO_GRAPH"] = "0"
    c.plain_trace = {}
    c.plain = _edit(_pipe(c), c, trace=c.plain_trace)
    return c


def _pipe(c, phi=0.0):
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMScheduler
    pipe = I2VGenXLPipeline(unet=c.native, scheduler=DDIMScheduler())
    pipe._device = torch.device("cuda")
    pipe.enable_guidance_rescale(phi)
    return pipe


def _edit(pipe, c, eta=0.0, seed=0, trace=None, ratios=(0.5, 0.75, 1.0)):
    from anyv2v_amd import pnp_utils
    from anyv2v_amd.schedulers import DDIMScheduler
    sched = DDIMScheduler()
    sched.set_timesteps(STEPS)
    pipe.register_modules(scheduler=sched)
    k = lambda r: sched.timesteps[: int(STEPS * r)]
    pnp_utils.register_conv_injection(pipe, k(ratios[0]))
    pnp_utils.register_spatial_attention_pnp(pipe, k(ratios[1]))
    pnp_utils.register_temp_attention_pnp(pipe, k(ratios[2]))
    try:
        return pipe.sample_with_pnp(prompt_embeds=c.ehs[2:3], negative_prompt_embeds=c.ehs[1:2], image_embeddings=c.ie[2:3],
                                    image_latents=c.il[2:3], height=HW_ * 8, width=HW_ * 8, num_frames=FR, num_inference_steps=STEPS,
                                    guidance_scale=G, target_fps=8, eta=eta, generator=torch.Generator().manual_seed(seed),
                                    latents=c.traj[c.T].clone(), output_type="latent", ddim_init_latents_t_idx=0, ddim_inv_latents_path=c.traj,
                                    ddim_inv_prompt_embeds=c.ehs[:1], ddim_inv_image_embeddings=c.ie[:1], ddim_inv_image_latents=c.il[:1],
                                    latents_trace=trace).frames.clone()
    finally:
        pnp_utils.clear_time(pipe)


def _half_plane(Fm=1):
    m = torch.zeros(Fm, HW_ * 8, HW_ * 8)
    m[:, :, : HW_ * 4] = 1.0          # the left half is edited, the right half keeps the source
    return m


def test_all_ones_and_all_zeros_masks(clip, monkeypatch):
    """All ones: the blend selects the edit everywhere -- bit-equal to the unmasked edit at every traced step.  All zeros: every traced
    step is the trajectory entry of the next level, the final latents are ``source_latents``, bit for bit."""
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "0")
    pipe = _pipe(clip)
    pipe.enable_masked_edit(torch.ones(FR, HW_ * 8, HW_ * 8, dtype=torch.bool), clip.src)
    trace = {}
    out = _edit(pipe, clip, trace=trace)
    assert any(e.graphs and e.blend is not None for e in pipe._engines.values()), "no HIP graph with the blend was captured"
    assert list(trace) == list(clip.plain_trace) == clip.ts
    for t in trace:
        assert torch.equal(trace[t], clip.plain_trace[t]), f"all-ones mask differs from the unmasked edit after t = {t}"
    assert torch.equal(out, clip.plain)
    pipe.enable_masked_edit(torch.zeros(HW_ * 8, HW_ * 8), clip.src)
    trace = {}
    out = _edit(pipe, clip, trace=trace)
    for i, t in enumerate(clip.ts):
        want = clip.traj[clip.ts[i + 1]] if i + 1 < STEPS else clip.src
        assert torch.equal(trace[t], want), f"all-zeros mask: the latent after t = {t} is not the source at the next level"
    assert torch.equal(out, clip.src)


@pytest.mark.parametrize("ratios", [(0.5, 0.75, 1.0), (0.25, 0.25, 0.5)], ids=["three-branch", "with-source-free-steps"])
def test_half_plane_mask_keeps_the_source_bit_for_bit(clip, monkeypatch, ratios):
    """grow = 0, feather = 0: the latent mask is exactly 0 / 1; the kept half of the final latent is ``source_latents``, bit for bit,
    the edited half is not; also when the last steps run on the [negative, editing] engine."""
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "0")
    pipe = _pipe(clip)
    pipe.enable_masked_edit(_half_plane(), clip.src)
    out = _edit(pipe, clip, ratios=ratios)
    kept = slice(HW_ // 2, HW_)
    assert torch.equal(out[..., kept], clip.src[..., kept]), "outside the mask the result is not the source's bits"
    assert not torch.equal(out[..., : HW_ // 2], clip.src[..., : HW_ // 2]) and torch.isfinite(out.float()).all()
    if ratios[2] < 1.0:
        eng = next(e for e in pipe._engines.values() if e.blend is not None)
        assert eng.nosrc is not None and eng.nosrc.graphs and eng.nosrc.blend[0] is eng.blend[0] and eng.nosrc.blend[1] is eng.blend[1]


def test_graph_replay_equals_eager_with_eta_rescale_and_mask(clip, monkeypatch):
    """eta = 0.5 and guidance rescale 0.7 together with a grown, feathered per-frame mask: the latents after EVERY step under HIP graphs
    are bit-equal to ANYV2V_NO_GRAPH=1; the kept region far from the feather is the source; same seed, same bits."""
    from anyv2v_amd import ops
    mask = _half_plane(FR)
    mask[0] = 0.0                      # (frame 0 is kept whole: a per-frame mask, Fm = F)
    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("ANYV2V_NO_GRAPH", mode)
        pipe = _pipe(clip, PHI)
        pipe.enable_masked_edit(mask, clip.src, grow=1, feather=0.5)
        trace = {}
        out = _edit(pipe, clip, eta=ETA, seed=21, trace=trace)
        assert any(bool(e.graphs) for e in pipe._engines.values()) == (mode == "0")
        runs[mode] = (out, trace, _edit(pipe, clip, eta=ETA, seed=21))
    (g_out, g_trace, g_again), (e_out, e_trace, _) = runs["0"], runs["1"]
    assert list(g_trace) == list(e_trace) == clip.ts
    for t in g_trace:
        assert torch.equal(g_trace[t], e_trace[t]), f"HIP graphs differ from ANYV2V_NO_GRAPH=1 after the step at t = {t}"
    assert torch.equal(g_out, e_out) and torch.equal(g_again, g_out) and torch.isfinite(g_out.float()).all()
    lm = ops.latent_mask(mask.half().cuda(), 1, 0.5)
    kept = (lm == 0)[None, None].expand(g_out.shape)
    assert bool(kept[0, 0, 0].all()) and int(kept.sum()) > kept[0, 0, 0].numel() * 4, "the test's mask keeps nothing beyond frame 0"
    assert torch.equal(g_out[kept], clip.src[kept]), "outside the mask the result is not the source's bits"
    assert float((g_out.float() - clip.plain.float()).abs().max()) > 1e-2, "the options do not move the sample"


def test_setter_off_is_the_parent_path(clip, monkeypatch):
    """Without a mask neither op is reached and no engine carries blend buffers; a pipeline that had a mask and cleared it gives the
    bits of one that never had."""
    from anyv2v_amd import ops
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "0")
    calls = []
    for name in ("latent_mask", "masked_blend"):
        inner = getattr(ops, name)
        monkeypatch.setattr(ops, name, (lambda inner, name: lambda *a, **k: (calls.append(name), inner(*a, **k))[1])(inner, name))
    never_pipe = _pipe(clip)
    never = _edit(never_pipe, clip, ratios=(0.25, 0.25, 0.5))
    assert calls == [], "the default path reached a masked-edit op"
    engines = list(never_pipe._engines.values()) + [e.nosrc for e in never_pipe._engines.values() if e.nosrc is not None]
    assert len(engines) == 2 and all(e.blend is None for e in engines), "an engine without a mask carries blend buffers"
    assert not any(isinstance(x, tuple) and x and x[0] == "blend" for k in never_pipe._engines for x in k)
    pipe = _pipe(clip)
    pipe.enable_masked_edit(_half_plane(), clip.src)
    on = _edit(pipe, clip, ratios=(0.25, 0.25, 0.5))
    assert calls.count("latent_mask") == 1 and "masked_blend" in calls
    pipe.disable_masked_edit()
    calls.clear()
    after = _edit(pipe, clip, ratios=(0.25, 0.25, 0.5))
    assert calls == [] and torch.equal(after, never) and not torch.equal(on, never)


def test_source_cache_replays_bit_equal_with_a_mask(clip, monkeypatch):
    """Multi-edit job with a mask on: the first edit records the source features, the second replays them ([negative, editing] only) --
    both bit-equal to the uncached masked edit (the source branch never sees the edit latent, blended or not)."""
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "0")
    ref = _pipe(clip)
    ref.enable_masked_edit(_half_plane(), clip.src, grow=1, feather=1.0)
    want = _edit(ref, clip)
    pipe = _pipe(clip)
    cache = pipe.enable_source_cache(True)
    pipe.enable_masked_edit(_half_plane(), clip.src, grow=1, feather=1.0)
    first = _edit(pipe, clip)
    assert cache.recorded_steps > 0 and cache.replayed_steps == 0
    second = _edit(pipe, clip)
    assert cache.replayed_steps > 0
    assert torch.equal(first, want), "recording masked edit differs from the uncached one"
    assert torch.equal(second, want), "replayed masked edit differs from the uncached one"
    assert not torch.equal(want, clip.plain)
