"""FreeU on the GPU, every call through the C ABI: the kernel against the fp64 ``torch.fft`` definition on the same fp16 inputs, the mini
UNet against the hooked CPU oracle (calibrated bound of ``gpu_checks``), and the mini pipeline (HIP graphs, engine cache, multi-edit
source-feature cache).  tests/freeu_spec.py holds the definition."""
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

FREEU = (0.9, 0.2, 1.2, 1.4)   # s1, s2, b1, b2
B_, S_ = 1.4, 0.2
# (n_img, H, W, C_hidden, C_skip, leading dimension > C on the inputs as well)
CASES = [(3, 8, 8, 128, 128, False), (2, 16, 16, 1280, 1280, False), (2, 5, 7, 64, 72, False), (1, 22, 40, 64, 64, False),
         (2, 1, 1, 256, 256, False), (1, 2, 2, 16, 8, False), (2, 5, 7, 64, 72, True)]


def _case_id(c):
    return f"{c[0]}x{c[1]}x{c[2]} C{c[3]}+{c[4]}" + (" ld>C" if c[5] else "")


@pytest.mark.parametrize("case", CASES, ids=[_case_id(c) for c in CASES])
def test_kernel_vs_fp64_fft_definition(case):
    """skip': |y - ref| <= 2^-10 |ref| + 1e-5 max |x| (one fp16 ulp for the single final rounding plus the fp32 accumulation error of
    <= 1024-term sums) against the fp64 torch.fft definition on the same fp16 inputs (1.5 randn + 2: the mean makes the correction
    matter); hidden': bit-equal to fp16(float(x) * b) on the first half of the channels and to x on the other; nothing outside
    [rows, C] of the framed outputs changes; two runs are bit-equal."""
    import freeu_spec as spec
    import gpu_checks as gc
    from anyv2v_amd import ops
    n_img, H, W, Ch, Cs, strided = case
    rows = n_img * H * W
    g = torch.Generator().manual_seed(1000 * H + W)
    hidden = (1.5 * torch.randn(rows, Ch, generator=g) + 2).half()
    skip = (1.5 * torch.randn(rows, Cs, generator=g) + 2).half()
    ref_h, ref_s = spec.freeu_tokens_reference(hidden, skip, n_img, H, W, B_, S_, dtype=torch.float64)
    if strided:
        _, dh, _ = gc._framed_like(hidden.cuda())
        _, ds, _ = gc._framed_like(skip.cuda())
        assert dh.stride(0) > Ch and ds.stride(0) > Cs
    else:
        dh, ds = hidden.cuda(), skip.cuda()
    buf_h, out_h, frame_h = gc._framed(rows, Ch)
    buf_s, out_s, frame_s = gc._framed(rows, Cs)
    assert out_h.stride(0) > Ch and out_s.stride(0) > Cs
    ops.freeu(dh, ds, n_img, H, W, B_, S_, out=(out_h, out_s))
    torch.cuda.synchronize()
    assert gc._frame_intact(buf_h, frame_h) and gc._frame_intact(buf_s, frame_s), "the kernel wrote outside [rows, C]"
    assert torch.equal(dh.cpu(), hidden) and torch.equal(ds.cpu(), skip), "out of place: the inputs changed"
    got_h, got_s = out_h.cpu(), out_s.cpu()
    assert torch.equal(got_h[:, :Ch // 2], (hidden[:, :Ch // 2].float() * B_).half()), "backbone half is not fp16(float(x) * b)"
    assert torch.equal(got_h[:, Ch // 2:], hidden[:, Ch // 2:]), "the other half of the backbone changed"
    assert torch.equal(got_h, ref_h)
    assert torch.isfinite(got_s.float()).all()
    bound = 2.0 ** -10 * ref_s.abs() + 1e-5 * float(skip.float().abs().max())
    ratio = float(((got_s.double() - ref_s).abs() / bound).max())
    moved = float((ref_s - skip.double()).abs().max())
    print(f"[freeu] {_case_id(case)}: max |y - ref| / bound = {ratio:.3f}; the filter moves the skip by up to {moved:.3f}")
    assert ratio <= 1.0
    assert moved > 0.5, "the correction is too small for this comparison to say anything"
    h2, s2 = ops.freeu(dh, ds, n_img, H, W, B_, S_)   # fresh contiguous outputs
    assert h2.is_contiguous() and s2.is_contiguous()
    assert torch.equal(h2.cpu(), got_h) and torch.equal(s2.cpu(), got_s), "two runs differ"


def test_result_does_not_depend_on_the_images_around():
    """A [negative, editing] step computes, bit for bit, what the three-branch step computes for those images."""
    from anyv2v_amd import ops
    g = torch.Generator().manual_seed(5)
    hidden = (1.5 * torch.randn(3 * 48, 256, generator=g) + 2).half().cuda()
    skip = (1.5 * torch.randn(3 * 48, 128, generator=g) + 2).half().cuda()
    h3, s3 = ops.freeu(hidden, skip, 6, 4, 6, B_, S_)
    h2, s2 = ops.freeu(hidden[48:], skip[48:], 4, 4, 6, B_, S_)
    assert torch.equal(h2, h3[48:]) and torch.equal(s2, s3[48:])


def _assert_all(results):
    for r in results:
        print(f"{'PASS' if r['ok'] else 'FAIL'} {r['name']}: err {r['err']:.3e} (tol {r['tol']:.1e})")
    bad = [r["name"] for r in results if not r["ok"]]
    assert not bad, bad


def test_mini_unet_with_freeu_vs_hooked_cpu_oracle():
    """B = 3, F = 2, latent 24 x 40 (up_blocks[0] at 3 x 5, up_blocks[1] at 6 x 10), without hooks and with all PnP hooks at t = 981: HIP
    against the fp32 CPU oracle with the torch.fft definition hooked in; bound = 2 x the error of the same hooked oracle run in eager
    fp16 on this GPU (``gpu_checks._calibrated``; its filter is the closed form in fp32, torch.fft runs on the CPU only)."""
    import freeu_spec as spec
    import gpu_checks as gc
    from anyv2v_amd import pnp_utils
    from oracle import pnp_oracle
    m = gc.full_models("mini", 1234, want=("native", "ocpu", "o16"))
    native, ocpu, o16 = m["native"], m["ocpu"], m["o16"]
    inp = gc.config1_inputs(m["ocfg"], 3, 2, (24, 40))
    inp16 = {k: (v.half() if v.is_floating_point() else v) for k, v in inp.items()}
    kw_o, kw_n = gc._cond_kw(inp16, "cpu", torch.float32), gc._cond_kw(inp16, "cuda", torch.float16)
    smp = inp16["sample"].cuda()

    def compare(name, t):
        with torch.no_grad():
            vo = ocpu(inp16["sample"].float(), t, **kw_o)[0]
            v16 = o16(smp, t, **kw_n)[0]
        vn = native(smp, t, **kw_n)[0]
        torch.cuda.synchronize()
        return gc._calibrated(name, vn, vo, v16), vn.float().cpu()

    v_off = native(smp, 981, **kw_n)[0].float().cpu()
    handles = spec.hook_oracle(ocpu, *FREEU) + spec.hook_oracle(o16, *FREEU)
    native.enable_freeu(*FREEU)
    try:
        r0, v_on = compare("unet mini B3 F2 24x40 + FreeU vs hooked oracle", 981)
        moved = gc._rel(v_on, v_off)
        print(f"[freeu] FreeU on vs off: max {moved[0]:.3e} l2 {moved[1]:.3e}")
        assert moved[0] > r0["tol"] and moved[1] > r0["tol_l2"], "FreeU moves the prediction by less than the bound: the comparison would be vacuous"
        pipe = gc._hook_all(m, ("ocpu", "o16"))
        try:
            pnp_utils.register_time(pipe, 981)
            pnp_oracle.register_time(ocpu, 981)
            pnp_oracle.register_time(o16, 981)
            r1, _ = compare("unet mini B3 F2 24x40 + FreeU + PnP hooks t=981 vs hooked oracle", 981)
        finally:
            gc._unhook_all(m, ("ocpu", "o16"), pipe)
    finally:
        native.disable_freeu()
        for h in handles:
            h.remove()
    _assert_all([r0, r1])
    assert torch.equal(native(smp, 981, **kw_n)[0].float().cpu(), v_off), "after disable_freeu: not bit-equal to never enabled"


# ------------------------------------------------------------------------------------------------ mini pipeline, 4 steps
FR, HW_, STEPS = 4, 8, 4   # 8 x 8 latents: up_blocks[0] works on 1 x 1 images (the wrapped slice), up_blocks[1] on 2 x 2


@pytest.fixture(scope="module")
def clip():
    """One mini model, one clip, its inversion (FreeU off) -- shared, unchanged, by the pipeline tests below."""
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
    yield c
    native.disable_freeu()


def _pipe(c):
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMScheduler
    pipe = I2VGenXLPipeline(unet=c.native, scheduler=DDIMScheduler())
    pipe._device = torch.device("cuda")
    return pipe


def _sample(pipe, c):
    return pipe(prompt_embeds=c.ehs[2:3], negative_prompt_embeds=c.ehs[1:2], image_embeddings=c.ie[2:3], image_latents=c.il[2:3],
                height=HW_ * 8, width=HW_ * 8, num_frames=FR, num_inference_steps=STEPS, guidance_scale=9.0, target_fps=8,
                latents=c.traj[c.T].clone(), output_type="latent", ddim_init_latents_t_idx=0).frames.clone()


def _edit(pipe, c, ratios=(0.5, 0.75, 1.0)):
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
                                    guidance_scale=9.0, target_fps=8, latents=c.traj[c.T].clone(), output_type="latent",
                                    ddim_init_latents_t_idx=0, ddim_inv_latents_path=c.traj, ddim_inv_prompt_embeds=c.ehs[:1],
                                    ddim_inv_image_embeddings=c.ie[:1], ddim_inv_image_latents=c.il[:1]).frames.clone()
    finally:
        pnp_utils.clear_time(pipe)


@pytest.mark.parametrize("loop", ["__call__", "sample_with_pnp"])
def test_pipeline_graphs_engine_cache_and_disable(clip, loop, monkeypatch):
    """One pipeline: off -> enable -> on -> disable -> off again.  FreeU on differs from off; after disable_freeu the run is bit-equal
    to the one before enable_freeu (the engine captured under FreeU is not replayed); FreeU on under HIP graphs is bit-equal to
    ANYV2V_NO_GRAPH=1."""
    run = _sample if loop == "__call__" else _edit
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "0")
    pipe = _pipe(clip)
    try:
        before = run(pipe, clip)
        pipe.enable_freeu(*FREEU)
        on_graph = run(pipe, clip)
        assert torch.equal(run(pipe, clip), on_graph), "the engine kept under FreeU does not replay to the same latents"
        pipe.disable_freeu()
        after = run(pipe, clip)
        assert torch.isfinite(on_graph.float()).all()
        d = float((on_graph.float() - before.float()).abs().max())
        print(f"[freeu] {loop}: FreeU on vs off max |diff| {d:.3e}")
        assert d > 1e-2, "FreeU on equals FreeU off"
        assert torch.equal(after, before), "after disable_freeu: not bit-equal to the run before enable_freeu"
        monkeypatch.setenv("ANYV2V_NO_GRAPH", "1")
        eager = _pipe(clip)
        eager.enable_freeu(*FREEU)
        on_eager = run(eager, clip)
        assert torch.equal(on_graph, on_eager), "FreeU on: HIP graphs differ from ANYV2V_NO_GRAPH=1"
    finally:
        clip.native.disable_freeu()


def test_source_cache_does_not_replay_features_recorded_under_another_setting(clip, monkeypatch):
    """Multi-edit job with the source-feature cache: first edit with FreeU off (records), enable_freeu, second edit -- it must not
    replay the stale features: bit-equal to a fresh pipeline with FreeU on.  A third edit then replays what the second recorded."""
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "0")
    pipe = _pipe(clip)
    try:
        cache = pipe.enable_source_cache(True)
        _edit(pipe, clip)
        assert cache.recorded_steps > 0 and cache.replayed_steps == 0
        pipe.enable_freeu(*FREEU)
        assert cache.steps == {}
        second = _edit(pipe, clip)
        assert cache.replayed_steps == 0, "features recorded with FreeU off were replayed"
        third = _edit(pipe, clip)
        assert cache.replayed_steps > 0
        fresh = _pipe(clip)
        assert fresh.unet.freeu == FREEU
        want = _edit(fresh, clip)
        assert torch.equal(second, want), "second edit differs from a fresh pipeline with FreeU on"
        assert torch.equal(third, want), "replayed edit differs from a fresh pipeline with FreeU on"
    finally:
        clip.native.disable_freeu()
