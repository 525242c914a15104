"""Automatic edit masks on the GPU, the kernels through the C ABI: the accumulate launch bit-equal to an fp32 torch restatement, the finish
launch against the fp64 definition (tests/auto_mask_spec.py) on the same inputs, both inside NaN-poisoned frames (aligned, and offset so
that the scalar path runs), and the mini pipeline (HIP graphs against ANYV2V_NO_GRAPH=1, both variants, the generated mask driving the
masked edit).

Bounds: the accumulator bit-equal; the soft map within 1 fp16 ulp of the definition rounded to fp16 (the fp32 / fp64 error of the mean
and of the quotient is orders of magnitude below half an fp16 ulp, so only ties can move); the binary mask the exact function of the
returned map, the pixel mask its exact 8 x 8 replication.  No claim is made about WHERE the mask lies on a randomly initialised UNet."""
import os
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

POISON16, POISON32 = 0x7E5A, 0x7FC5A5A5      # NaN bit patterns no kernel computes (tests/gpu_checks.py)
SHAPES = [(1, 1, 1), (3, 5, 5), (1, 8, 8), (3, 3, 16), (2, 9, 7), (5, 64, 64)]
IDS = ["x".join(map(str, s)) for s in SHAPES]
C = 4


def _seed(shape):
    from test_auto_mask_host import GPU_SEEDS   # (one table: the host test asserts the near-threshold share of exactly these inputs)
    return GPU_SEEDS[shape]


def _window(t, shift=0, pad=64):
    """``t`` copied into a contiguous window of a NaN-poisoned allocation, ``shift`` elements behind a 16-byte boundary (0: aligned;
    1: no 16-byte access can be aligned) -> (buffer, view, check) with ``check()`` true while everything outside the window is intact."""
    item = t.element_size()
    idt, bits = {1: (torch.uint8, 0xA5), 2: (torch.int16, POISON16), 4: (torch.int32, POISON32)}[item]
    n, lo = t.numel(), pad + shift
    buf = torch.full((lo + n + pad,), bits, dtype=idt, device="cuda")
    assert buf.data_ptr() % 16 == 0 and (pad * item) % 16 == 0
    view = buf.view(t.dtype)[lo:lo + n].view(t.shape)
    view.copy_(t)
    return buf, view, lambda: bool((buf[:lo] == bits).all() and (buf[lo + n:] == bits).all())


def _tokens(vs, vt, ldv):
    """(v_src, v_tgt) fp16 [C, n] -> the UNet's token layout [2 n, ldv] on the host, the padding columns C .. ldv - 1 poisoned."""
    n = vs.shape[1]
    tok = torch.full((2 * n, ldv), POISON16, dtype=torch.int16).view(torch.float16)
    tok[:n, :C], tok[n:, :C] = vs.t(), vt.t()
    return tok


def _c_accum(tok, ldv, F, HW, acc, first, flag=None):
    from anyv2v_amd import _lib
    _lib.check(_lib.load().anyv2v_diff_map_accum_f16(tok.data_ptr(), ldv, C, F, HW, acc.data_ptr(), int(first), None if flag is None else flag.data_ptr(),
                                                    torch.cuda.current_stream().cuda_stream), "anyv2v_diff_map_accum_f16")


def _c_finish(acc, F, h, w, ratio, thr, rec, m, pm):
    from anyv2v_amd import _lib
    _lib.check(_lib.load().anyv2v_diff_map_finish_f16(acc.data_ptr(), F, h, w, ratio, thr, rec.data_ptr(), m.data_ptr(), pm.data_ptr(),
                                                     torch.cuda.current_stream().cuda_stream), "anyv2v_diff_map_finish_f16")


# ------------------------------------------------------------------------------------------------ accumulate
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "offset"])
@pytest.mark.parametrize("ldv", [4, 8, 320])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_accumulate_bit_equal_inside_poisoned_frames(shape, ldv, shift):
    """Three maps, the first overwriting a NaN-poisoned accumulator and two adding to it: bit-equal to ``(a.float() - b.float()).abs()`` with
    channels added in order, in fp32.  +-65504, subnormals and equal values among the inputs; the token matrix (padding columns poisoned)
    and the accumulator are windows of NaN-filled allocations; the frames and the inputs are intact afterwards."""
    import auto_mask_spec as spec
    F, h, w = shape
    n = F * h * w
    pairs = spec.fixture(F, h, w, 3, _seed(shape), special=True)
    fa, acc, ok_a = _window(torch.zeros(n, dtype=torch.float32, device="cuda"), shift)
    acc.view(torch.int32).fill_(POISON32)                  # never read before the first map overwrites it
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    want = None
    for k, (vs, vt) in enumerate(pairs):
        tok = _tokens(vs, vt, ldv)
        ft, vtok, ok_t = _window(tok.cuda(), shift)
        if k == 2:                                          # the device flag of a captured graph; the host's value is then ignored
            flag.fill_(0)
            _c_accum(vtok, ldv, F, h * w, acc, 1, flag)
        else:
            _c_accum(vtok, ldv, F, h * w, acc, k == 0)
        torch.cuda.synchronize()
        d = (vt.float() - vs.float()).abs()
        s = torch.zeros(n)
        for c in range(C):
            s = s + d[c]
        want = s if want is None else want + s
        assert torch.equal(acc.cpu().view(torch.int32), want.view(torch.int32)), f"map {k}"
        assert ok_t() and ok_a() and torch.equal(vtok.cpu().view(torch.int16), tok.view(torch.int16)), "a frame or the input changed"
    assert torch.equal(want, spec.generate([(a.view(C, F, h, w), b.view(C, F, h, w)) for a, b in pairs], 3.0, 0.5)[2].view(-1))
    # the device flag set: overwrite, whatever the accumulator held
    flag.fill_(1)
    _c_accum(vtok, ldv, F, h * w, acc, 0, flag)
    torch.cuda.synchronize()
    assert torch.equal(acc.cpu(), s) and ok_a()


# ------------------------------------------------------------------------------------------------ finish
def _finish_case(acc_host, F, h, w, ratio, thr, shift):
    fa, acc, ok_a = _window(acc_host.cuda(), shift)
    fr, rec, ok_r = _window(torch.zeros(64, dtype=torch.float32, device="cuda"), shift)
    fm, m, ok_m = _window(torch.zeros(F, h, w, dtype=torch.float16, device="cuda"), shift)
    fp, pm, ok_p = _window(torch.zeros(F, 8 * h, 8 * w, dtype=torch.uint8, device="cuda"), shift)
    _c_finish(acc, F, h, w, ratio, thr, rec, m, pm)
    torch.cuda.synchronize()
    assert ok_a() and ok_r() and ok_m() and ok_p(), "a frame changed"
    assert torch.equal(acc.cpu().view(torch.int32), acc_host.view(torch.int32)), "the accumulator changed"
    return m.cpu(), pm.cpu(), rec.cpu()


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "offset-scalar-path"])
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_finish_against_the_definition(shape, shift):
    """The soft map within 1 fp16 ulp of the fp64 definition rounded to fp16; the binary mask EXACTLY ``map > fp16(threshold)`` on the returned
    map, the pixel mask its exact 8 x 8 replication; the mask equals the definition's wherever the definition's map is more than 1 fp16 ulp
    from the threshold (at most 1 % is left out: tests/test_auto_mask_host.py asserts that share for these inputs).  w % 8 == 0 and aligned:
    the 16-byte kernel; (2, 9, 7) and every offset window: the scalar one.  Also: all-zero accumulator (mean == 0), every value clamped,
    and two runs bit-equal.  Measured on an MI355X (printed by this test): 0 fp16 ulp on every shape, both paths."""
    import auto_mask_spec as spec
    from sampler_options_spec import ulp_distance_fp16
    F, h, w = shape
    n = F * h * w
    acc = None
    for a, b in spec.fixture(F, h, w, 3, _seed(shape), special=False):
        acc = spec.accumulate(a, b, acc)
    worst = 0
    for ratio, thr in ((3.0, 0.5), (1.0, 0.3)):
        m64, m16, mask = spec.finish(acc.view(F, h, w), ratio, thr)
        m, pm, rec = _finish_case(acc, F, h, w, ratio, thr, shift)
        d = ulp_distance_fp16(m, m16)
        worst = max(worst, d)
        assert d <= 1, (ratio, thr, d)
        got = m > torch.tensor(thr).half()
        assert torch.equal(pm, spec.pixel_mask(got).to(torch.uint8)), "the pixel mask is not the 8 x 8 replication of map > threshold"
        near = spec.near_threshold(m64, thr)
        assert int(near.sum()) <= 0.01 * n and torch.equal(got[~near], mask[~near])
        m2, pm2, rec2 = _finish_case(acc, F, h, w, ratio, thr, shift)
        assert torch.equal(m2.view(torch.int16), m.view(torch.int16)) and torch.equal(pm2, pm) and torch.equal(rec2.view(torch.int32), rec.view(torch.int32))
        assert abs(float(rec.double().sum()) - float(acc.double().sum())) <= 1e-5 * float(acc.double().sum())
    print(f"[auto-mask] finish {shape} shift {shift}: map at most {worst} fp16 ulp from the rounded definition")
    # mean == 0: an empty mask, a zero map, no NaN
    m, pm, _ = _finish_case(torch.zeros(n), F, h, w, 3.0, 0.5, shift)
    assert float(m.abs().max()) == 0.0 and int(pm.sum()) == 0 and not bool(torch.isnan(m).any())
    # every value clamped: a constant accumulator with ratio 3 -> map 1 everywhere, mask full
    m, pm, _ = _finish_case(torch.full((n,), 0.75), F, h, w, 3.0, 0.5, shift)
    assert float(m.min()) == 1.0 and int(pm.sum()) == 64 * n


def test_ops_wrappers_match_the_c_abi():
    """``ops.diff_map_accum`` / ``ops.diff_map_finish`` (the allocating wrappers the pipeline calls) on a token matrix of width 8."""
    import auto_mask_spec as spec
    from anyv2v_amd import ops
    F, h, w = 3, 3, 16
    pairs = spec.fixture(F, h, w, 2, 5, special=False)
    acc = torch.empty(F * h * w, dtype=torch.float32, device="cuda")
    flag = torch.ones(1, dtype=torch.int32, device="cuda")
    for k, (a, b) in enumerate(pairs):
        flag.fill_(1 if k == 0 else 0)
        ops.diff_map_accum(_tokens(a, b, 8).cuda(), C, F, h * w, acc, flag)
    want = spec.generate([(a.view(C, F, h, w), b.view(C, F, h, w)) for a, b in pairs], 3.0, 0.5)
    assert torch.equal(acc.cpu(), want[2].view(-1))
    m, pm = ops.diff_map_finish(acc, F, h, w, 3.0, 0.5)
    assert pm.dtype == torch.bool and tuple(pm.shape) == (F, 8 * h, 8 * w) and torch.equal(pm.cpu(), spec.pixel_mask(m.cpu() > 0.5))


# ------------------------------------------------------------------------------------------------ mini pipeline, 4 steps
FR, HW_, STEPS, G = 4, 8, 4, 9.0


@pytest.fixture(scope="module")
def clip():
    """One mini model, one clip, its inversion, the unmasked edit -- shared, unchanged, by the pipeline tests below."""
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
    c.src = (c.lat0 + 0.5).contiguous()
    os.environ["ANYV2V_NO_GRAPH"] = "0"
    c.plain = _edit(_pipe(c), c)
    return c


def _pipe(c):
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMScheduler
    pipe = I2VGenXLPipeline(unet=c.native, scheduler=DDIMScheduler())
    pipe._device = torch.device("cuda")
    return pipe


def _edit(pipe, c):
    from anyv2v_amd import pnp_utils
    from anyv2v_amd.schedulers import DDIMScheduler
    sched = DDIMScheduler()
    sched.set_timesteps(STEPS)
    pipe.register_modules(scheduler=sched)
    k = lambda r: sched.timesteps[: int(STEPS * r)]
    pnp_utils.register_conv_injection(pipe, k(0.5))
    pnp_utils.register_spatial_attention_pnp(pipe, k(0.75))
    pnp_utils.register_temp_attention_pnp(pipe, k(1.0))
    try:
        return pipe.sample_with_pnp(prompt_embeds=c.ehs[2:3], negative_prompt_embeds=c.ehs[1:2], image_embeddings=c.ie[2:3],
                                    image_latents=c.il[2:3], height=HW_ * 8, width=HW_ * 8, num_frames=FR, num_inference_steps=STEPS,
                                    guidance_scale=G, target_fps=8, generator=torch.Generator().manual_seed(0),
                                    latents=c.traj[c.T].clone(), output_type="latent", ddim_init_latents_t_idx=0, ddim_inv_latents_path=c.traj,
                                    ddim_inv_prompt_embeds=c.ehs[:1], ddim_inv_image_embeddings=c.ie[:1], ddim_inv_image_latents=c.il[:1]).frames.clone()
    finally:
        pnp_utils.clear_time(pipe)


def _generate(pipe, c, same=False, **kw):
    e = 0 if same else 2
    return pipe.generate_edit_mask(prompt_embeds=c.ehs[e:e + 1], image_embeddings=c.ie[e:e + 1], image_latents=c.il[e:e + 1],
                                   ddim_inv_prompt_embeds=c.ehs[:1], ddim_inv_image_embeddings=c.ie[:1], ddim_inv_image_latents=c.il[:1],
                                   height=HW_ * 8, width=HW_ * 8, num_frames=FR, target_fps=8, num_inference_steps=STEPS, **kw)


def _check_against_trace(pm, trace, ratio, thr):
    """The mask is the definition evaluated on the traced accumulator (1 fp16 ulp on the map, the mask wherever the map is not within 1 ulp
    of the threshold), the exact function of the returned map, and its exact replication."""
    import auto_mask_spec as spec
    from sampler_options_spec import ulp_distance_fp16
    m64, m16, mask = spec.finish(trace["acc"].cpu(), ratio, thr)
    assert ulp_distance_fp16(trace["map"].cpu(), m16) <= 1
    got = trace["map"].cpu() > torch.tensor(thr).half()
    near = spec.near_threshold(m64, thr)
    assert torch.equal(got[~near], mask[~near]) and torch.equal(pm.cpu(), spec.pixel_mask(got))
    return got


def test_pipeline_graphs_against_eager_and_the_definition(clip, monkeypatch):
    """Three maps from noise draws: HIP graphs (one captured graph replayed per map) against ANYV2V_NO_GRAPH=1 bit-equal in accumulator, map
    and mask; the same seed twice bit-equal; the mask is the definition on the traced accumulator; the generator ends where three
    ``draw_noise`` calls end."""
    from anyv2v_amd.schedulers import DDIMScheduler
    runs = {}
    for mode in ("0", "1"):
        monkeypatch.setenv("ANYV2V_NO_GRAPH", mode)
        pipe = _pipe(clip)
        trace, gen = {}, torch.Generator().manual_seed(31)
        pm = _generate(pipe, clip, source_latents=clip.lat0, num_maps_per_mask=3, generator=gen, trace=trace, mask_thresholding_ratio=1.0)
        runs[mode] = (pm, trace, gen.get_state())
        assert pm.dtype == torch.bool and pm.is_cuda and tuple(pm.shape) == (FR, HW_ * 8, HW_ * 8) and pipe._masked_edit is None
    (g_pm, g_tr, g_state), (e_pm, e_tr, _) = runs["0"], runs["1"]
    assert torch.equal(g_tr["acc"].view(torch.int32), e_tr["acc"].view(torch.int32)), "HIP graphs differ from ANYV2V_NO_GRAPH=1 in the accumulator"
    assert torch.equal(g_tr["map"].view(torch.int16), e_tr["map"].view(torch.int16)) and torch.equal(g_pm, e_pm)
    got = _check_against_trace(g_pm, g_tr, 1.0, 0.5)
    assert 0 < int(got.sum()) < got.numel() and float(g_tr["acc"].min()) > 0.0
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "0")
    again, gen = {}, torch.Generator().manual_seed(31)
    pm2 = _generate(_pipe(clip), clip, source_latents=clip.lat0, num_maps_per_mask=3, generator=gen, trace=again, mask_thresholding_ratio=1.0)
    assert torch.equal(pm2, g_pm) and torch.equal(again["acc"].view(torch.int32), g_tr["acc"].view(torch.int32))
    sched, ref = DDIMScheduler(), torch.Generator().manual_seed(31)
    for _ in range(3):
        sched.draw_noise(clip.lat0, ref)
    assert torch.equal(g_state, ref.get_state()) and torch.equal(gen.get_state(), ref.get_state())


def test_pipeline_trajectory_variant_and_identical_conditioning(clip, monkeypatch):
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "0")
    pipe = _pipe(clip)
    trace = {}
    pm = _generate(pipe, clip, ddim_inv_latents_path=clip.traj, trace=trace, mask_thresholding_ratio=1.0)
    assert trace["timestep"] == 251 and len(trace["x_t"]) == 1 and torch.equal(trace["x_t"][0], clip.traj[251])
    _check_against_trace(pm, trace, 1.0, 0.5)
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "1")
    eager = {}
    pm_e = _generate(_pipe(clip), clip, ddim_inv_latents_path=clip.traj, trace=eager, mask_thresholding_ratio=1.0)
    assert torch.equal(pm_e, pm) and torch.equal(eager["acc"].view(torch.int32), trace["acc"].view(torch.int32))
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "0")
    same = {}
    empty = _generate(pipe, clip, same=True, source_latents=clip.lat0, num_maps_per_mask=2, generator=torch.Generator().manual_seed(1), trace=same)
    assert not bool(empty.any()) and float(same["acc"].abs().max()) == 0.0 and float(same["map"].abs().max()) == 0.0


def test_generated_mask_drives_the_masked_edit(clip, monkeypatch):
    """The generated mask handed to ``enable_masked_edit``: outside it the edit carries ``source_latents``' bits, inside an all-true mask it
    equals the unmasked edit (the assertions of tests/test_masked_edit_gpu.py, restated); ``ops.latent_mask`` of the result is the
    latent-size mask, bit for bit."""
    from anyv2v_amd import ops
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "0")
    pipe = _pipe(clip)
    trace = {}
    pm = _generate(pipe, clip, source_latents=clip.lat0, num_maps_per_mask=2, generator=torch.Generator().manual_seed(7), trace=trace,
                   mask_thresholding_ratio=1.0)
    lat_mask = trace["map"] > 0.5
    assert 0 < int(lat_mask.sum()) < lat_mask.numel()
    pipe.enable_masked_edit(pm, clip.src)
    assert torch.equal(ops.latent_mask(pipe._masked_edit["mask"].cuda()), lat_mask.half())
    out = _edit(pipe, clip)
    kept = (~lat_mask)[None, None].expand(out.shape)
    assert torch.equal(out[kept], clip.src[kept]), "outside the mask the result is not the source's bits"
    assert not torch.equal(out[~kept], clip.src[~kept]) and torch.isfinite(out.float()).all()
    # an all-true mask (a threshold every clamped value exceeds cannot be had: ratio large, threshold small)
    full = _generate(pipe, clip, source_latents=clip.lat0, num_maps_per_mask=1, generator=torch.Generator().manual_seed(7),
                     mask_thresholding_ratio=1000.0, threshold=0.001)
    assert bool(full.all())
    pipe.enable_masked_edit(full, clip.src)
    assert torch.equal(_edit(pipe, clip), clip.plain), "an all-true generated mask differs from the unmasked edit"
    pipe.disable_masked_edit()
