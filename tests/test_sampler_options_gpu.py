"""Stochastic DDIM (``eta``) and guidance rescale on the GPU, every call through the C ABI: the two kernels against the fp64 definitions
(tests/sampler_options_spec.py) on the same fp16 inputs, their bit-reproducibility (twice; inside NaN-poisoned frames), the default
path's bit-equality with ``cfg_ddim_step``, and the mini pipeline (HIP graphs against ANYV2V_NO_GRAPH=1, fresh noise every step, the
multi-edit source-feature cache)."""
import os
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ETA, PHI, G = 0.5, 0.7, 9.0


def _two_pass_shape():
    """Smallest 64 x 64 clip at which EVERY block of the statistics kernel's fixed grid makes two grid-stride passes: the pixel count
    reaches twice the grid's thread count (ANYV2V_GUIDANCE_STATS_BLOCKS x _THREADS)."""
    from anyv2v_amd import _lib
    threads = _lib.GUIDANCE_STATS_BLOCKS * _lib.GUIDANCE_STATS_THREADS
    frames = -(-2 * threads // (64 * 64))
    assert frames <= 16, "larger than the 16 x 64 x 64 workload latent"
    return (3, 4, frames, 64, 64)


SHAPES = {"one-block": (3, 4, 2, 8, 8), "n420": (3, 4, 3, 5, 7), "two-pass": None}
# (shape, prediction, b_unc, phi, eta of the row, noise operand): every prediction type, no guidance, phi in {0, 0.7, 1}, sigma = 0 with
# a null noise pointer, sigma > 0 -- across the three shapes
CASES = [("one-block", 0, 0, PHI, ETA, True), ("one-block", 1, 0, 1.0, 0.0, False), ("one-block", 2, -1, PHI, ETA, True),
         ("n420", 0, 0, 1.0, ETA, True), ("n420", 1, 0, PHI, ETA, True), ("n420", 2, 0, PHI, 0.0, False), ("n420", 0, 0, 0.0, ETA, True),
         ("n420", 0, -1, 0.0, 0.0, False),
         ("two-pass", 0, 0, PHI, ETA, True), ("two-pass", 2, 1, 1.0, 0.0, False), ("two-pass", 1, 0, 0.0, ETA, True)]


def _shape(name):
    return SHAPES[name] or _two_pass_shape()


def _operands(shape, seed=0):
    """vtok [(3 F) H W, 8] channels-last prediction of three branches (4 of 8 columns used, as the UNet's conv_out writes it), the latent,
    the noise: fp16 on the host."""
    nb, C, F, H, W = shape
    g = torch.Generator().manual_seed(1000 * F + H + seed)
    vtok = (torch.randn(nb * F * H * W, 8, generator=g) + 0.25).half()
    lat = torch.randn(1, C, F, H, W, generator=g).half()
    noise = torch.randn(1, C, F, H, W, generator=g).half()
    return vtok, lat, noise


def _row(eta, phi, n, t=501):
    from anyv2v_amd.schedulers import DDIMScheduler
    s = DDIMScheduler()
    s.set_timesteps(50)
    return s.coefficient_table([t], "cpu", eta=eta, phi=phi, n=n)[0] if (eta > 0 or phi > 0) else \
        torch.tensor(tuple(s.eta_coefficients(t, 0.0)) + (0.0, float(n), 0.0), dtype=torch.float32)


def _launch(vtok, lat, noise, row, b_unc, b_cond, pred, phi, out=None, stats=None):
    from anyv2v_amd import ops
    rescale = phi > 0 and b_unc >= 0
    if rescale:
        stats = ops.guidance_stats(vtok, b_unc, b_cond, G, lat.shape, out=stats)
    out = torch.empty_like(lat) if out is None else out
    ops.cfg_ddim_step_ex(vtok, b_unc, b_cond, G, row, lat, out, prediction=pred, stats=stats if rescale else None, phi=phi if rescale else 0.0,
                         noise=noise)
    return out, (stats if rescale else None)


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]} pred{c[1]} b_unc{c[2]} phi{c[3]} eta{c[4]}{' noise' if c[5] else ' null-noise'}" for c in CASES])
def test_kernels_vs_fp64_definition(case):
    """max |y - ref| <= KTOL x max |ref| (and the relative L2 error likewise) against the fp64 definition on the same fp16 inputs; a second
    launch gives the same records and the same result, bit for bit."""
    import gpu_checks as gc
    import sampler_options_spec as spec
    name, pred, b_unc, phi, eta, with_noise = case
    shape = _shape(name)
    b_cond = 2
    vtok, lat, noise = _operands(shape)
    n = lat.numel()
    row = _row(eta, phi, n)
    assert (float(row[4]) > 0) == (eta > 0)
    ref = spec.fused_step(vtok, b_unc, b_cond, G, [float(c) for c in row], lat, noise if with_noise else None, pred)
    dv, dl, dn, dr = vtok.cuda(), lat.cuda(), (noise.cuda() if with_noise else None), row.cuda()
    got, stats = _launch(dv, dl, dn, dr, b_unc, b_cond, pred, phi)
    got2, stats2 = _launch(dv, dl, dn, dr, b_unc, b_cond, pred, phi)
    torch.cuda.synchronize()
    r = gc._res(f"sampler step {case}", got.cpu(), ref, gc.KTOL)
    print(f"[sampler] {name} pred {pred} b_unc {b_unc} phi {phi} eta {eta}: max {r['err']:.3e} l2 {r['l2']:.3e} (KTOL {gc.KTOL})")
    assert r["ok"], r
    assert torch.equal(got, got2), "two launches differ"
    assert (stats is None) == (not (phi > 0 and b_unc >= 0))
    if stats is not None:
        assert torch.equal(stats, stats2), "the statistics records of two launches differ"
        rec = stats.cpu().view(-1, 8).double()
        txt = spec.branch_planar(vtok, b_cond, *shape[1:]).double()
        cfg = spec.guided_fp16(spec.branch_planar(vtok, b_unc, *shape[1:]), spec.branch_planar(vtok, b_cond, *shape[1:]), G).double()
        for col, x in ((0, txt), (2, cfg)):
            k = float(rec[0, 4 + col // 2])
            assert (rec[:, 4 + col // 2] == k).all() and abs(k - float(x.reshape(-1)[0])) <= 2.0 ** -9 * abs(k)   # (the pivot: the first element)
            var = (float(rec[:, col + 1].sum()) - float(rec[:, col].sum()) ** 2 / n) / (n - 1)
            assert abs(var ** 0.5 - float(x.std())) <= 1e-4 * float(x.std()), "records do not fold to the unbiased standard deviation"
        assert float(rec[:, 6:].abs().max()) == 0.0


@pytest.mark.parametrize("name", list(SHAPES))
def test_operands_inside_nan_poisoned_frames(name):
    """Every operand a window of a NaN-filled allocation (``check_edges_*`` style): records and result bit-equal to the plain launch,
    every frame intact -- the kernels read nothing outside their operands and write nothing outside the latent / the records."""
    import gpu_checks as gc
    from anyv2v_amd import ops
    shape = _shape(name)
    vtok, lat, noise = _operands(shape, seed=1)
    row = _row(ETA, PHI, lat.numel())
    dv, dl, dn, dr = vtok.cuda(), lat.cuda(), noise.cuda(), row.cuda()
    plain, stats = _launch(dv, dl, dn, dr, 0, 2, 0, PHI)
    bufs = {}
    fv = gc._framed_like(dv[:, :4].contiguous())                # the 4 prediction columns as a window of a wider matrix (ldv > C)
    bufs["vtok"] = fv
    for key, t in (("lat", dl), ("noise", dn), ("row", dr)):
        bufs[key] = gc._framed_like(t, flat=True)
    fo = gc._framed(1, lat.numel())
    fs = gc._framed(1, ops.GUIDANCE_STATS_FLOATS, dtype=torch.float32, rows=1, cols=64)
    out = fo[1][0].view(lat.shape)
    got, stats_f = _launch(fv[1], bufs["lat"][1], bufs["noise"][1], bufs["row"][1], 0, 2, 0, PHI, out=out, stats=fs[1][0])
    torch.cuda.synchronize()
    assert torch.equal(stats_f, stats), "records differ inside frames"
    assert torch.equal(got, plain), "result differs inside frames"
    for key, (buf, _view, frame) in list(bufs.items()) + [("out", fo), ("records", fs)]:
        assert gc._frame_intact(buf, frame), f"the frame around {key} changed"
    assert torch.equal(fv[1], dv[:, :4]) and torch.equal(bufs["lat"][1], dl) and torch.equal(bufs["noise"][1], dn), "an input changed"


@pytest.mark.parametrize("name", list(SHAPES))
@pytest.mark.parametrize("b_unc", [0, -1])
def test_both_off_is_cfg_ddim_step_bit_for_bit(name, b_unc):
    """phi = 0, sigma = 0, no noise operand: the new step kernel reproduces ``anyv2v_cfg_ddim_step_f16`` bit for bit; with a noise
    operand and sigma = 0 as well; in place (out aliasing lat) as the engine calls it."""
    from anyv2v_amd import ops
    from anyv2v_amd.schedulers import DDIMScheduler
    shape = _shape(name)
    vtok, lat, noise = _operands(shape, seed=2)
    s = DDIMScheduler()
    s.set_timesteps(50)
    for t in (981, 501, 1):
        coef = s.coefficient_table([t], "cuda")[0]
        row = _row(0.0, 0.0, lat.numel(), t).cuda()
        assert torch.equal(row[:4], coef)
        dv, dl = vtok.cuda(), lat.cuda()
        want = ops.cfg_ddim_step(dv, b_unc, 2, G, coef, dl, torch.empty_like(dl))
        got, _ = _launch(dv, dl, None, row, b_unc, 2, 0, 0.0)
        assert torch.equal(got, want), (name, b_unc, t)
        got_n, _ = _launch(dv, dl, noise.cuda(), row, b_unc, 2, 0, 0.0)
        assert torch.equal(got_n, want), "sigma = 0 with a noise operand"
        inplace = dl.clone()
        _launch(dv, inplace, None, row, b_unc, 2, 0, 0.0, out=inplace)
        assert torch.equal(inplace, want), "in place"


def test_distance_to_the_references_own_fp16_rescale():
    """The rescaled guided prediction itself (sample prediction with c_x0 = 1, c_eps = 0: the kernel's output IS fp16(g')) against what
    the reference's ``rescale_noise_cfg`` returned on fp16 tensors (fixture): KTOL against the fp64 definition is the assertion; the
    largest fp16-ulp distance to the reference's fp16 result is measured and printed (profiles/sampler_options_parity.md)."""
    import gpu_checks as gc
    import sampler_options_spec as spec
    from anyv2v_amd import ops
    fx = torch.load(os.path.join(ROOT, "tests", "golden", "sampler_options_ref.pt"))
    for r in fx["rescale"]:
        if r["noise_cfg"].shape[0] != 1:
            continue
        _, C, F, H, W = r["noise_cfg"].shape
        tok = lambda x: x[0].permute(1, 2, 3, 0).reshape(-1, C)
        vtok = torch.zeros(2 * F * H * W, 8, dtype=torch.float16)
        vtok[:F * H * W, :C], vtok[F * H * W:, :C] = tok(r["noise_pred_uncond"]), tok(r["noise_pred_text"])
        phi, n = r["guidance_rescale"], r["noise_cfg"].numel()
        row = torch.tensor((0.0, 1.0, 1.0, 0.0, 0.0, phi, n, 0.0), dtype=torch.float32).cuda()
        lat = torch.zeros_like(r["noise_cfg"]).cuda()
        dv = vtok.cuda()
        stats = ops.guidance_stats(dv, 0, 1, fx["guidance"], lat.shape) if phi > 0 else None
        got = ops.cfg_ddim_step_ex(dv, 0, 1, fx["guidance"], row, lat, torch.empty_like(lat), prediction=2, stats=stats, phi=phi).cpu()
        res = gc._res(f"rescaled prediction phi {phi}", got, r["out_fp64"], gc.KTOL)
        ulps = spec.ulp_distance_fp16(got, r["out_fp16"])
        ulps64 = spec.ulp_distance_fp16(got, r["out_fp64"].half())
        print(f"[sampler-parity] phi {phi} n {n}: vs fp64 definition max {res['err']:.3e}; {ulps} fp16 ulp from the reference's fp16 result, "
              f"{ulps64} from the rounded fp64 definition; the reference's fp16 result is {spec.ulp_distance_fp16(r['out_fp16'], r['out_fp64'].half())} from it")
        assert res["ok"], res
        if phi == 0.0:
            assert spec.ulp_distance_fp16(got, r["noise_cfg"]) <= 1   # (the guided prediction itself: v_fma_mix rounds g * diff once, torch twice)


# ------------------------------------------------------------------------------------------------ mini pipeline, 4 steps
FR, HW_, STEPS = 4, 8, 4


@pytest.fixture(scope="module")
def clip():
    """One mini model, one clip, its inversion -- shared, unchanged, by the pipeline tests below."""
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
    return c


def _pipe(c, phi=0.0):
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMScheduler
    pipe = I2VGenXLPipeline(unet=c.native, scheduler=DDIMScheduler())
    pipe._device = torch.device("cuda")
    pipe.enable_guidance_rescale(phi)
    return pipe


def _sample(pipe, c, eta=0.0, seed=0, trace=None):
    return pipe(prompt_embeds=c.ehs[2:3], negative_prompt_embeds=c.ehs[1:2], image_embeddings=c.ie[2:3], image_latents=c.il[2:3],
                height=HW_ * 8, width=HW_ * 8, num_frames=FR, num_inference_steps=STEPS, guidance_scale=G, target_fps=8, eta=eta,
                generator=torch.Generator().manual_seed(seed), latents=c.traj[c.T].clone(), output_type="latent", ddim_init_latents_t_idx=0,
                latents_trace=trace).frames.clone()


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


@pytest.mark.parametrize("loop", ["__call__", "sample_with_pnp"])
def test_graph_replay_equals_eager_and_every_step_gets_fresh_noise(clip, loop, monkeypatch):
    """eta = 0.5, phi = 0.7, 4 steps: the latents after EVERY step under HIP graphs are bit-equal to ANYV2V_NO_GRAPH=1; the noise buffer
    the captured step reads holds, at each step, that step's draw from the caller's generator -- step 2's differs from step 1's (a draw
    recorded inside the graph, or a buffer filled once, would replay stale noise); same seed same bits, another seed other bits."""
    from anyv2v_amd.pipeline import _StepEngine
    run = _sample if loop == "__call__" else _edit
    seen = []
    inner = _StepEngine._step

    def spy(self, t_row, coef_row, key, noise=None):
        inner(self, t_row, coef_row, key, noise)
        seen.append(self.noise.clone())          # what the replay that was just enqueued reads (stream order)
    monkeypatch.setattr(_StepEngine, "_step", spy)
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "0")
    pipe = _pipe(clip, PHI)
    tr_graph = {}
    on_graph = run(pipe, clip, eta=ETA, seed=21, trace=tr_graph)
    assert any(e.graphs or (e.nosrc is not None and e.nosrc.graphs) for e in pipe._engines.values()), "no HIP graph was captured"
    gen = torch.Generator().manual_seed(21)
    want = [torch.randn(clip.lat0.shape, generator=gen, dtype=torch.float32).half() for _ in range(STEPS)]
    assert len(seen) == STEPS and all(torch.equal(s.cpu(), w) for s, w in zip(seen, want)), "a step did not read its own draw"
    assert not torch.equal(seen[0], seen[1]), "step 2 consumed step 1's noise"
    assert torch.equal(run(pipe, clip, eta=ETA, seed=21), on_graph), "same seed, other bits (replayed graphs)"
    assert not torch.equal(run(pipe, clip, eta=ETA, seed=22), on_graph), "another seed, the same bits"
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "1")
    tr_eager = {}
    on_eager = run(_pipe(clip, PHI), clip, eta=ETA, seed=21, trace=tr_eager)
    assert list(tr_graph) == list(tr_eager) and len(tr_graph) == STEPS
    for t in tr_graph:
        assert torch.equal(tr_graph[t], tr_eager[t]), f"HIP graphs differ from ANYV2V_NO_GRAPH=1 after the step at t = {t}"
    assert torch.equal(on_graph, on_eager) and torch.isfinite(on_graph.float()).all()


@pytest.mark.parametrize("loop", ["__call__", "sample_with_pnp"])
def test_both_options_off_is_the_parent_path(clip, loop, monkeypatch):
    """Both off: neither new op is reached (same launches as before the options existed), and a pipeline that had them on and switched
    them off again gives the bits of one that never had; on differs from off."""
    from anyv2v_amd import ops
    run = _sample if loop == "__call__" else _edit
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "0")
    calls = []
    for name in ("guidance_stats", "cfg_ddim_step_ex"):
        inner = getattr(ops, name)
        monkeypatch.setattr(ops, name, (lambda inner, name: lambda *a, **k: (calls.append(name), inner(*a, **k))[1])(inner, name))
    never = run(_pipe(clip), clip)
    assert calls == [], "the default path reached a sampler-option op"
    pipe = _pipe(clip)
    before = run(pipe, clip)
    pipe.enable_guidance_rescale(PHI)
    on = run(pipe, clip, eta=ETA, seed=5)
    assert set(calls) == {"guidance_stats", "cfg_ddim_step_ex"}
    pipe.disable_guidance_rescale()
    calls.clear()
    after = run(pipe, clip, eta=0.0)
    assert calls == [] and torch.equal(before, never) and torch.equal(after, never)
    assert float((on.float() - never.float()).abs().max()) > 1e-2, "the options do not move the sample"


def test_source_cache_replays_bit_equal_under_both_options(clip, monkeypatch):
    """Multi-edit job under eta + rescale: the first edit records, the second replays ([negative, editing] only) -- both bit-equal to
    the uncached edit; features recorded by a DEFAULT edit serve an edit with both options on just as well (the source branch never
    sees the edit latent)."""
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "0")
    want = _edit(_pipe(clip, PHI), clip, eta=ETA, seed=9)
    pipe = _pipe(clip, PHI)
    cache = pipe.enable_source_cache(True)
    first = _edit(pipe, clip, eta=ETA, seed=9)
    assert cache.recorded_steps > 0 and cache.replayed_steps == 0
    second = _edit(pipe, clip, eta=ETA, seed=9)
    assert cache.replayed_steps > 0
    assert torch.equal(first, want), "recording edit differs from the uncached one"
    assert torch.equal(second, want), "replayed edit differs from the uncached one"
    mixed = _pipe(clip)
    cache2 = mixed.enable_source_cache(True)
    _edit(mixed, clip)                              # default edit records
    mixed.enable_guidance_rescale(PHI)
    third = _edit(mixed, clip, eta=ETA, seed=9)     # both options on: replays those features
    assert cache2.replayed_steps > 0, "the options dropped the cache"
    assert torch.equal(third, want), "edit replaying features recorded by a default edit differs from the uncached one"
