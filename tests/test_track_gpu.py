"""Mask tracking on the GPU (``anyv2v_amd/csrc/track.hip``): every kernel against ``track_spec`` bit for bit -- all of it is integer
arithmetic, there is no tolerance anywhere -- then the tracked mask through ``enable_masked_edit`` and two edit steps of the mini model."""
import functools
import os
import types

import pytest
import torch

import track_spec as spec
from test_track_host import inside_cells, moving_clip, periodic_pair, texture, translated_pair

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(F, H, W, R):
    """A seeded clip under smooth motion and the definition's field for it: computed once, shared, never modified."""
    y = moving_clip(F, H, W, seed=F + H + R, smooth=2)
    return y, spec.block_match(y, R)


def _match(y, R):
    from anyv2v_amd import ops
    return ops.block_match(y.cuda().contiguous(), R).cpu()


# F=3 64x64 R=4: several blocks of 4 x 4 cells.  F=2 40x72 R=7: an odd radius, 5 x 9 cells (no multiple of the block's 4, a width that is
# no multiple of 16), every window row and column clamps somewhere, all four byte alignments of dx.  F=2 96x80 R=32: the largest radius,
# the halo larger than the frame in places.  R=0 and F=1: the paths that search nothing.
@pytest.mark.parametrize("F,H,W,R", [(3, 64, 64, 4), (2, 40, 72, 7), (2, 96, 80, 32), (2, 40, 72, 0), (1, 64, 64, 4)])
def test_block_match_against_the_definition(F, H, W, R):
    y, want = _case(F, H, W, R)
    got = _match(y, R)
    assert got.dtype == torch.int16 and tuple(got.shape) == (F, H // 8, W // 8, 2)
    if F > 1 and R > 0:
        assert bool(want[1:].any()) and len({tuple(v) for v in want[1].reshape(-1, 2).tolist()}) >= 2, "the clip moves in more than one way"
    else:
        assert not bool(want.any())
    bad = (got != want).any(-1)
    assert torch.equal(got, want), f"{int(bad.sum())} of {bad.numel()} cells differ, first at {bad.nonzero()[:4].tolist()}"


@pytest.mark.parametrize("d,R", [((3, -5), 6), ((-6, 6), 6), ((0, 7), 7), ((-2, 0), 3)])
def test_block_match_recovers_a_known_translation(d, R):
    H, W = 48, 64
    flow = _match(translated_pair(H, W, d, R, seed=1), R)
    ok = inside_cells(H, W, d)
    assert not bool(flow[0].any()) and torch.equal(flow[1][ok], torch.tensor(d, dtype=torch.int16).expand(int(ok.sum()), 2))


def test_block_match_flat_saturated_and_periodic_frames():
    assert not bool(_match(torch.full((3, 32, 40), 117, dtype=torch.uint8), 5).any())
    steps = torch.stack([torch.zeros(32, 40, dtype=torch.uint8), torch.full((32, 40), 255, dtype=torch.uint8)])
    assert not bool(_match(steps, 5).any()), "every candidate costs 65 280: the zero vector is the shortest"
    assert not bool(_match(steps, 32).any())
    pair = periodic_pair(64, 64, 8, (6, 5))
    flow = _match(pair, 12)
    assert torch.equal(flow[1, 2:6, 2:6], torch.tensor([-2, -3], dtype=torch.int16).expand(4, 4, 2)), "not the shortest of the zero-cost vectors"
    assert torch.equal(flow, spec.block_match(pair, 12))


def test_luma_against_the_definition():
    from anyv2v_amd import ops
    g = torch.Generator().manual_seed(2)
    rgb = torch.randint(0, 256, (3, 40, 72, 3), generator=g, dtype=torch.uint8)
    rgb[0, 0, :4] = torch.tensor([[255, 255, 255], [0, 0, 0], [255, 0, 0], [0, 0, 255]], dtype=torch.uint8)
    want = spec.luma(rgb)
    assert torch.equal(ops.luma_u8(rgb.cuda()).cpu(), want)
    odd = torch.zeros(rgb.numel() + 1, dtype=torch.uint8, device="cuda")[1:].view(rgb.shape)      # a pointer that is not 4-byte aligned
    odd.copy_(rgb)
    assert odd.data_ptr() % 4 == 1 and torch.equal(ops.luma_u8(odd).cpu(), want)


def test_median_with_planted_outliers_at_borders_and_corners():
    from anyv2v_amd import ops
    g = torch.Generator().manual_seed(5)
    flow = torch.randint(-3, 4, (2, 5, 9, 2), generator=g).to(torch.int16)
    for (cy, cx) in ((0, 0), (0, 8), (4, 0), (4, 8), (0, 4), (4, 5), (2, 0), (2, 8), (2, 4)):      # corners, borders, the interior
        flow[0, cy, cx] = torch.tensor([32, -32])
    flow[1, :2, :2] = torch.tensor([-32, 32])      # a corner patch the clamped neighbourhood makes a majority
    flow[1, 4, :] = 17                             # a border row
    want = spec.flow_median(flow)
    got = ops.flow_median(flow.cuda()).cpu()
    assert torch.equal(got, want)
    assert int(want[0].abs().max()) <= 3 and int(want[1, 0, 0, 0]) == -32 and int(want[1, 4, 4, 1]) == 17
    one = torch.tensor([[[[5, -7]]]], dtype=torch.int16)
    assert torch.equal(ops.flow_median(one.cuda()).cpu(), one)


def test_propagation_against_the_sequential_definition():
    from anyv2v_amd import ops
    g = torch.Generator().manual_seed(3)
    flow = torch.randint(-32, 33, (5, 5, 9, 2), generator=g).to(torch.int16)
    mask0 = torch.rand(40, 72, generator=g) < 0.4
    want = spec.propagate(mask0, flow)
    got = ops.mask_propagate(mask0.cuda(), flow.cuda()).cpu()
    assert got.dtype == torch.bool and torch.equal(got, want) and torch.equal(want, spec.propagate_chain(mask0, flow))
    assert torch.equal(ops.mask_propagate((mask0.to(torch.uint8) * 255).cuda(), flow.cuda()).cpu(), want)
    assert torch.equal(ops.mask_propagate(mask0.cuda(), flow[:1].cuda().contiguous()).cpu(), mask0[None]), "F = 1 returns the input mask"
    # a mask under a known translation: Y_k[p] = Y_{k-1}[p + d] moves the content by -d per frame
    d = (3, -5)
    const = torch.tensor(d, dtype=torch.int16).expand(3, 5, 9, 2).contiguous()
    box = torch.zeros(40, 72, dtype=torch.bool)
    box[16:28, 30:50] = True
    moved = ops.mask_propagate(box.cuda(), const.cuda()).cpu()
    for k in range(3):
        shifted = torch.zeros_like(box)
        shifted[16 - 3 * k: 28 - 3 * k, 30 + 5 * k: 50 + 5 * k] = True
        assert torch.equal(moved[k], shifted), k


def test_first_frame_mask_at_the_decision_edges():
    from anyv2v_amd import ops
    thr, cnt = 24, 8
    src = torch.full((24, 40, 3), 100, dtype=torch.uint8)
    ed = src.clone()
    ed[0, :8, 1] = 100 + thr                      # cell (0, 0): min_count pixels at exactly the threshold        -> not set
    ed[8, :8, 2] = 100 + thr + 1                  # cell (1, 0): min_count pixels one over it                     -> set
    ed[16:18, 8:12, 0] = 100 - thr - 1            # cell (2, 1): min_count pixels one under it, downwards          -> set
    ed[9, 16:23, 0] = 255                         # cell (1, 2): min_count - 1 pixels                              -> not set
    ed[:8, 32:, :] = 0                            # cell (0, 4): all 64
    got = ops.first_frame_mask(src.cuda(), ed.cuda(), thr, cnt).cpu()
    assert got.dtype == torch.bool and tuple(got.shape) == (1, 24, 40) and torch.equal(got, spec.first_frame_mask(src, ed, thr, cnt))
    cells = got[0, ::8, ::8]
    assert cells.tolist() == [[False, False, False, False, True], [True, False, False, False, False], [False, True, False, False, False]]
    assert torch.equal(got[0], cells.repeat_interleave(8, 0).repeat_interleave(8, 1)), "constant on cells"
    g = torch.Generator().manual_seed(8)
    a = torch.randint(0, 256, (40, 72, 3), generator=g, dtype=torch.uint8)
    b = torch.where(torch.rand(40, 72, 1, generator=g) < 0.15, torch.randint(0, 256, (40, 72, 3), generator=g, dtype=torch.uint8), a)
    for t, c in ((24, 8), (0, 1), (255, 1), (100, 64), (10, 9)):
        assert torch.equal(ops.first_frame_mask(a.cuda(), b.cuda(), t, c).cpu(), spec.first_frame_mask(a, b, t, c)), (t, c)


def test_two_calls_return_equal_tensors():
    from anyv2v_amd import ops
    y, _ = _case(2, 40, 72, 7)
    yd = y.cuda()
    first = ops.block_match(yd, 7)
    second = ops.block_match(yd, 7)
    assert torch.equal(first, second)
    mask0 = (texture(40, 72, 4) > 128).cuda()
    assert torch.equal(ops.mask_propagate(mask0, ops.flow_median(first)), ops.mask_propagate(mask0, ops.flow_median(second)))


# ------------------------------------------------------------------------------------------------ through the pipeline
FR, HW_, STEPS, G = 3, 8, 2, 9.0


@pytest.fixture(scope="module")
def clip():
    """One mini model, one clip and its two-step inversion -- shared, unchanged, by the pipeline test below."""
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
    c.src = (c.lat0 + 0.5).contiguous()
    c.frames = moving_clip(FR, HW_ * 8, HW_ * 8, seed=11)[..., None].expand(FR, HW_ * 8, HW_ * 8, 3).contiguous()
    return c


def _edit(c, mask, trace=None):
    from anyv2v_amd import pnp_utils
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMScheduler
    sched = DDIMScheduler()
    sched.set_timesteps(STEPS)
    pipe = I2VGenXLPipeline(unet=c.native, scheduler=sched)
    pipe._device = torch.device("cuda")
    pipe.enable_masked_edit(mask, c.src)
    pnp_utils.register_conv_injection(pipe, sched.timesteps[:1])
    pnp_utils.register_spatial_attention_pnp(pipe, sched.timesteps[:1])
    pnp_utils.register_temp_attention_pnp(pipe, sched.timesteps[:2])
    try:
        out = pipe.sample_with_pnp(prompt_embeds=c.ehs[2:3], negative_prompt_embeds=c.ehs[1:2], image_embeddings=c.ie[2:3],
                                   image_latents=c.il[2:3], height=HW_ * 8, width=HW_ * 8, num_frames=FR, num_inference_steps=STEPS,
                                   guidance_scale=G, target_fps=8, eta=0.0, generator=torch.Generator().manual_seed(0),
                                   latents=c.traj[c.T].clone(), output_type="latent", ddim_init_latents_t_idx=0, ddim_inv_latents_path=c.traj,
                                   ddim_inv_prompt_embeds=c.ehs[:1], ddim_inv_image_embeddings=c.ie[:1], ddim_inv_image_latents=c.il[:1],
                                   latents_trace=trace).frames.clone()
    finally:
        pnp_utils.clear_time(pipe)
    return out, pipe


def test_tracked_mask_through_the_masked_edit(clip, monkeypatch):
    """``propagate_edit_mask`` -> ``enable_masked_edit`` -> ``sample_with_pnp``: a mask that tracks to all zeros gives the trajectory /
    ``source_latents`` bit for bit (the masked edit's own contract); a tracked mask is a mask like any other to the engines -- their keys
    are those of a hand-made mask of the same shape."""
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "0")
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMScheduler
    tracker = I2VGenXLPipeline(unet=clip.native, scheduler=DDIMScheduler())
    tracker._device = torch.device("cuda")
    H = W = HW_ * 8
    none, flow = tracker.propagate_edit_mask(clip.frames, torch.zeros(H, W, dtype=torch.bool), return_flow=True)
    want_flow = spec.flow_median(spec.block_match(spec.luma(clip.frames), 16))
    assert none.is_cuda and none.dtype == torch.bool and tuple(none.shape) == (FR, H, W) and not bool(none.any())
    assert torch.equal(flow.cpu(), want_flow) and bool(want_flow.any())
    assert tracker._masked_edit is None and not tracker._engines
    trace = {}
    out, _ = _edit(clip, none, trace)
    for i, t in enumerate(clip.ts):
        want = clip.traj[clip.ts[i + 1]] if i + 1 < STEPS else clip.src
        assert torch.equal(trace[t], want), f"all-zeros tracked mask: the latent after t = {t} is not the source at the next level"
    assert torch.equal(out, clip.src)
    box = torch.zeros(1, H, W, dtype=torch.bool)
    box[:, 16:48, 8:40] = True
    tracked = tracker.propagate_edit_mask(clip.frames, box)
    assert torch.equal(tracked.cpu(), spec.propagate(box[0], want_flow)) and not torch.equal(tracked[2], tracked[0])
    out_t, pipe_t = _edit(clip, tracked)
    hand = torch.zeros(FR, H, W, dtype=torch.bool)
    hand[:, :, : W // 2] = True
    out_h, pipe_h = _edit(clip, hand)
    assert list(pipe_t._engines.keys()) == list(pipe_h._engines.keys()) and len(pipe_t._engines) >= 1
    assert torch.isfinite(out_t.float()).all() and not torch.equal(out_t, clip.src)
    keep = ~torch.nn.functional.max_pool2d(tracked[None].float(), 8)[0].bool()       # latent cells the tracked mask misses entirely
    assert int(keep.sum()) > 0 and torch.equal(out_t[0, :, keep], clip.src[0, :, keep]), "outside the tracked mask the result is not the source's bits"
