"""Pixel-space composite of a masked edit on the GPU, the kernels through the C ABI on caller-owned operands against the fp64 definition
(tests/composite_spec.py): the alpha plane inside NaN-poisoned frames, the ``to_pil`` quantisation at every fp16 bit pattern, the paste
(aligned, and offset so that the scalar kernel runs) inside byte guard bands, the colour match, and ``composite_over_source`` behind a
masked ``sample_with_pnp`` on the mini checkpoint.

Bounds: alpha bit-equal to the definition without the feather; with it exactly 1 on the core and exactly 0 beyond the reach, elsewhere
``2 (2 R + 1) 2^-24`` (two passes of at most 2 R + 1 non-negative fp32 fma terms on values in [0, 1]).  The paste: byte-equal.  The colour
match: statistics exact, bytes within 0.5 + 1e-3 levels of the definition's real value (fp32 slack in gain and bias)."""
import ctypes
import os
import types

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PARAMS = [(0, 0.0), (1, 0.0), (64, 0.0), (0, 0.5), (3, 4.0), (0, 16.0)]
SHAPES = [(8, 8), (40, 24), (64, 64)]
POISON16, POISON32, POISON8 = 0x7E5A, 0x7FC5A5A5, 0xA5      # NaN bit patterns no kernel computes (tests/gpu_checks.py); a guard byte


def _taps(sigma):
    from anyv2v_amd import _lib, ops
    return ops.gaussian_taps(sigma, _lib.COMPOSITE_MAX_RADIUS, "feather_px", "pixels")


def _latent_masks(Fm, h, w):
    g = torch.Generator().manual_seed(100 * Fm + 10 * h + w)
    one = torch.zeros(Fm, h, w)
    one[:, h // 2, w // 2] = 1.0
    half = torch.zeros(Fm, h, w)
    half[:, :, : max(1, w // 2)] = 1.0
    rnd = (torch.rand(Fm, h, w, generator=g) > 0.8).float() * torch.rand(Fm, h, w, generator=g)     # soft cells count as support
    return {"empty": torch.zeros(Fm, h, w).half(), "full": torch.ones(Fm, h, w).half(), "one-cell": one.half(), "half-plane": half.half(),
            "random-cells": rnd.half()}


def _window(t, shift=0, pad=64):
    """``t`` copied into a contiguous window of a poisoned allocation, ``shift`` elements behind a 16-byte boundary -> (view, check) with
    ``check()`` true while everything outside the window is intact.  uint8 / int64 operands get guard bytes, floats a NaN pattern."""
    item = t.element_size()
    idt, bits = {1: (torch.uint8, POISON8), 2: (torch.int16, POISON16), 4: (torch.int32, POISON32), 8: (torch.int64, 0x5A5A5A5A5A5A5A5A)}[item]
    n, lo = t.numel(), pad + shift
    buf = torch.full((lo + n + pad,), bits, dtype=idt, device="cuda")
    assert buf.data_ptr() % 16 == 0 and (pad * item) % 16 == 0
    view = buf.view(t.dtype)[lo:lo + n].view(t.shape)
    view.copy_(t)
    return view, lambda: bool((buf[:lo] == bits).all() and (buf[lo + n:] == bits).all())


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _c_alpha(lm, grow_px, sigma, ws, out):
    from anyv2v_amd import _lib
    taps = _taps(sigma)
    arr = (ctypes.c_float * len(taps))(*taps) if taps else None
    Fm, h, w = lm.shape
    _lib.check(_lib.load().anyv2v_pixel_alpha_f16(lm.data_ptr(), Fm, h, w, grow_px, arr, len(taps) // 2, ws.data_ptr(), out.data_ptr(), _stream()),
               "anyv2v_pixel_alpha_f16")
    return out


def _c_stats(video, source, alpha, rec):
    from anyv2v_amd import _lib
    _, _, F, H, W = video.shape
    _lib.check(_lib.load().anyv2v_composite_stats_u8(video.data_ptr(), source.data_ptr(), alpha.data_ptr(), alpha.shape[0], F, H, W, rec.data_ptr(),
                                                    _stream()), "anyv2v_composite_stats_u8")
    return rec


def _c_composite(video, source, alpha, rec, out):
    from anyv2v_amd import _lib
    _, _, F, H, W = video.shape
    _lib.check(_lib.load().anyv2v_composite_u8(video.data_ptr(), source.data_ptr(), alpha.data_ptr(), alpha.shape[0],
                                              None if rec is None else rec.data_ptr(), out.data_ptr(), F, H, W, _stream()), "anyv2v_composite_u8")
    return out


def _records():
    from anyv2v_amd import _lib
    return torch.zeros(_lib.COMPOSITE_STATS_BLOCKS, _lib.COMPOSITE_STATS_RECORD, dtype=torch.int64, device="cuda")


# ------------------------------------------------------------------------------------------------ pixel alpha
@pytest.mark.parametrize("Fm", [1, 3])
@pytest.mark.parametrize("H,W", SHAPES)
def test_pixel_alpha_against_the_definition(Fm, H, W):
    """(8, 8) is one latent cell: every window and radius is wider than the image; (40, 24) has W smaller than one tap window.  Output and
    workspace sit inside NaN-poisoned frames, which stay intact."""
    import composite_spec as spec
    worst = 0.0
    for name, lm in _latent_masks(Fm, H // 8, W // 8).items():
        dlm = lm.cuda()
        for grow_px, sigma in PARAMS:
            R = len(_taps(sigma)) // 2
            want = spec.pixel_alpha(lm, grow_px, _taps(sigma))
            out, ok_o = _window(torch.zeros(Fm, H, W, dtype=torch.float32, device="cuda"))
            ws, ok_w = _window(torch.zeros(2 * Fm * H * W, dtype=torch.float32, device="cuda"))
            _c_alpha(dlm, grow_px, sigma, ws, out)
            torch.cuda.synchronize()
            got = out.cpu()
            assert ok_o() and ok_w() and torch.equal(dlm.cpu(), lm), (name, grow_px, sigma, "a frame or the input changed")
            assert not bool(torch.isnan(got).any()), (name, grow_px, sigma, "poison reached alpha")
            if R == 0:
                assert torch.equal(got.double(), want["alpha"]), (name, grow_px)
                continue
            assert bool((got[want["core"]] == 1).all()), (name, grow_px, sigma, "alpha is not exactly 1 on the grown support")
            assert bool((got[~want["reach"]] == 0).all()), (name, grow_px, sigma, "alpha is not exactly 0 beyond grow_px + 2 R")
            err = float((got.double() - want["alpha"]).abs().max())
            worst = max(worst, err / ((2 * R + 1) * 2.0 ** -24))
            assert err <= 2 * (2 * R + 1) * 2.0 ** -24, (name, grow_px, sigma, err)
    print(f"[composite] pixel alpha Fm {Fm} {H} x {W}: with the feather at most {worst:.3f} x (2 R + 1) 2^-24 from the definition (bound 2)")


def test_pixel_alpha_binding_and_shifted_operands():
    """``ops.pixel_alpha`` gives the C call's bits; with every operand one element behind a 16-byte boundary too."""
    from anyv2v_amd import ops
    lm = _latent_masks(3, 5, 3)["random-cells"].cuda()
    plain = ops.pixel_alpha(lm, 3, 4.0)
    vl, ok_l = _window(lm, 1)
    out, ok_o = _window(torch.zeros_like(plain), 1)
    ws, ok_w = _window(torch.zeros(2 * plain.numel(), dtype=torch.float32, device="cuda"), 1)
    _c_alpha(vl, 3, 4.0, ws, out)
    torch.cuda.synchronize()
    assert torch.equal(out, plain) and ok_l() and ok_o() and ok_w()


# ------------------------------------------------------------------------------------------------ the to_pil quantisation
def test_every_fp16_bit_pattern_gives_the_to_pil_byte():
    """All 65 536 fp16 bit patterns as video values, alpha = 1, no colour match: the bytes of ``vae.to_pil`` of the same tensor on the CPU,
    NaN and +-Inf included; through the 4-pixel kernel and through the scalar one."""
    import numpy as np
    from anyv2v_amd.encoders import SyntheticVAE
    bits = torch.zeros(3 * 152 * 144, dtype=torch.int32)
    bits[:65536] = torch.arange(65536, dtype=torch.int32)
    video = bits.to(torch.int16).view(torch.float16).view(1, 3, 1, 152, 144).clone()
    want = torch.from_numpy(np.stack([np.asarray(f) for f in SyntheticVAE().to_pil(video)]))
    source = torch.randint(0, 256, (1, 152, 144, 3), generator=torch.Generator().manual_seed(0), dtype=torch.uint8)
    alpha = torch.ones(1, 152, 144, dtype=torch.float32)
    for shift in (0, 1):
        dv, _ = _window(video.cuda(), shift)
        ds, _ = _window(source.cuda(), shift)
        da, _ = _window(alpha.cuda(), shift)
        out, ok = _window(torch.zeros_like(source).cuda(), shift)
        _c_composite(dv, ds, da, None, out)
        torch.cuda.synchronize()
        got = out.cpu()
        bad = (got != want).nonzero()
        assert bad.numel() == 0, (shift, int(bad.shape[0]), bad[:4].tolist())
        assert ok()


# ------------------------------------------------------------------------------------------------ the paste
def _case(F, Fm, H, W, seed, plant=True):
    """Random video and source, alpha from the kernel (hard core, feathered border, kept region), Inf / NaN planted where alpha == 0."""
    from anyv2v_amd import ops
    g = torch.Generator().manual_seed(seed)
    lm = _latent_masks(Fm, H // 8, W // 8)["half-plane" if W > 8 else "empty"]
    if W == 8:
        lm[-1] = 1.0     # (one latent cell per frame: the last mask frame is edited, any other kept)
    alpha = ops.pixel_alpha(lm.cuda(), 1, 0.5).cpu() if W > 8 else lm.float().repeat_interleave(8, 1).repeat_interleave(8, 2)
    if W == 8:   # a kept band and a soft band by hand: the cell is narrower than any feather
        alpha[:, :, :2], alpha[:, :, 3], alpha[:, :, 4] = 0.0, alpha[:, :, 3] * 0.75, alpha[:, :, 4] * 0.3330078125
    video = (torch.rand(1, 3, F, H, W, generator=g) * 2.4 - 1.2).half()
    source = torch.randint(0, 256, (F, H, W, 3), generator=g, dtype=torch.uint8)
    kept = (alpha.expand(F, H, W) == 0)[None, None].expand(1, 3, F, H, W)
    n0 = int(kept.sum()) if plant else 0
    video[kept if plant else torch.zeros_like(kept)] = torch.tensor([float("inf"), float("nan"), float("-inf")]).half().repeat(n0 // 3 + 1)[:n0]
    return video, source, alpha.contiguous()


@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "offset-scalar-path"])
@pytest.mark.parametrize("H,W", SHAPES)
def test_composite_against_the_definition(H, W, shift):
    """Byte-equal to the definition everywhere; the source's bytes where alpha == 0 even under the planted NaN / Inf; the ``to_pil`` bytes
    where alpha == 1; inputs unchanged, guard bands intact."""
    import composite_spec as spec
    for F in (1, 3):
        for Fm in sorted({1, F}):
            video, source, alpha = _case(F, Fm, H, W, 10 * H + W + F + Fm)
            want = spec.composite(video, source, alpha)["out"]
            a = alpha.expand(F, H, W)
            assert int((a == 0).sum()) > 0 and int((a == 1).sum()) > 0 and int(((a > 0) & (a < 1)).sum()) > 0, "the case lacks a region"
            dv, ok_v = _window(video.cuda(), shift)
            ds, ok_s = _window(source.cuda(), shift)
            da, ok_a = _window(alpha.cuda(), shift)
            out, ok_o = _window(torch.zeros_like(source).cuda(), shift)
            assert (dv.data_ptr() % 8 == 0) == (shift == 0)
            _c_composite(dv, ds, da, None, out)
            torch.cuda.synchronize()
            got = out.cpu()
            assert torch.equal(got, want), (F, Fm, int((got != want).sum()))
            assert torch.equal(got[a == 0], source[a == 0]), "a kept pixel is not the source's byte"
            assert torch.equal(got[a == 1], spec.pil_bytes(video)[0].permute(1, 2, 3, 0)[a == 1]), "an edited pixel is not to_pil's byte"
            assert ok_v() and ok_s() and ok_a() and ok_o() and torch.equal(ds.cpu(), source) and torch.equal(da.cpu(), alpha)
            assert torch.equal(dv.cpu().view(torch.int16), video.view(torch.int16))


# ------------------------------------------------------------------------------------------------ the colour match
@pytest.mark.parametrize("shift", [0, 1], ids=["aligned", "offset-scalar-path"])
def test_colour_match(shift):
    """Records: summed over the blocks, the definition's integer sums exactly.  Bytes: within 0.5 + 1e-3 levels of the definition's real
    value.  Two runs: the same bits."""
    import composite_spec as spec
    from anyv2v_amd import ops
    for F, Fm, H, W in ((3, 1, 40, 24), (3, 3, 64, 64)):
        video, source, alpha = _case(F, Fm, H, W, 77 + F + Fm, plant=False)
        source = (source.float() * 0.6 + 30).to(torch.uint8)                   # (another contrast and level than the edit's)
        dv, _ = _window(video.cuda(), shift)
        ds, _ = _window(source.cuda(), shift)
        da, _ = _window(alpha.cuda(), shift)
        rec, ok_r = _window(_records(), 2 * shift)                             # (int64 records stay 8-byte aligned)
        out, ok_o = _window(torch.zeros_like(source).cuda(), shift)
        _c_stats(dv, ds, da, rec)
        _c_composite(dv, ds, da, rec, out)
        torch.cuda.synchronize()
        st = spec.stats(video, source, alpha)
        assert torch.equal(rec.cpu().sum(dim=0)[:15].view(3, 5), st) and int(rec[:, 15].abs().sum()) == 0 and int(st[0, 0]) >= 64
        gain, _bias = spec.gain_bias(st)
        assert bool((gain != 1).all()), "the case does not exercise the match"
        want = spec.composite(video, source, alpha, match_color=True)
        got = out.cpu()
        err = float((got.double() - want["real"]).abs().max())
        share = float((got == want["out"]).float().mean())
        print(f"[composite] colour match F {F} Fm {Fm} {H} x {W} shift {shift}: max |byte - real| {err:.6f} (bound 0.501), "
              f"{100 * share:.3f} % of the bytes equal the definition's own rounding")
        assert err <= 0.5 + 1e-3 and ok_r() and ok_o()
        a = alpha.expand(F, H, W)
        assert torch.equal(got[a == 0], source[a == 0])
        rec2, out2 = _records(), torch.zeros_like(out)
        _c_stats(dv, ds, da, rec2)
        _c_composite(dv, ds, da, rec2, out2)
        assert torch.equal(rec2, rec) and torch.equal(out2, out), "two runs differ"
        if shift == 0:
            assert torch.equal(ops.composite(video.cuda(), source.cuda(), alpha.cuda(), match_color=True), out), "ops.composite differs"
            assert torch.equal(ops.composite_stats(video.cuda(), source.cuda(), alpha.cuda()), rec)


def test_colour_match_identity_cases():
    """Fewer than 64 kept pixels, or a constant edit channel: gain 1, bias 0 -- the bytes of the plain paste."""
    g = torch.Generator().manual_seed(5)
    F, H, W = 2, 16, 24
    source = torch.randint(0, 256, (F, H, W, 3), generator=g, dtype=torch.uint8).cuda()
    soft = torch.rand(1, H, W, generator=g)
    few = soft.clone()
    few.view(-1)[:31] = 0.0              # 31 pixels x 2 frames = 62 kept: the count is the clip's
    many = soft.clone()
    many.view(-1)[:200] = 0.0
    cases = [((torch.rand(1, 3, F, H, W, generator=g) * 2 - 1).half(), few), (torch.zeros(1, 3, F, H, W).half(), many)]
    for video, alpha in cases:
        dv, da = video.cuda(), alpha.cuda()
        rec = _c_stats(dv, source, da, _records())
        plain = _c_composite(dv, source, da, None, torch.zeros_like(source))
        matched = _c_composite(dv, source, da, rec, torch.zeros_like(source))
        assert int(rec.sum(dim=0)[0]) == int((alpha == 0).sum()) * F
        assert torch.equal(matched, plain)


# ------------------------------------------------------------------------------------------------ mini pipeline
FR, HW_, STEPS = 4, 8, 4


def test_composite_over_source_behind_a_masked_edit(monkeypatch):
    """A masked ``sample_with_pnp`` with a half-plane mask on the mini checkpoint, decoded by the native VAE (random weights): the kept half of the composite
    is the source frames byte for byte, the edited half is the uncomposited ``to_pil`` output of the decode as fp16; without the call
    the pipeline's own ``pil`` output is what it was."""
    import numpy as np
    import gpu_checks as gc
    from anyv2v_amd import pnp_utils
    from anyv2v_amd.encoders import NativeVAE
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMInverseScheduler, DDIMScheduler
    from anyv2v_amd.vae import VAEConfig
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "0")
    native, _, ocfg = gc.build_pair("mini", 1234)
    inp = gc.config1_inputs(ocfg, 3, FR, HW_)
    h = lambda x: x.half().cuda()
    lat0, ehs, ie, il = h(inp["sample"][:1]), h(inp["encoder_hidden_states"]), h(inp["image_embeddings"]), h(inp["image_latents"])
    vae = NativeVAE(random_init_seed=1, cfg=VAEConfig()).to("cuda")     # the 8x architecture (the mini VAE decodes 2x): 8 x 8 latents -> 64 x 64
    inv = I2VGenXLPipeline(unet=native, scheduler=DDIMInverseScheduler())
    inv._device = torch.device("cuda")
    traj = inv.invert(prompt_embeds=ehs[:1], image_embeddings=ie[:1], image_latents=il[:1], height=HW_ * 8, width=HW_ * 8, num_frames=FR,
                      num_inference_steps=STEPS, guidance_scale=1.0, target_fps=8, latents=lat0, return_trajectory=True)
    pipe = I2VGenXLPipeline(unet=native, scheduler=DDIMScheduler())
    pipe._device = torch.device("cuda")
    pipe.register_modules(vae=vae)
    mask = torch.zeros(1, HW_ * 8, HW_ * 8)
    mask[:, :, : HW_ * 4] = 1.0          # the left half is edited, the right half keeps the source

    def edit(output_type):
        sched = DDIMScheduler()
        sched.set_timesteps(STEPS)
        pipe.register_modules(scheduler=sched)
        k = lambda r: sched.timesteps[: int(STEPS * r)]
        pnp_utils.register_conv_injection(pipe, k(0.5))
        pnp_utils.register_spatial_attention_pnp(pipe, k(0.75))
        pnp_utils.register_temp_attention_pnp(pipe, k(1.0))
        try:
            return pipe.sample_with_pnp(prompt_embeds=ehs[2:3], negative_prompt_embeds=ehs[1:2], image_embeddings=ie[2:3], image_latents=il[2:3],
                                        height=HW_ * 8, width=HW_ * 8, num_frames=FR, num_inference_steps=STEPS, guidance_scale=9.0, target_fps=8,
                                        latents=traj[max(traj.keys())].clone(), output_type=output_type, ddim_init_latents_t_idx=0,
                                        ddim_inv_latents_path=traj, ddim_inv_prompt_embeds=ehs[:1], ddim_inv_image_embeddings=ie[:1],
                                        ddim_inv_image_latents=il[:1]).frames
        finally:
            pnp_utils.clear_time(pipe)

    stack = lambda frames: torch.from_numpy(np.stack([np.asarray(f) for f in frames]))
    pipe.enable_masked_edit(mask, lat0)
    before = stack(edit("pil")[0])
    latents = edit("latent").clone()
    video = pipe.decode_latents(latents, decode_chunk_size=1)     # (the chunking of the pipeline's own decode)
    assert tuple(video.shape) == (1, 3, FR, HW_ * 8, HW_ * 8)
    full = stack(vae.to_pil(video))
    assert torch.equal(full, before)
    # the native decode hands its fp16 values over as an fp32 tensor, and ``to_pil`` then quantises in fp32; the composite's contract is
    # the quantisation of the fp16 tensor (include/anyv2v_hip.h), to which the method casts -- losslessly, asserted here
    assert torch.equal(video.half().float(), video), "the decode's values are not fp16 values"
    pil = stack(vae.to_pil(video.half()))
    print(f"[composite] {100 * float((pil == full).float().mean()):.2f} % of to_pil's bytes are the same from the fp16 tensor and from its "
          f"fp32 copy (max difference {int((pil.int() - full.int()).abs().max())} level)")
    source = torch.randint(0, 256, (FR, HW_ * 8, HW_ * 8, 3), generator=torch.Generator().manual_seed(2), dtype=torch.uint8)
    out = pipe.composite_over_source(video, source.cuda(), mask)
    assert out.is_cuda and out.dtype == torch.uint8
    out = out.cpu()
    assert torch.equal(out[:, :, HW_ * 4:], source[:, :, HW_ * 4:]), "the kept half is not the source frames, byte for byte"
    assert torch.equal(out[:, :, : HW_ * 4], pil[:, :, : HW_ * 4]), "the edited half is not the uncomposited to_pil output"
    soft = pipe.composite_over_source(video, source.cuda(), mask, grow_px=2, feather_px=1.0, match_color=True).cpu()
    assert torch.equal(soft[:, :, HW_ * 4 + 8:], source[:, :, HW_ * 4 + 8:]) and not torch.equal(soft, out)
    assert torch.equal(stack(edit("pil")[0]), before), "the pipeline's own output changed after the composite ran"
    pipe.disable_masked_edit()
