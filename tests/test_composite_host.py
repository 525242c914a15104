"""Pixel-space composite of a masked edit, host side (no GPU): the fp64 definition against itself (tests/composite_spec.py), the CPU
emulation against the definition, the header / binding / ABI, the C entry points' argument validation, every refusal of
``composite_over_source`` and ``composite_options``, the config keys through the output suffix and through ``Stage2`` down to the PNG files."""
import ctypes
import logging
import os
import re
import types

import pytest
import torch

import composite_spec as spec
import cpu_composite_emulation as cemu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _taps(sigma):
    from anyv2v_amd import _lib, ops
    return ops.gaussian_taps(sigma, _lib.COMPOSITE_MAX_RADIUS, "feather_px", "pixels")


def _half_plane(h=8, w=8, Fm=1):
    lm = torch.zeros(Fm, h, w, dtype=torch.float16)
    lm[:, :, : w // 2] = 1.0
    return lm


def _clip(F=2, H=64, W=64, seed=0):
    g = torch.Generator().manual_seed(seed)
    video = (torch.rand(1, 3, F, H, W, generator=g) * 2.4 - 1.2).half()
    source = torch.randint(0, 256, (F, H, W, 3), generator=g, dtype=torch.uint8)
    return video, source


# ------------------------------------------------------------------------------------------------ the definition against itself
def test_spec_all_ones_is_to_pil_and_all_zeros_is_the_source():
    from anyv2v_amd.encoders import SyntheticVAE
    import numpy as np
    video, source = _clip()
    video[0, 0, 0, 0, :4] = torch.tensor([float("nan"), float("inf"), float("-inf"), 65504.0]).half()
    pil = torch.from_numpy(np.stack([np.asarray(f) for f in SyntheticVAE().to_pil(video)]))
    for grow_px, sigma in ((0, 0.0), (3, 4.0)):
        ones = spec.pixel_alpha(torch.ones(1, 8, 8, dtype=torch.float16), grow_px, _taps(sigma))["alpha"]
        zeros = spec.pixel_alpha(torch.zeros(2, 8, 8, dtype=torch.float16), grow_px, _taps(sigma))["alpha"]
        assert bool((ones == 1).all()) and bool((zeros == 0).all())
        assert torch.equal(spec.composite(video, source, ones.float())["out"], pil)
        assert torch.equal(spec.composite(video, source, zeros.float())["out"], source)
        assert torch.equal(spec.composite(video, source, zeros.float(), match_color=True)["out"], source)


@pytest.mark.parametrize("grow_px,sigma", [(0, 0.0), (5, 0.0), (0, 0.5), (3, 4.0), (0, 16.0)])
def test_spec_alpha_along_a_ray_leaving_a_half_plane(grow_px, sigma):
    """1 on the core, monotone non-increasing along the ray, exactly 0 beyond grow_px + 2 R; a soft latent cell (mask 2^-10) counts as
    support like a full one."""
    taps = _taps(sigma)
    R = len(taps) // 2
    w = 40                                                  # 320 pixels: the support ends at x = 160, the reach (<= 160 + 96) inside
    lm = _half_plane(2, w)
    lm[0, 1, w // 2 - 1] = 2.0 ** -10
    r = spec.pixel_alpha(lm, grow_px, taps)
    ray = r["alpha"][0, 9]
    edge = 8 * (w // 2)
    assert bool((ray[: edge + grow_px] == 1).all()) and bool(r["core"][0, 9, : edge + grow_px].all()) and not bool(r["core"][0, 9, edge + grow_px])
    assert bool((ray[1:] <= ray[:-1]).all()), "alpha is not monotone along the ray"
    assert bool((ray[edge + grow_px + 2 * R:] == 0).all()) and not bool(r["reach"][0, 9, edge + grow_px + 2 * R:].any())
    if R > 0:
        assert 0 < float(ray[edge + grow_px]) < 1 and float(ray[edge + grow_px + 2 * R - 1]) > 0
    assert bool(((r["alpha"] >= 0) & (r["alpha"] <= 1)).all())


def test_spec_paste_and_colour_match():
    video, source = _clip(F=3, H=16, W=24, seed=3)
    alpha = torch.rand(3, 16, 24, generator=torch.Generator().manual_seed(1))
    alpha.view(-1)[::3], alpha.view(-1)[1::3] = 0.0, 1.0
    e = spec.pil_bytes(video)[0].permute(1, 2, 3, 0)
    r = spec.composite(video, source, alpha)
    a = alpha[..., None].expand_as(e)
    assert torch.equal(r["out"][a == 0], source[a == 0]) and torch.equal(r["out"][a == 1], e[a == 1])
    lo, hi = torch.minimum(e, source), torch.maximum(e, source)
    assert bool(((r["out"] >= lo) & (r["out"] <= hi)).all())
    # a source that is an affine map of the edit over the kept region: the match recovers gain and bias
    src2 = (e.double() * 0.75 + 20.0).round().clamp(0, 255).to(torch.uint8)
    gain, bias = spec.gain_bias(spec.stats(video, src2, alpha))
    assert float((gain - 0.75).abs().max()) < 0.01 and float((bias - 20.0).abs().max()) < 1.5
    few = torch.ones(3, 16, 24)
    few.view(-1)[:63] = 0.0                                  # 63 kept pixels: identity
    assert spec.gain_bias(spec.stats(video, src2, few))[0].tolist() == [1.0] * 3
    flat = torch.zeros_like(video)
    gain, bias = spec.gain_bias(spec.stats(flat, src2, alpha))    # a constant edit channel: identity
    assert gain.tolist() == [1.0] * 3 and bias.tolist() == [0.0] * 3


@pytest.mark.parametrize("grow_px,sigma", [(0, 0.0), (1, 0.0), (64, 0.0), (0, 0.5), (3, 4.0), (0, 16.0)])
def test_emulation_against_the_definition(grow_px, sigma):
    g = torch.Generator().manual_seed(7)
    lm = (torch.rand(2, 5, 3, generator=g) > 0.7).half() * torch.rand(2, 5, 3, generator=g).half()
    want = spec.pixel_alpha(lm, grow_px, _taps(sigma))
    got = cemu.pixel_alpha(lm, grow_px, sigma)
    R = len(_taps(sigma)) // 2
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 40, 24)
    assert bool((got[want["core"]] == 1).all()) and bool((got[~want["reach"]] == 0).all())
    assert float((got.double() - want["alpha"]).abs().max()) <= 2 * (2 * R + 1) * 2.0 ** -23      # (mul + add where the kernel has one fmaf)
    video, source = _clip(F=2, H=40, W=24, seed=9)
    assert torch.equal(cemu.composite(video, source, got), spec.composite(video, source, got)["out"])
    st = cemu.composite_stats(video, source, got)
    assert torch.equal(st.sum(dim=0)[:15].view(3, 5), spec.stats(video, source, got))
    m = cemu.composite(video, source, got, match_color=True)
    assert float((m.double() - spec.composite(video, source, got, match_color=True)["real"]).abs().max()) <= 0.5 + 1e-3


# ------------------------------------------------------------------------------------------------ header, binding, validation
def test_header_binding_and_abi_version():
    from anyv2v_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "anyv2v_hip.h")).read()
    for sym, nargs in (("anyv2v_pixel_alpha_f16", 10), ("anyv2v_composite_stats_u8", 9), ("anyv2v_composite_u8", 10)):
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % sym, hdr)
        assert decl and len(decl.group(1).split(",")) == nargs, sym
        assert sym in _lib.SYMBOLS and len(_lib.SYMBOLS[sym][1]) == nargs, sym
        if os.path.isfile(_lib.LIB_PATH):
            assert hasattr(ctypes.CDLL(_lib.LIB_PATH), sym)
    consts = {k: int(v) for k, v in re.findall(r"#define ANYV2V_COMPOSITE_(\w+) (\d+)", hdr)}
    assert consts == dict(MAX_GROW=_lib.COMPOSITE_MAX_GROW, MAX_RADIUS=_lib.COMPOSITE_MAX_RADIUS, STATS_BLOCKS=_lib.COMPOSITE_STATS_BLOCKS,
                          STATS_RECORD=_lib.COMPOSITE_STATS_RECORD)
    assert consts["MAX_GROW"] == 64 and consts["MAX_RADIUS"] == 3 * 16 and consts["STATS_RECORD"] >= 15
    assert "alpha = core ? 1.0f : min(a, 1.0f)" in hdr and "2206.02779" in hdr
    assert callable(ops.pixel_alpha) and callable(ops.composite_stats) and callable(ops.composite)
    assert _lib.ABI_VERSION == 105 and "#define ANYV2V_ABI_VERSION 105" in hdr
    mk = open(os.path.join(ROOT, "anyv2v_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\bcomposite\.hip\b", mk, re.M)


def _lib_or_skip():
    from anyv2v_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.skip("libanyv2v_hip.so is not built")
    return _lib.load()


def test_abi_validation_without_gpu():
    """Host-side validation returns ANYV2V_EINVAL (-1) with a message before anything touches a device."""
    lib = _lib_or_skip()
    P = 4096   # any 16-byte-aligned non-null address: nothing on the device is dereferenced before the checks
    taps = (ctypes.c_float * 3)(0.25, 0.5, 0.25)
    good = dict(lm=P, Fm=1, h=8, w=8, grow=1, taps=taps, R=1, ws=2 * P, out=3 * P)

    def pa(**over):
        a = dict(good, **over)
        return lib.anyv2v_pixel_alpha_f16(a["lm"], a["Fm"], a["h"], a["w"], a["grow"], a["taps"], a["R"], a["ws"], a["out"], None)

    for name in ("lm", "ws", "out", "taps"):
        assert pa(**{name: None}) == -1 and b"null pointer" in lib.anyv2v_last_error(), name
    for over in (dict(Fm=0), dict(h=0), dict(w=-1)):
        assert pa(**over) == -1 and b"at least 1" in lib.anyv2v_last_error(), over
    for grow in (-1, 65):
        assert pa(grow=grow) == -1 and b"grow_px" in lib.anyv2v_last_error()
    for R in (-1, 49):
        assert pa(R=R) == -1 and b"R =" in lib.anyv2v_last_error()
    assert pa(Fm=1 << 5, h=1 << 10, w=1 << 10) == -1 and b"fit an int" in lib.anyv2v_last_error()
    assert pa(out=2 * P) == -1 and b"workspace may not be the output" in lib.anyv2v_last_error()
    for bad in (float("nan"), -0.5, 2.0, float("inf")):
        assert pa(taps=(ctypes.c_float * 3)(0.25, bad, 0.25)) == -1 and b"tap 1" in lib.anyv2v_last_error(), bad
    good2 = dict(video=P, src=2 * P, alpha=3 * P, Fm=1, rec=4 * P, out=5 * P, F=2, H=8, W=8)

    def st(**over):
        a = dict(good2, **over)
        return lib.anyv2v_composite_stats_u8(a["video"], a["src"], a["alpha"], a["Fm"], a["F"], a["H"], a["W"], a["rec"], None)

    def co(**over):
        a = dict(good2, **over)
        return lib.anyv2v_composite_u8(a["video"], a["src"], a["alpha"], a["Fm"], a["rec"], a["out"], a["F"], a["H"], a["W"], None)

    for fn, names in ((st, ("video", "src", "alpha", "rec")), (co, ("video", "src", "alpha", "out"))):
        for name in names:
            assert fn(**{name: None}) == -1 and b"null pointer" in lib.anyv2v_last_error(), name
        for over in (dict(F=0), dict(H=0), dict(W=-8)):
            assert fn(**over) == -1 and b"bad arguments" in lib.anyv2v_last_error(), over
        for Fm in (0, 3, -1):
            assert fn(Fm=Fm) == -1 and b"must be 1 or F" in lib.anyv2v_last_error()
        assert fn(Fm=1, F=1 << 10, H=1 << 10, W=1 << 10) == -1 and b"fit an int" in lib.anyv2v_last_error()
        assert fn(rec=4 * P + 4) == -1 and b"8-byte aligned" in lib.anyv2v_last_error()
    for name in ("video", "src", "alpha", "rec"):
        assert co(out=good2[name]) == -1 and b"may not alias" in lib.anyv2v_last_error(), name


# ------------------------------------------------------------------------------------------------ refusals
def _meta_pipe():
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMScheduler
    from anyv2v_amd.unet import I2VGenXLUNet, I2VGenXLUNetConfig
    with torch.device("meta"):
        unet = I2VGenXLUNet(I2VGenXLUNetConfig.mini())
    return I2VGenXLPipeline(unet=unet, scheduler=DDIMScheduler()), unet


def test_composite_over_source_refusals_and_forms(monkeypatch):
    from PIL import Image
    cemu.install(monkeypatch)
    pipe, unet = _meta_pipe()
    video, source = _clip(F=2, H=64, W=64)
    mask = torch.zeros(64, 64, dtype=torch.bool)
    mask[:, :32] = True
    out = pipe.composite_over_source(video, source, mask)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (2, 64, 64, 3)
    e = spec.pil_bytes(video)[0].permute(1, 2, 3, 0)
    assert torch.equal(out[:, :, 32:], source[:, :, 32:]) and torch.equal(out[:, :, :32], e[:, :, :32])
    frames = [Image.fromarray(f.numpy()) for f in source]
    assert torch.equal(pipe.composite_over_source(video, frames, mask), out)
    assert torch.equal(pipe.composite_over_source(video, frames, mask[None].expand(2, 64, 64).float()), out)
    soft = pipe.composite_over_source(video, source, mask, grow_px=4, feather_px=2.0, match_color=True)    # reach 4 + 2 * 6 pixels
    assert torch.equal(soft[:, :, 48:], source[:, :, 48:]) and not torch.equal(soft[:, :, 36:48], source[:, :, 36:48])
    grown = pipe.composite_over_source(video, source, mask, grow=1, feather=0.5)                           # the latent mask's reach: 3 cells
    assert torch.equal(grown[:, :, 56:], source[:, :, 56:]) and torch.equal(grown[:, :, :56], e[:, :, :56])
    bad = [(dict(video=video[0]), "video"), (dict(video=video[:, :2]), "video"), (dict(video=video.long()), "video"),
           (dict(mask=torch.zeros(32, 64)), "does not match the video"), (dict(mask=torch.zeros(3, 64, 64)), "does not match the video"),
           (dict(mask=torch.zeros(60, 64)), "multiples of 8"), (dict(mask=torch.full((64, 64), 2.0)), r"\[0, 1\]"),
           (dict(source_frames=source.float()), "uint8"), (dict(source_frames=source[:1]), "do not match the video"),
           (dict(source_frames=source[:, :32]), "do not match the video"), (dict(source_frames=frames[:1]), "do not match the video"),
           (dict(source_frames=[f.resize((32, 32)) for f in frames]), "nothing is resized"), (dict(source_frames="clip.mp4"), "list of PIL"),
           (dict(grow=9), "grow=9"), (dict(feather=float("nan")), "feather=nan"), (dict(grow_px=65), "grow_px=65"), (dict(grow_px=-1), "grow_px"),
           (dict(grow_px=1.5), "grow_px"), (dict(grow_px=float("nan")), "grow_px"), (dict(feather_px=16.5), "feather_px"),
           (dict(feather_px=-0.1), "feather_px"), (dict(feather_px=float("nan")), "feather_px=nan"), (dict(match_color=1), "match_color")]
    for over, msg in bad:
        kw = dict(dict(video=video, source_frames=source, mask=mask), **over)
        with pytest.raises(ValueError, match=msg):
            pipe.composite_over_source(**kw)
    unet.frame_parallel = object()
    with pytest.raises(NotImplementedError, match="frame-parallel"):
        pipe.composite_over_source(video, source, mask)
    import inspect
    for call in ("__call__", "sample_with_pnp", "invert"):
        assert not any("composite" in p or p.endswith("_px") for p in inspect.signature(getattr(type(pipe), call)).parameters), call


def test_composite_options_refusals_and_defaults():
    from anyv2v_amd.config import OmegaConf, composite_options
    tmpl = OmegaConf.load(os.path.join(ROOT, "configs", "group_pnp_edit", "template.yaml"))
    mk = lambda **kw: OmegaConf.merge(tmpl, OmegaConf.create(kw))
    assert not any(k.startswith("edit_mask") for k in tmpl) and composite_options(tmpl) is None
    assert composite_options(mk(edit_mask_composite=False)) is None and composite_options(mk(edit_mask_composite=None)) is None
    assert composite_options(mk(edit_mask_path="m.png", edit_mask_composite=True)) == dict(grow_px=0, feather_px=0.0, match_color=False)
    assert composite_options(mk(edit_mask_auto=True, edit_mask_composite=True, edit_mask_composite_grow=4, edit_mask_composite_feather=2,
                                edit_mask_match_color=True)) == dict(grow_px=4, feather_px=2.0, match_color=True)
    assert composite_options(types.SimpleNamespace(edit_mask_path="m.png", edit_mask_composite=True, edit_mask_composite_grow=64,
                                                   edit_mask_composite_feather=16.0))["grow_px"] == 64
    on = dict(edit_mask_path="m.png", edit_mask_composite=True)
    for bad, msg in ((dict(edit_mask_composite=True), "without edit_mask_path or edit_mask_auto"),
                     (dict(edit_mask_composite=True, edit_mask_auto=False), "without edit_mask_path or edit_mask_auto"),
                     (dict(edit_mask_composite="yes", edit_mask_path="m.png"), "true or false"), (dict(on, edit_mask_match_color=1), "true or false"),
                     (dict(edit_mask_path="m.png", edit_mask_composite_grow=4), "without edit_mask_composite"),
                     (dict(edit_mask_path="m.png", edit_mask_composite_feather=2.0), "without edit_mask_composite"),
                     (dict(edit_mask_path="m.png", edit_mask_match_color=True), "without edit_mask_composite"),
                     (dict(edit_mask_path="m.png", edit_mask_composite=False, edit_mask_match_color=True), "without edit_mask_composite"),
                     (dict(on, edit_mask_composite_grow=65), "edit_mask_composite_grow"), (dict(on, edit_mask_composite_grow=-1), "edit_mask_composite_grow"),
                     (dict(on, edit_mask_composite_grow=1.5), "edit_mask_composite_grow"), (dict(on, edit_mask_composite_grow=True), "edit_mask_composite_grow"),
                     (dict(on, edit_mask_composite_grow=float("nan")), "edit_mask_composite_grow"),
                     (dict(on, edit_mask_composite_feather=16.5), "edit_mask_composite_feather"), (dict(on, edit_mask_composite_feather=-1), "edit_mask_composite_feather"),
                     (dict(on, edit_mask_composite_feather=float("nan")), "edit_mask_composite_feather")):
        with pytest.raises(ValueError, match=msg):
            composite_options(mk(**bad))


# ------------------------------------------------------------------------------------------------ configuration keys -> suffix -> files
def test_config_keys_through_the_runner(tmp_path, monkeypatch):
    """The keys extend the suffix only when on (absent: byte-identical to the pinned one) and reach ``composite_over_source`` through
    ``Stage2`` with the entry's mask, grow and feather; the PNG files written carry the SOURCE PNGs' pixels outside the mask and the
    ``to_pil`` bytes inside it; an entry without the keys calls nothing new and writes what ``to_pil`` gives."""
    import numpy as np
    from PIL import Image

    from anyv2v_amd.config import OmegaConf
    from anyv2v_amd.encoders import SyntheticVAE
    from anyv2v_amd.run_group_pnp_edit import Stage2, output_suffix
    from anyv2v_amd.schedulers import DDIMScheduler
    from anyv2v_amd.utils import LatentTrajectory
    cemu.install(monkeypatch)
    tmpl = OmegaConf.load(os.path.join(ROOT, "configs", "group_pnp_edit", "template.yaml"))
    entry = {"active": True, "task_name": "T", "video_name": "clip", "edited_first_frame_path": "demo/clip/e.png", "editing_prompt": "a robot",
             "edited_video_name": "robot"}
    base = "ddim_init_latents_t_idx_1_nsteps_50_cfg_9.0_pnpf0.2_pnps0.2_pnpt0.5"     # (pinned by tests/test_masked_edit_host.py)
    mk = lambda **kw: OmegaConf.merge(tmpl, OmegaConf.create(dict(entry, **kw)))
    assert output_suffix(mk(), 1) == base
    assert output_suffix(mk(edit_mask_path="demo/clip/hat.png"), 1) == base + "_mask-hat"
    assert output_suffix(mk(edit_mask_path="demo/clip/hat.png", edit_mask_composite=False), 1) == base + "_mask-hat"
    assert output_suffix(mk(edit_mask_path="demo/clip/hat.png", edit_mask_composite=True), 1) == base + "_mask-hat_comp"
    assert output_suffix(mk(edit_mask_path="demo/clip/hat.png", edit_mask_grow=2, edit_mask_composite=True, edit_mask_composite_grow=4,
                            edit_mask_composite_feather=2.5, edit_mask_match_color=True), 1) == base + "_mask-hat_grow2_comp_grow4_feather2.5_match"
    assert output_suffix(mk(edit_mask_auto=True, edit_mask_composite=True, edit_mask_match_color=True), 1) == base + "_mask-auto_comp_match"
    with pytest.raises(ValueError, match="without edit_mask_path or edit_mask_auto"):
        output_suffix(mk(edit_mask_composite=True), 1)
    # files
    g = torch.Generator().manual_seed(4)
    clip = tmp_path / "demo" / "clip"
    clip.mkdir(parents=True)
    source = torch.randint(0, 256, (2, 64, 64, 3), generator=g, dtype=torch.uint8)
    for i in range(2):
        Image.fromarray(source[i].numpy()).save(clip / f"{i:05d}.png")
    Image.fromarray(np.full((64, 64, 3), 99, dtype=np.uint8)).save(clip / "e.png")
    hat = np.zeros((64, 64), dtype=np.uint8)
    hat[:24, 8:40] = 255
    Image.fromarray(hat).save(clip / "hat.png")
    tmpl.data_dir, tmpl.device, tmpl.image_size, tmpl.n_frames, tmpl.n_steps = str(tmp_path), "cpu", [64, 64], 2, 4
    pipe, _unet = _meta_pipe()
    decoded = (torch.rand(1, 3, 2, 64, 64, generator=g) * 2.4 - 1.2).half()
    calls = []
    inner = pipe.composite_over_source

    def spy(video, source_frames, mask, **kw):
        calls.append(dict(kw, mask=mask.clone(), n=len(source_frames)))
        return inner(video, source_frames, mask, **kw)
    monkeypatch.setattr(pipe, "composite_over_source", spy)
    monkeypatch.setattr(pipe, "sample_with_pnp", lambda **kw: types.SimpleNamespace(frames=torch.zeros(1, 4, 2, 8, 8, dtype=torch.float16)))
    monkeypatch.setattr(pipe, "encode_vae_video", lambda frames, device=None, height=None, width=None: torch.zeros(1, 4, 2, 8, 8, dtype=torch.float16))
    monkeypatch.setattr(pipe, "auto_vae_tiling", lambda *a: None)
    monkeypatch.setattr(pipe, "decode_latents", lambda lat, decode_chunk_size=None: decoded.clone())
    pipe.vae = types.SimpleNamespace(to_pil=SyntheticVAE().to_pil)
    sched = DDIMScheduler()
    sched.set_timesteps(4)
    traj = LatentTrajectory()
    for t in sched.timesteps.tolist():
        traj[int(t)] = torch.zeros(1, 4, 2, 8, 8, dtype=torch.float16)
    lat_dir = os.path.abspath(str(OmegaConf.merge(tmpl, OmegaConf.create(entry)).ddim_latents_path))
    entries = [dict(entry), dict(entry, edit_mask_path="demo/clip/hat.png", edited_video_name="masked"),
               dict(entry, edit_mask_path="demo/clip/hat.png", edit_mask_composite=True, edited_video_name="hard"),
               dict(entry, edit_mask_path="demo/clip/hat.png", edit_mask_grow=1, edit_mask_feather=0.5, edit_mask_composite=True,
                    edit_mask_composite_grow=2, edit_mask_composite_feather=1.0, edit_mask_match_color=True, edited_video_name="soft")]
    stage = Stage2(tmpl, entries, torch.device("cpu"), logging.getLogger("composite"), pipe=pipe, trajectories={lat_dir: traj})
    for e in entries:
        stage.run_entry(e)

    def pngs(e):
        cfg = OmegaConf.merge(tmpl, OmegaConf.create(e))
        d = os.path.join(str(cfg.output_dir), output_suffix(cfg, 1))
        assert sorted(os.listdir(d)) == ["edited_latents.pt", "video.gif", "video.mp4", "video_00000.png", "video_00001.png"]
        return torch.from_numpy(np.stack([np.asarray(Image.open(os.path.join(d, f"video_{i:05d}.png")).convert("RGB")) for i in range(2)]))

    pil = spec.pil_bytes(decoded)[0].permute(1, 2, 3, 0)
    assert len(calls) == 2, "an entry without the composite key reached composite_over_source"
    assert torch.equal(pngs(entries[0]), pil) and torch.equal(pngs(entries[1]), pil), "keys absent: the files are not to_pil's"
    assert calls[0]["n"] == 2 and torch.equal(calls[0]["mask"][0], torch.from_numpy(hat)) and \
        {k: calls[0][k] for k in ("grow", "feather", "grow_px", "feather_px", "match_color")} == dict(grow=0, feather=0.0, grow_px=0, feather_px=0.0, match_color=False)
    assert {k: calls[1][k] for k in ("grow", "feather", "grow_px", "feather_px", "match_color")} == dict(grow=1, feather=0.5, grow_px=2, feather_px=1.0, match_color=True)
    inside = torch.from_numpy(hat > 0)
    hard = pngs(entries[2])
    assert torch.equal(hard[:, ~inside], source[:, ~inside]), "kept pixels are not the source PNGs' pixels"
    assert torch.equal(hard[:, inside], pil[:, inside]) and not torch.equal(hard, source)
    soft = pngs(entries[3])
    # latent reach: 1 cell grown + ceil(3 * 0.5) = 2 cells feathered -> 3 cells = 24 px beyond the hat; pixel reach 2 + 2 * 3 = 8 px more
    far = torch.ones(64, 64, dtype=torch.bool)
    far[: 24 + 32, : 40 + 32] = False
    assert int(far.sum()) > 0 and torch.equal(soft[:, far], source[:, far]), "beyond the reach the files are not the source's pixels"
    assert not torch.equal(soft, hard)
