"""Mask tracking without a GPU: the definition's own properties (``track_spec``), the CPU emulation against it, the configuration keys,
the header / binding table, the host-side validation of the C entry points, the two pipeline methods' refusals, and the runner end to end
under the CPU emulation."""
import ctypes
import logging
import os
import re
import types

import pytest
import torch

import cpu_track_emulation as temu
import track_spec as spec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def texture(H, W, seed, smooth=0):
    """Seeded random uint8 texture; ``smooth`` box-blur passes make neighbouring displacements nearly as good as the right one."""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(0, 256, (H, W), generator=g).float()
    for _ in range(smooth):
        t = torch.nn.functional.avg_pool2d(torch.nn.functional.pad(t[None, None], (1, 1, 1, 1), mode="replicate"), 3, stride=1)[0, 0]
    return t.round().to(torch.uint8)


def translated_pair(H, W, d, R, seed=0):
    """Y_1[p] = Y_0[p + d]: two crops of one larger texture."""
    big = texture(H + 2 * R, W + 2 * R, seed)
    return torch.stack([big[R: R + H, R: R + W], big[R + d[0]: R + d[0] + H, R + d[1]: R + d[1] + W]])


def inside_cells(H, W, d):
    """Cells whose displaced 16 x 16 window stays inside the frame."""
    cy, cx = torch.arange(H // 8) * 8 - 4 + d[0], torch.arange(W // 8) * 8 - 4 + d[1]
    return ((cy >= 0) & (cy + 16 <= H))[:, None] & ((cx >= 0) & (cx + 16 <= W))[None, :]


def periodic_pair(H, W, P, d, seed=0):
    g = torch.Generator().manual_seed(seed)
    block = torch.randint(0, 256, (P, P), generator=g, dtype=torch.uint8)
    big = block.repeat((H + 2 * P) // P + 2, (W + 2 * P) // P + 2)
    return torch.stack([big[P: P + H, P: P + W], big[P + d[0]: P + d[0] + H, P + d[1]: P + d[1] + W]])


# ------------------------------------------------------------------------------------------------ the definition's own properties
@pytest.mark.parametrize("d,R", [((3, -5), 6), ((-6, 6), 6), ((0, 7), 7), ((-2, 0), 3)])
def test_spec_recovers_a_known_translation(d, R):
    H, W = 48, 64
    flow = spec.block_match(translated_pair(H, W, d, R, seed=1), R)
    ok = inside_cells(H, W, d)
    assert int(ok.sum()) >= 6 and not bool(flow[0].any())
    assert torch.equal(flow[1][ok], torch.tensor(d, dtype=torch.int16).expand(int(ok.sum()), 2))


def test_spec_flat_and_saturated_frames_stay_put():
    flat = torch.full((3, 32, 40), 117, dtype=torch.uint8)
    assert not bool(spec.block_match(flat, 5).any())
    steps = torch.stack([torch.zeros(32, 40, dtype=torch.uint8), torch.full((32, 40), 255, dtype=torch.uint8)])
    assert not bool(spec.block_match(steps, 5).any())
    assert not bool(spec.block_match(translated_pair(32, 40, (2, 1), 4), 0).any()), "radius 0 has one candidate"


def test_spec_periodic_texture_gives_the_shortest_vector():
    """Period 8 <= R = 12, true shift (6, 5): (6, 5), (-2, 5), (6, -3), (-2, -3), ... all cost 0 where no window clamps; the shortest wins."""
    H = W = 64
    flow = spec.block_match(periodic_pair(H, W, 8, (6, 5)), 12)
    inner = flow[1, 2:6, 2:6]      # 8 c - 4 - 12 >= 0 and 8 c + 12 + 12 <= 64
    assert torch.equal(inner, torch.tensor([-2, -3], dtype=torch.int16).expand(4, 4, 2))


def test_spec_chain_per_pixel_equals_the_sequential_warp():
    g = torch.Generator().manual_seed(3)
    flow = torch.randint(-32, 33, (5, 5, 9, 2), generator=g).to(torch.int16)
    mask0 = torch.rand(40, 72, generator=g) < 0.4
    seq = spec.propagate(mask0, flow)
    assert torch.equal(seq, spec.propagate_chain(mask0, flow)) and torch.equal(seq[0], mask0)
    assert 0 < int(seq[4].sum()) < seq[4].numel()


def test_spec_median_and_first_frame_mask_edges():
    flow = torch.zeros(1, 4, 5, 2, dtype=torch.int16)
    flow[0, 0, 0] = torch.tensor([30, -30])          # a lone outlier in a corner: four of the nine clamped samples, not a majority
    flow[0, 2, 2, 0] = 9
    assert not bool(spec.flow_median(flow).any())
    flow[0, :2, :2, 1] = 7                            # a 2 x 2 corner patch: the corner cell sees it nine times over...
    med = spec.flow_median(flow)
    assert int(med[0, 0, 0, 1]) == 7 and int(med[0, 1, 1, 1]) == 0
    src = torch.full((16, 16, 3), 100, dtype=torch.uint8)
    ed = src.clone()
    ed[0, :8, 1] = 124                                # cell (0, 0): eight pixels at exactly the threshold
    ed[8, :7, 2] = 125                                # cell (1, 0): seven pixels over it
    ed[8:10, 8:12, 0] = 75                            # cell (1, 1): eight pixels over it, downwards
    m = spec.first_frame_mask(src, ed, 24, 8)
    assert m.dtype == torch.bool and tuple(m.shape) == (1, 16, 16)
    assert torch.equal(m[0, ::8, ::8], torch.tensor([[False, False], [False, True]])) and bool(m[0, 8:, 8:].all())
    assert bool(spec.first_frame_mask(src, ed, 24, 7)[0, 8, 0]) and bool(spec.first_frame_mask(src, ed, 23, 8)[0, 0, 0])


# ------------------------------------------------------------------------------------------------ the emulation against the definition
def moving_clip(F, H, W, seed, smooth=1):
    """Frames of one texture under a smooth motion: a global drift plus a slower drift of the right half."""
    big = texture(H + 32, W + 32, seed, smooth)
    frames = []
    for k in range(F):
        a = big[16 + 2 * k: 16 + 2 * k + H, 16 - 3 * k: 16 - 3 * k + W].clone()
        a[:, W // 2:] = big[16 + k: 16 + k + H, 16 - k + W // 2: 16 - k + W]
        frames.append(a)
    return torch.stack(frames)


@pytest.mark.parametrize("F,H,W,R", [(3, 32, 40, 5), (2, 24, 24, 12), (2, 16, 16, 0), (1, 16, 24, 4)])
def test_emulation_against_the_definition(F, H, W, R):
    g = torch.Generator().manual_seed(F * 100 + R)
    y = moving_clip(F, H, W, seed=R)
    rgb = torch.randint(0, 256, (F, H, W, 3), generator=g, dtype=torch.uint8)
    assert torch.equal(temu.luma_u8(rgb), spec.luma(rgb))
    flow = spec.block_match(y, R)
    assert torch.equal(temu.block_match(y, R), flow)
    noisy = torch.randint(-32, 33, (F, H // 8, W // 8, 2), generator=g).to(torch.int16)
    assert torch.equal(temu.flow_median(noisy), spec.flow_median(noisy))
    mask0 = torch.rand(H, W, generator=g) < 0.5
    assert torch.equal(temu.mask_propagate(mask0, noisy), spec.propagate(mask0, noisy))
    assert torch.equal(temu.mask_propagate(mask0.to(torch.uint8) * 255, noisy), spec.propagate(mask0, noisy))
    ed = torch.where(torch.rand(H, W, 1, generator=g) < 0.2, rgb[0] // 2, rgb[0])
    for thr, cnt in ((24, 8), (0, 1), (60, 64)):
        assert torch.equal(temu.first_frame_mask(rgb[0], ed, thr, cnt), spec.first_frame_mask(rgb[0], ed, thr, cnt))


# ------------------------------------------------------------------------------------------------ header, binding, validation
SYMS = (("anyv2v_luma_u8", 6), ("anyv2v_block_match_u8", 7), ("anyv2v_flow_median_i16", 6), ("anyv2v_mask_propagate_u8", 7),
        ("anyv2v_first_frame_mask_u8", 8))


def test_header_binding_and_abi_version():
    from anyv2v_amd import _lib, ops
    hdr = open(os.path.join(ROOT, "include", "anyv2v_hip.h")).read()
    for sym, nargs in SYMS:
        decl = re.search(r"\bint %s\s*\(([^;]*)\);" % sym, hdr)
        assert decl and len(decl.group(1).split(",")) == nargs, sym
        assert sym in _lib.SYMBOLS and len(_lib.SYMBOLS[sym][1]) == nargs, sym
        if os.path.isfile(_lib.LIB_PATH):
            assert hasattr(ctypes.CDLL(_lib.LIB_PATH), sym)
    assert re.search(r"#define ANYV2V_TRACK_MAX_RADIUS (\d+)", hdr).group(1) == str(_lib.TRACK_MAX_RADIUS) == "32"
    assert "(77 R + 150 G + 29 B + 128) >> 8" in hdr and "(cost, dy^2 + dx^2, dy, dx)" in hdr
    for name in ("luma_u8", "block_match", "flow_median", "mask_propagate", "first_frame_mask"):
        assert callable(getattr(ops, name)), name
    assert _lib.ABI_VERSION == 105 and "#define ANYV2V_ABI_VERSION 105" in hdr
    mk = open(os.path.join(ROOT, "anyv2v_amd", "csrc", "Makefile")).read()
    assert re.search(r"^SRCS\s*:=.*\btrack\.hip\b", mk, re.M)
    assert len(re.findall(r"\btrack\.o\b", mk)) == 2, "both object lists of the experiments target"


def test_abi_validation_without_gpu():
    """Host-side validation returns ANYV2V_EINVAL (-1) with a message before anything touches a device."""
    from anyv2v_amd import _lib
    if not os.path.isfile(_lib.LIB_PATH):
        pytest.skip("libanyv2v_hip.so is not built")
    lib = _lib.load()
    P = 4096   # any aligned non-null address: nothing on the device is dereferenced before the checks
    calls = {
        "luma": (lambda a: lib.anyv2v_luma_u8(a["x"], a["y"], a["F"], a["H"], a["W"], None), ("x", "y")),
        "block_match": (lambda a: lib.anyv2v_block_match_u8(a["x"], a["y"], a["F"], a["H"], a["W"], a["R"], None), ("x", "y")),
        "mask_propagate": (lambda a: lib.anyv2v_mask_propagate_u8(a["x"], a["y"], a["z"], a["F"], a["H"], a["W"], None), ("x", "y", "z")),
        "first_frame_mask": (lambda a: lib.anyv2v_first_frame_mask_u8(a["x"], a["y"], a["z"], a["H"], a["W"], a["thr"], a["cnt"], None),
                             ("x", "y", "z")),
    }
    good = dict(x=P, y=2 * P, z=3 * P, F=2, H=16, W=24, R=4, thr=24, cnt=8)
    for what, (fn, ptrs) in calls.items():
        for name in ptrs:
            assert fn(dict(good, **{name: None})) == -1 and b"null pointer" in lib.anyv2v_last_error(), (what, name)
        for over in (dict(H=12), dict(W=20), dict(H=0), dict(W=-8)):
            assert fn(dict(good, **over)) == -1 and b"multiples of 8" in lib.anyv2v_last_error(), (what, over)
        assert what.encode() in lib.anyv2v_last_error()
        if what != "first_frame_mask":
            for F in (0, -1):
                assert fn(dict(good, F=F)) == -1 and b"F = " in lib.anyv2v_last_error(), (what, F)
            assert fn(dict(good, F=1 << 10, H=1 << 10, W=1 << 10)) == -1 and b"fit an int" in lib.anyv2v_last_error()
    for R in (-1, 33):
        assert calls["block_match"][0](dict(good, R=R)) == -1 and b"radius" in lib.anyv2v_last_error()
    assert calls["block_match"][0](dict(good, y=2 * P + 2)) == -1 and b"4-byte aligned" in lib.anyv2v_last_error()
    assert calls["mask_propagate"][0](dict(good, z=P)) == -1 and b"may not alias" in lib.anyv2v_last_error()
    for over, msg in ((dict(thr=-1), b"threshold"), (dict(thr=256), b"threshold"), (dict(cnt=0), b"min_count"), (dict(cnt=65), b"min_count"),
                      (dict(z=2 * P), b"may not alias")):
        assert calls["first_frame_mask"][0](dict(good, **over)) == -1 and msg in lib.anyv2v_last_error(), over
    med = lambda **o: (lambda a: lib.anyv2v_flow_median_i16(a["x"], a["y"], a["F"], a["h"], a["w"], None))(dict(dict(x=P, y=2 * P, F=2, h=2, w=3), **o))
    for o, msg in ((dict(x=None), b"null pointer"), (dict(y=None), b"null pointer"), (dict(F=0), b"F = "), (dict(h=0), b"at least 1"),
                   (dict(w=-1), b"at least 1"), (dict(y=P), b"may not alias"), (dict(F=1 << 12, h=1 << 10, w=1 << 10), b"fit an int")):
        assert med(**o) == -1 and msg in lib.anyv2v_last_error(), o


# ------------------------------------------------------------------------------------------------ the pipeline's two methods
def _meta_pipe():
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMScheduler
    from anyv2v_amd.unet import I2VGenXLUNet, I2VGenXLUNetConfig
    with torch.device("meta"):
        unet = I2VGenXLUNet(I2VGenXLUNetConfig.mini())
    return I2VGenXLPipeline(unet=unet, scheduler=DDIMScheduler()), unet


def _rgb_clip(F=3, H=32, W=40, seed=5):
    return moving_clip(F, H, W, seed)[..., None].expand(F, H, W, 3).contiguous()


def test_pipeline_methods_forms_and_refusals(monkeypatch):
    import inspect

    from PIL import Image
    temu.install(monkeypatch)
    pipe, _unet = _meta_pipe()
    frames = _rgb_clip()
    edited = frames[0].clone()
    edited[8:24, 8:24] = 255 - edited[8:24, 8:24] // 2
    want0 = spec.first_frame_mask(frames[0], edited)
    m0 = pipe.first_frame_edit_mask(frames[0], edited)
    assert m0.dtype == torch.bool and torch.equal(m0, want0) and bool(m0.any()) and not bool(m0.all())
    assert torch.equal(pipe.first_frame_edit_mask(Image.fromarray(frames[0].numpy()), Image.fromarray(edited.numpy())), want0)
    assert torch.equal(pipe.first_frame_edit_mask(frames[0], edited, threshold=200, min_count=64), spec.first_frame_mask(frames[0], edited, 200, 64))
    want, flow = spec.track(frames, want0[0], 6, True)
    got, gflow = pipe.propagate_edit_mask(frames, m0, radius=6, return_flow=True)
    assert got.dtype == torch.bool and torch.equal(got, want) and gflow.dtype == torch.int16 and torch.equal(gflow, flow)
    assert bool(flow.any()) and not torch.equal(got[2], got[0]), "the clip moves: the test would say nothing otherwise"
    pil = [Image.fromarray(f.numpy()) for f in frames]
    assert torch.equal(pipe.propagate_edit_mask(pil, m0[0], radius=6), want)
    assert torch.equal(pipe.propagate_edit_mask(pil, m0[0].to(torch.uint8) * 255, radius=6), want)
    assert torch.equal(pipe.propagate_edit_mask(frames, m0, radius=6, median=False), spec.track(frames, want0[0], 6, False)[0])
    assert torch.equal(pipe.propagate_edit_mask(frames[:1], m0), want0)
    for kw, msg in ((dict(edited_first_frame=edited[:24]), "does not match"), (dict(edited_first_frame=edited.float()), "uint8"),
                    (dict(source_first_frame=frames), "one frame"), (dict(source_first_frame=frames[0, :30], edited_first_frame=edited[:30]), "multiples of 8"),
                    (dict(edited_first_frame="e.png"), "PIL images or"), (dict(threshold=256), "threshold=256"), (dict(threshold=-1), "threshold"),
                    (dict(threshold=1.5), "threshold"), (dict(threshold=float("nan")), "threshold"), (dict(threshold=True), "threshold"),
                    (dict(min_count=0), "min_count=0"), (dict(min_count=65), "min_count"), (dict(min_count=2.5), "min_count")):
        with pytest.raises(ValueError, match=msg):
            pipe.first_frame_edit_mask(**dict(dict(source_first_frame=frames[0], edited_first_frame=edited), **kw))
    for kw, msg in ((dict(mask=m0.expand(3, 32, 40)), "already has 3 frames"), (dict(mask=m0[0, :24]), "does not match the frames"),
                    (dict(mask=m0.float()), "bool or uint8"), (dict(mask=[m0]), "tensor expected"), (dict(mask=m0[None]), "tensor expected"),
                    (dict(source_frames=frames.float()), "uint8"), (dict(source_frames=frames[..., :2]), r"\[F, H, W, 3\]"),
                    (dict(source_frames=[pil[0], pil[1].resize((16, 16))]), "different sizes"), (dict(source_frames="clip.mp4"), "PIL images or"),
                    (dict(radius=33), "radius=33"), (dict(radius=-1), "radius"), (dict(radius=2.5), "radius"), (dict(radius=float("nan")), "radius"),
                    (dict(radius=True), "radius"), (dict(median=1), "median")):
        with pytest.raises(ValueError, match=msg):
            pipe.propagate_edit_mask(**dict(dict(source_frames=frames, mask=m0), **kw))
    assert pipe._masked_edit is None, "neither method sets the masked edit"
    for call in ("__call__", "sample_with_pnp", "invert"):
        assert not any("track" in p or "first_frame_edit" in p for p in inspect.signature(getattr(type(pipe), call)).parameters), call
    assert "edit_mask_grow" in type(pipe).propagate_edit_mask.__doc__ and "Occlusion" in type(pipe).propagate_edit_mask.__doc__


# ------------------------------------------------------------------------------------------------ configuration keys
def test_options_acceptance_and_refusals():
    from anyv2v_amd.config import (OmegaConf, auto_mask_options, composite_options, first_frame_mask_options, masked_edit_options,
                                   track_options)
    tmpl = OmegaConf.load(os.path.join(ROOT, "configs", "group_pnp_edit", "template.yaml"))
    mk = lambda **kw: OmegaConf.merge(tmpl, OmegaConf.create(kw))
    assert not any(k.startswith("edit_mask") for k in tmpl)
    for off in (tmpl, mk(edit_mask_first_frame=False, edit_mask_track=False), mk(edit_mask_first_frame=None, edit_mask_track=None)):
        assert first_frame_mask_options(off) is None and track_options(off) is None
    ff = mk(edit_mask_first_frame=True)
    assert first_frame_mask_options(ff) == dict(threshold=24, min_count=8, grow=0, feather=0.0) and track_options(ff) is None
    assert masked_edit_options(ff) is None and auto_mask_options(ff) is None and composite_options(ff) is None
    full = mk(edit_mask_first_frame=True, edit_mask_first_frame_threshold=40, edit_mask_first_frame_min_count=1, edit_mask_grow=2,
              edit_mask_feather=1.5, edit_mask_track=True, edit_mask_track_radius=32, edit_mask_track_median=False, edit_mask_composite=True)
    assert first_frame_mask_options(full) == dict(threshold=40, min_count=1, grow=2, feather=1.5)
    assert track_options(full) == dict(radius=32, median=False) and masked_edit_options(full) is None
    assert composite_options(full) == dict(grow_px=0, feather_px=0.0, match_color=False)
    assert track_options(mk(edit_mask_path="m.png", edit_mask_track=True)) == dict(radius=16, median=True)
    assert track_options(types.SimpleNamespace(edit_mask_first_frame=True, edit_mask_track=True, edit_mask_track_radius=0))["radius"] == 0
    for fn, bad, msg in (
            (first_frame_mask_options, dict(edit_mask_first_frame="yes"), "true or false"),
            (first_frame_mask_options, dict(edit_mask_first_frame_threshold=30), "without edit_mask_first_frame"),
            (first_frame_mask_options, dict(edit_mask_first_frame=False, edit_mask_first_frame_min_count=4), "without edit_mask_first_frame"),
            (first_frame_mask_options, dict(edit_mask_first_frame=True, edit_mask_path="m.png"), "together with edit_mask_path"),
            (masked_edit_options, dict(edit_mask_first_frame=True, edit_mask_path="m.png"), "together with edit_mask_path"),
            (first_frame_mask_options, dict(edit_mask_first_frame=True, edit_mask_auto=True), "together with edit_mask_auto"),
            (auto_mask_options, dict(edit_mask_first_frame=True, edit_mask_auto=True), "together with edit_mask_auto"),
            (first_frame_mask_options, dict(edit_mask_first_frame=True, edit_mask_first_frame_threshold=256), "edit_mask_first_frame_threshold"),
            (first_frame_mask_options, dict(edit_mask_first_frame=True, edit_mask_first_frame_threshold=-1), "edit_mask_first_frame_threshold"),
            (first_frame_mask_options, dict(edit_mask_first_frame=True, edit_mask_first_frame_threshold=1.5), "edit_mask_first_frame_threshold"),
            (first_frame_mask_options, dict(edit_mask_first_frame=True, edit_mask_first_frame_min_count=0), "edit_mask_first_frame_min_count"),
            (first_frame_mask_options, dict(edit_mask_first_frame=True, edit_mask_first_frame_min_count=65), "edit_mask_first_frame_min_count"),
            (first_frame_mask_options, dict(edit_mask_first_frame=True, edit_mask_first_frame_min_count=True), "edit_mask_first_frame_min_count"),
            (first_frame_mask_options, dict(edit_mask_first_frame=True, edit_mask_grow=9), "edit_mask_grow"),
            (track_options, dict(edit_mask_track=True), "without edit_mask_first_frame or edit_mask_path"),
            (track_options, dict(edit_mask_track=True, edit_mask_auto=True), "together with edit_mask_auto"),
            (track_options, dict(edit_mask_track=1, edit_mask_first_frame=True), "true or false"),
            (track_options, dict(edit_mask_track=True, edit_mask_first_frame=True, edit_mask_track_median="no"), "true or false"),
            (track_options, dict(edit_mask_first_frame=True, edit_mask_track_radius=8), "without edit_mask_track"),
            (track_options, dict(edit_mask_first_frame=True, edit_mask_track=False, edit_mask_track_median=False), "without edit_mask_track"),
            (track_options, dict(edit_mask_first_frame=True, edit_mask_track=True, edit_mask_track_radius=33), "edit_mask_track_radius"),
            (track_options, dict(edit_mask_first_frame=True, edit_mask_track=True, edit_mask_track_radius=-1), "edit_mask_track_radius"),
            (track_options, dict(edit_mask_first_frame=True, edit_mask_track=True, edit_mask_track_radius=2.5), "edit_mask_track_radius"),
            (track_options, dict(edit_mask_first_frame=True, edit_mask_track=True, edit_mask_track_radius=float("nan")), "edit_mask_track_radius")):
        with pytest.raises(ValueError, match=msg):
            fn(mk(**bad))
    # the three earlier option functions on their earlier inputs: results and messages as before the keys existed
    assert masked_edit_options(mk(edit_mask_path="m.png", edit_mask_grow=2, edit_mask_feather=1.0)) == ("m.png", 2, 1.0)
    assert auto_mask_options(mk(edit_mask_auto=True, edit_mask_auto_maps=3, edit_mask_grow=1)) == \
        dict(maps=3, strength=0.5, ratio=3.0, threshold=0.5, grow=1, feather=0.0)
    assert composite_options(mk(edit_mask_auto=True, edit_mask_composite=True, edit_mask_composite_grow=4)) == dict(grow_px=4, feather_px=0.0, match_color=False)
    assert masked_edit_options(mk(edit_mask_auto=True, edit_mask_grow=2)) is None
    for fn, bad, msg in ((masked_edit_options, dict(edit_mask_grow=2), "edit_mask_grow / edit_mask_feather without edit_mask_path"),
                         (masked_edit_options, dict(edit_mask_path="m.png", edit_mask_auto=True), "edit_mask_auto together with edit_mask_path"),
                         (auto_mask_options, dict(edit_mask_path="m.png", edit_mask_auto=True), "edit_mask_auto together with edit_mask_path"),
                         (auto_mask_options, dict(edit_mask_auto_maps=3), "edit_mask_auto_maps without edit_mask_auto"),
                         (composite_options, dict(edit_mask_composite=True), "without edit_mask_path or edit_mask_auto"),
                         (composite_options, dict(edit_mask_first_frame=False, edit_mask_composite=True), "without edit_mask_path or edit_mask_auto")):
        with pytest.raises(ValueError, match=msg):
            fn(mk(**bad))


ENTRY = {"active": True, "task_name": "T", "video_name": "clip", "edited_first_frame_path": "demo/clip/e.png", "editing_prompt": "a robot",
         "edited_video_name": "robot"}
BASE = "ddim_init_latents_t_idx_1_nsteps_50_cfg_9.0_pnpf0.2_pnps0.2_pnpt0.5"     # (pinned by tests/test_masked_edit_host.py)


def test_output_suffix():
    from anyv2v_amd.config import OmegaConf
    from anyv2v_amd.run_group_pnp_edit import output_suffix
    tmpl = OmegaConf.load(os.path.join(ROOT, "configs", "group_pnp_edit", "template.yaml"))
    mk = lambda **kw: OmegaConf.merge(tmpl, OmegaConf.create(dict(ENTRY, **kw)))
    for kw, tag in ((dict(), ""), (dict(edit_mask_first_frame=False, edit_mask_track=False), ""),
                    (dict(edit_mask_path="demo/clip/hat.png", edit_mask_grow=2), "_mask-hat_grow2"),
                    (dict(edit_mask_auto=True, edit_mask_composite=True), "_mask-auto_comp"),
                    (dict(edit_mask_first_frame=True), "_mask-ff"),
                    (dict(edit_mask_first_frame=True, edit_mask_first_frame_threshold=24, edit_mask_first_frame_min_count=8, edit_mask_track=True,
                          edit_mask_track_radius=16, edit_mask_track_median=True), "_mask-ff-track"),
                    (dict(edit_mask_first_frame=True, edit_mask_first_frame_threshold=30, edit_mask_first_frame_min_count=4, edit_mask_grow=1,
                          edit_mask_feather=0.5), "_mask-ff_threshold30_min_count4_grow1_feather0.5"),
                    (dict(edit_mask_first_frame=True, edit_mask_track=True, edit_mask_track_radius=8, edit_mask_track_median=False, edit_mask_grow=2,
                          edit_mask_composite=True, edit_mask_match_color=True), "_mask-ff-track_radius8_nomedian_grow2_comp_match"),
                    (dict(edit_mask_path="demo/clip/hat.png", edit_mask_track=True), "_mask-hat-track"),
                    (dict(edit_mask_path="demo/clip/hat.png", edit_mask_track=True, edit_mask_track_radius=32, edit_mask_feather=1.0),
                     "_mask-hat-track_radius32_feather1.0")):
        assert output_suffix(mk(**kw), 1) == BASE + tag, kw
    for kw, msg in ((dict(edit_mask_track=True), "without edit_mask_first_frame or edit_mask_path"),
                    (dict(edit_mask_first_frame=True, edit_mask_auto=True), "together with edit_mask_auto"),
                    (dict(edit_mask_first_frame_threshold=30), "without edit_mask_first_frame")):
        with pytest.raises(ValueError, match=msg):
            output_suffix(mk(**kw), 1)


# ------------------------------------------------------------------------------------------------ the runner, end to end
def test_first_frame_mask_tracked_through_the_runner(tmp_path, monkeypatch):
    """``edit_mask_first_frame`` + ``edit_mask_track`` + ``edit_mask_composite`` through ``Stage2`` on the mini checkpoint under the CPU
    emulation: the ``mask_%05d.png`` files are the definition's tracked mask, the mask reaches ``enable_masked_edit`` and the composite,
    the directory name carries the suffix; an entry without the keys writes no mask file; a directory of masks is refused."""
    import numpy as np
    from PIL import Image

    from anyv2v_amd.config import OmegaConf
    from anyv2v_amd.encoders import SyntheticVAE
    from anyv2v_amd.run_group_pnp_edit import Stage2, output_suffix
    from anyv2v_amd.schedulers import DDIMScheduler
    from anyv2v_amd.utils import LatentTrajectory
    temu.install(monkeypatch)
    tmpl = OmegaConf.load(os.path.join(ROOT, "configs", "group_pnp_edit", "template.yaml"))
    F, H, W = 3, 64, 64
    source = _rgb_clip(F, H, W, seed=9).clone()
    source[..., 1] = 255 - source[..., 1]
    edited = source[0].clone()
    edited[16:40, 24:48] = 255 - edited[16:40, 24:48]
    clip = tmp_path / "demo" / "clip"
    clip.mkdir(parents=True)
    for i in range(F):
        Image.fromarray(source[i].numpy()).save(clip / f"{i:05d}.png")
    Image.fromarray(edited.numpy()).save(clip / "e.png")
    (clip / "masks").mkdir()
    hat = np.zeros((H, W), dtype=np.uint8)
    hat[8:24, 8:40] = 255
    Image.fromarray(hat).save(clip / "hat.png")
    tmpl.data_dir, tmpl.device, tmpl.image_size, tmpl.n_frames, tmpl.n_steps = str(tmp_path), "cpu", [W, H], F, 4
    pipe, _unet = _meta_pipe()
    g = torch.Generator().manual_seed(4)
    decoded = (torch.rand(1, 3, F, H, W, generator=g) * 2.4 - 1.2).half()
    seen = dict(edit=[], comp=[])
    inner_edit, inner_comp = pipe.enable_masked_edit, pipe.composite_over_source
    monkeypatch.setattr(pipe, "enable_masked_edit", lambda mask, lat, **kw: (seen["edit"].append(mask.clone()), inner_edit(mask, lat, **kw))[1])
    monkeypatch.setattr(pipe, "composite_over_source", lambda v, s, mask, **kw: (seen["comp"].append(mask.clone()), inner_comp(v, s, mask, **kw))[1])
    zeros = lambda *a, **kw: torch.zeros(1, 4, F, H // 8, W // 8, dtype=torch.float16)
    monkeypatch.setattr(pipe, "sample_with_pnp", lambda **kw: types.SimpleNamespace(frames=zeros()))
    monkeypatch.setattr(pipe, "encode_vae_video", zeros)
    monkeypatch.setattr(pipe, "auto_vae_tiling", lambda *a: None)
    monkeypatch.setattr(pipe, "decode_latents", lambda lat, decode_chunk_size=None: decoded.clone())
    pipe.vae = types.SimpleNamespace(to_pil=SyntheticVAE().to_pil)
    sched = DDIMScheduler()
    sched.set_timesteps(4)
    traj = LatentTrajectory()
    for t in sched.timesteps.tolist():
        traj[int(t)] = zeros()
    lat_dir = os.path.abspath(str(OmegaConf.merge(tmpl, OmegaConf.create(ENTRY)).ddim_latents_path))
    entries = [dict(ENTRY),
               dict(ENTRY, edit_mask_first_frame=True, edit_mask_track=True, edit_mask_track_radius=6, edit_mask_composite=True, edited_video_name="tracked"),
               dict(ENTRY, edit_mask_first_frame=True, edited_video_name="static"),
               dict(ENTRY, edit_mask_path="demo/clip/hat.png", edit_mask_track=True, edit_mask_track_radius=6, edited_video_name="hat"),
               dict(ENTRY, edit_mask_path="demo/clip/masks", edit_mask_track=True, edited_video_name="dir")]
    stage = Stage2(tmpl, entries, torch.device("cpu"), logging.getLogger("track"), pipe=pipe, trajectories={lat_dir: traj})
    for e in entries[:4]:
        stage.run_entry(e)
    with pytest.raises(ValueError, match="directory of masks"):
        stage.run_entry(entries[4])

    def out_dir(e):
        cfg = OmegaConf.merge(tmpl, OmegaConf.create(e))
        return os.path.join(str(cfg.output_dir), output_suffix(cfg, 1))

    def mask_pngs(e):
        names = sorted(n for n in os.listdir(out_dir(e)) if n.startswith("mask_"))
        return names, [torch.from_numpy(np.array(Image.open(os.path.join(out_dir(e), n)))) for n in names]

    base = BASE.replace("nsteps_50", "nsteps_4")
    assert os.path.basename(out_dir(entries[0])) == base and mask_pngs(entries[0])[0] == []
    assert os.path.basename(out_dir(entries[1])) == base + "_mask-ff-track_radius6_comp"
    assert os.path.basename(out_dir(entries[2])) == base + "_mask-ff" and os.path.basename(out_dir(entries[3])) == base + "_mask-hat-track_radius6"
    m0 = spec.first_frame_mask(source[0], edited)
    want, flow = spec.track(source, m0[0], 6, True)
    assert bool(flow.any()) and not torch.equal(want[2], want[0]) and 0 < int(want[2].sum()) < H * W
    names, planes = mask_pngs(entries[1])
    assert names == [f"mask_{i:05d}.png" for i in range(F)]
    assert torch.equal(torch.stack(planes), want.to(torch.uint8) * 255), "the mask files are not the definition's tracked mask"
    names, planes = mask_pngs(entries[2])
    assert names == ["mask_00000.png"] and torch.equal(planes[0], m0[0].to(torch.uint8) * 255)
    names, planes = mask_pngs(entries[3])
    assert len(names) == F and torch.equal(torch.stack(planes), spec.track(source, torch.from_numpy(hat), 6, True)[0].to(torch.uint8) * 255)
    assert len(seen["edit"]) == 3 and len(seen["comp"]) == 1
    assert torch.equal(seen["edit"][0], want) and torch.equal(seen["comp"][0], want) and torch.equal(seen["edit"][1], m0)
    # the composite pastes the source back outside the tracked mask, frame by frame
    video = torch.from_numpy(np.stack([np.asarray(Image.open(os.path.join(out_dir(entries[1]), f"video_{i:05d}.png")).convert("RGB")) for i in range(F)]))
    kept = ~torch.nn.functional.max_pool2d(want[None].float(), 8)[0].bool().repeat_interleave(8, 1).repeat_interleave(8, 2)   # cells the mask misses
    assert int(kept.sum()) > 0 and torch.equal(video[kept], source[kept]) and not torch.equal(video, source)
    assert pipe._masked_edit is None
