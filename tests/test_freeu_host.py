"""FreeU without a GPU: the closed form the kernel evaluates against the ``torch.fft`` definition, the UNet / pipeline wiring under
the CPU op emulation against the hooked oracle, and the C ABI's host-side validation (tests/freeu_spec.py holds the definitions)."""
import ctypes
import math
import os
import re

import pytest
import torch

import freeu_spec as spec
import gpu_checks as gc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FREEU = (0.9, 0.2, 1.2, 1.4)   # s1, s2, b1, b2
SIZES = [(1, 1), (1, 4), (4, 1), (2, 2), (2, 3), (5, 7), (8, 8), (16, 16), (22, 40)]


@pytest.fixture()
def cpu_ops(monkeypatch):
    spec.install(monkeypatch)
    monkeypatch.setattr(gc, "DEV", "cpu")
    monkeypatch.setenv("ANYV2V_NO_GRAPH", "1")
    yield


@pytest.mark.parametrize("H,W", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_closed_form_equals_the_fft_definition_in_fp64(H, W):
    g = torch.Generator().manual_seed(100 * H + W)
    x = 1.5 * torch.randn(2, 3, H, W, generator=g, dtype=torch.float64) + 2
    for s in (0.2, 0.9, 1.0, 2.5):
        d = float((spec.fourier_filter_closed(x, s) - spec.fourier_filter_fft(x, s)).abs().max())
        print(f"[freeu] {H}x{W} s={s}: closed form vs torch.fft max |diff| {d:.2e}")
        assert d <= 1e-12


def test_single_frequency_facts():
    """The box is not Hermitian-symmetric: a (1, 0) cosine is scaled through its partner (-1, 0) only, by 1 + (s - 1) / 2; a (1, -1)
    cosine (partner (-1, 1), outside the box too) is unchanged; a constant is scaled by s."""
    H, W, s = 8, 6, 0.2
    h = torch.arange(H, dtype=torch.float64)[:, None].expand(H, W)
    w = torch.arange(W, dtype=torch.float64)[None, :].expand(H, W)
    cos10 = torch.cos(2 * math.pi * h / H)[None, None]
    cos1m1 = torch.cos(2 * math.pi * (h / H - w / W))[None, None]
    const = torch.full((1, 1, H, W), 3.0, dtype=torch.float64)
    for f in (spec.fourier_filter_fft, spec.fourier_filter_closed):
        assert float((f(cos10, s) - (1 + (s - 1) / 2) * cos10).abs().max()) <= 1e-12
        assert float((f(cos1m1, s) - cos1m1).abs().max()) <= 1e-12
        assert float((f(const, s) - s * const).abs().max()) <= 1e-12


def _mini_case():
    native, oracle, ocfg = gc.build_pair("mini", 1234)
    inp = gc.config1_inputs(ocfg, 3, 2, (24, 40))
    inp16 = {k: (v.half() if v.is_floating_point() else v) for k, v in inp.items()}
    return native, oracle, inp16


def test_mini_unet_with_freeu_vs_hooked_oracle(cpu_ops):
    """B = 3, F = 2, latent 24 x 40 (up_blocks[0] at 3 x 5, up_blocks[1] at 6 x 10): the native UNet under the op emulation with FreeU on
    against the oracle with the definition hooked in, within the CPU-emulation bound of ``check_unet_vs_oracle`` (3e-2) -- and FreeU
    moves the prediction by more than that bound; enable followed by disable is bit-equal to never enabled."""
    tol = 3e-2
    native, oracle, inp16 = _mini_case()
    kw_o, kw_n = gc._cond_kw(inp16, "cpu", torch.float32), gc._cond_kw(inp16, "cpu", torch.float16)
    v_off = native(inp16["sample"], 981, **kw_n)[0].clone()
    native.enable_freeu(*FREEU)
    assert native.freeu == FREEU
    assert native.up_blocks[0].freeu == (1.2, 0.9) and native.up_blocks[1].freeu == (1.4, 0.2)
    assert native.up_blocks[2].freeu is None and native.up_blocks[3].freeu is None
    v_on = native(inp16["sample"], 981, **kw_n)[0].clone()
    handles = spec.hook_oracle(oracle, *FREEU)
    try:
        with torch.no_grad():
            vo = oracle(inp16["sample"].float(), 981, **kw_o)[0]
    finally:
        for h in handles:
            h.remove()
    r = gc._res("mini unet B3 F2 24x40 + FreeU vs hooked oracle", v_on, vo, tol)
    moved = gc._res("FreeU on vs off", v_on, v_off.float(), tol)
    print(f"[freeu] vs hooked oracle: max {r['err']:.3e} l2 {r['l2']:.3e} (tol {tol}); on vs off: max {moved['err']:.3e} l2 {moved['l2']:.3e}")
    assert r["ok"], r
    assert moved["err"] > tol and moved["l2"] > tol, "FreeU does not move the prediction: the comparison above would be vacuous"
    native.disable_freeu()
    assert native.freeu is None
    assert torch.equal(native(inp16["sample"], 981, **kw_n)[0], v_off), "enable + disable is not bit-equal to never enabled"


def test_freeu_off_makes_no_freeu_call(cpu_ops, monkeypatch):
    """The default path: ``ops.freeu`` is not reached at all (no launch, no allocation); on: three calls per block, blocks 0 and 1."""
    from anyv2v_amd import ops
    calls = []
    inner = ops.freeu
    monkeypatch.setattr(ops, "freeu", lambda *a, **k: (calls.append((a[3], a[4], a[5], a[6])), inner(*a, **k))[1])
    native, _, ocfg = gc.build_pair("mini", 1234)
    inp = gc.config1_inputs(ocfg, 1, 2, (24, 40))
    kw = dict(fps=inp["fps"], image_latents=inp["image_latents"].half(), image_embeddings=inp["image_embeddings"].half(),
              encoder_hidden_states=inp["encoder_hidden_states"].half())
    native(inp["sample"].half(), 981, **kw)
    assert calls == []
    native.enable_freeu(*FREEU)
    native(inp["sample"].half(), 981, **kw)
    assert calls == [(3, 5, 1.2, 0.9)] * 3 + [(6, 10, 1.4, 0.2)] * 3


def test_enable_freeu_refuses_what_it_cannot_do():
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.unet import I2VGenXLUNet, I2VGenXLUNetConfig
    with pytest.raises(NotImplementedError, match="needs a UNet"):
        I2VGenXLPipeline().enable_freeu(*FREEU)
    I2VGenXLPipeline().disable_freeu()
    with torch.device("meta"):
        unet = I2VGenXLUNet(I2VGenXLUNetConfig.mini())
    with pytest.raises(ValueError, match="finite"):
        unet.enable_freeu(float("nan"), 0.2, 1.2, 1.4)
    pipe = I2VGenXLPipeline(unet=unet)
    unet.frame_parallel = object()
    with pytest.raises(NotImplementedError, match="frame-parallel"):
        pipe.enable_freeu(*FREEU)
    with pytest.raises(NotImplementedError, match="frame-parallel"):
        unet.enable_freeu(*FREEU)
    unet.frame_parallel = None
    pipe.enable_freeu(*FREEU)
    assert unet.freeu == FREEU
    with pytest.raises(NotImplementedError, match="FreeU"):
        unet.set_frame_parallel(object())
    pipe.disable_freeu()
    assert unet.freeu is None


def test_engine_cache_key_and_source_cache_follow_the_freeu_parameters(cpu_ops):
    """The four numbers are part of the step engines' cache key (a graph captured under another setting is never replayed), and
    enabling / disabling drops the multi-edit source-feature cache."""
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMScheduler
    native, _, ocfg = gc.build_pair("mini", 1234)
    inp = gc.config1_inputs(ocfg, 2, 2, 8)
    g = lambda x: x.half()
    pipe = I2VGenXLPipeline(unet=native, scheduler=DDIMScheduler())

    def run():
        return pipe(prompt_embeds=g(inp["encoder_hidden_states"][1:2]), negative_prompt_embeds=g(inp["encoder_hidden_states"][:1]),
                    image_embeddings=g(inp["image_embeddings"][1:2]), image_latents=g(inp["image_latents"][1:2]), height=64, width=64,
                    num_frames=2, num_inference_steps=2, guidance_scale=9.0, target_fps=8, latents=g(inp["sample"][:1]),
                    output_type="latent", ddim_init_latents_t_idx=0).frames.clone()

    lat_off = run()
    (key_off,) = list(pipe._engines)
    pipe.enable_freeu(*FREEU)
    lat_on = run()
    (key_on,) = list(pipe._engines)   # same loop kind: the engine of the other setting is evicted, not kept
    assert key_off != key_on and key_off[-1] is None and key_on[-1] == FREEU
    assert not torch.equal(lat_on, lat_off)
    pipe.enable_freeu(0.9, 0.2, 1.2, 1.5)
    run()
    assert list(pipe._engines)[0][-1] == (0.9, 0.2, 1.2, 1.5)
    pipe.disable_freeu()
    assert torch.equal(run(), lat_off)
    assert list(pipe._engines)[0] == key_off
    cache = pipe.enable_source_cache(True)
    cache.bind(("clip",))
    cache.store(981, (True,), {"site": torch.zeros(4)})
    pipe.enable_freeu(*FREEU)
    assert cache.steps == {} and cache.signature is None
    cache.bind(("clip",))
    cache.store(981, (True,), {"site": torch.zeros(4)})
    pipe.disable_freeu()
    assert cache.steps == {}


def test_abi_validation_without_gpu():
    """Host-side validation returns ANYV2V_EINVAL (-1) with a message before anything touches a device."""
    from anyv2v_amd import _lib
    lib = _lib.load()
    P = 4096   # any 16-byte-aligned non-null address: nothing is dereferenced before the checks
    good = dict(hidden=P, ld_h=64, hidden_out=2 * P, ld_ho=64, C_h=64, b=1.2, skip=3 * P, ld_s=64, skip_out=4 * P, ld_so=64, C_s=64, s=0.9,
                n_img=2, H=8, W=8)

    def call(**over):
        a = dict(good, **over)
        return lib.anyv2v_freeu_f16(a["hidden"], a["ld_h"], a["hidden_out"], a["ld_ho"], a["C_h"], a["b"], a["skip"], a["ld_s"],
                                    a["skip_out"], a["ld_so"], a["C_s"], a["s"], a["n_img"], a["H"], a["W"], None)

    for name in ("hidden", "hidden_out", "skip", "skip_out"):
        assert call(**{name: None}) == -1 and b"null pointer" in lib.anyv2v_last_error()
    for over in (dict(C_h=60), dict(C_s=12), dict(C_h=0), dict(C_s=-8)):
        assert call(**over) == -1 and b"multiples of 8" in lib.anyv2v_last_error(), over
    for name in ("ld_h", "ld_ho", "ld_s", "ld_so"):
        assert call(**{name: 56}) == -1 and b"leading dimension" in lib.anyv2v_last_error(), name
    for over in (dict(H=0), dict(W=0), dict(n_img=0), dict(H=-3)):
        assert call(**over) == -1 and b">= 1" in lib.anyv2v_last_error(), over
    for over in (dict(b=float("nan")), dict(b=float("inf")), dict(s=float("nan")), dict(s=-float("inf"))):
        assert call(**over) == -1 and b"finite" in lib.anyv2v_last_error(), over
    assert call(hidden=P + 2) == -1 and b"16-byte" in lib.anyv2v_last_error()
    assert call(ld_s=68) == -1 and b"16-byte" in lib.anyv2v_last_error()
    assert call(H=4000, W=200) == -1 and b"H + W" in lib.anyv2v_last_error()
    assert call(hidden_out=P) == -1 and b"out of place" in lib.anyv2v_last_error()


def test_header_binding_and_abi_version():
    """The new entry point is declared, bound and exported; the ABI version did not move (no structure changed)."""
    from anyv2v_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "anyv2v_hip.h")).read()
    assert re.search(r"\banyv2v_freeu_f16\s*\(", hdr)
    assert "anyv2v_freeu_f16" in _lib.SYMBOLS and len(_lib.SYMBOLS["anyv2v_freeu_f16"][1]) == 16
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "anyv2v_freeu_f16")
    assert _lib.ABI_VERSION == 105 and "#define ANYV2V_ABI_VERSION 105" in hdr
