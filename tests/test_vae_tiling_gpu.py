"""Tiled VAE encode / decode on the GPU: the stitch kernel (``anyv2v_tile_blend_f16``) against the sequential definition
(``tests/vae_tiling_spec.py``) evaluated in fp64, and ``AutoencoderKL.enable_tiling`` end to end.

Bounds.  Kernel: the four products and their sum are formed in fp64 (relative error <= 2^-50 of the largest term, far below half an fp16
subnormal step for fp16 data) and rounded to fp16 ONCE, so |got - exact| <= 1 fp16 ulp of the exact value -- and where the blend extent
e' is a power of two every product and the sum are exact in fp64 in the kernel and in the fp64 definition alike, so the result must EQUAL
the definition rounded once.  Model: the native tiled path and the definition driven by the native per-tile call stitch the same tiles
(one launch sequence per tile position either way), so they must be bit-equal; against the fp32 oracle the bounds are those of the
whole-frame parity rows of ``gpu_checks.check_vae`` (decode 7e-3, posterior mean 5e-3, log-variance 4e-3)."""
import pytest
import torch

import gpu_checks as gc
import vae_tiling_spec as spec
from vae_tiling_spec import CASES

pytestmark = pytest.mark.gpu

DEC_TOL, MEAN_TOL, LOGVAR_TOL = 7e-3, 5e-3, 4e-3   # gpu_checks.check_vae


def _fp16_tiles(plan, n_img, C, seed):
    """Random fp16 raw tiles [n_img, C, th, tw]: N(0, 1) with ~6 % values within 1 % of +-65504 / 4 and ~6 % subnormals."""
    g = torch.Generator().manual_seed(seed)
    rows = []
    for th in plan.ay.sizes:
        rows.append([])
        for tw in plan.ax.sizes:
            t = torch.randn(n_img, C, th, tw, generator=g)
            u = torch.rand(t.shape, generator=g)
            sign = torch.where(torch.rand(t.shape, generator=g) < 0.5, -1.0, 1.0)
            big = sign * (65504.0 / 4) * (1 - 0.01 * torch.rand(t.shape, generator=g))
            sub = sign * torch.randint(1, 1024, t.shape, generator=g).float() * 2.0 ** -24
            t = torch.where(u < 0.06, big, torch.where(u < 0.12, sub, t))
            rows[-1].append(t.half())
    return rows


@pytest.mark.parametrize("name,p,size", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("C", [3, 8])
def test_kernel_equals_the_definition(name, p, size, C):
    from anyv2v_amd import ops
    from anyv2v_amd.vae_tiling import AxisPlan, StitchPlan
    plan = StitchPlan(AxisPlan(size[0], **p), AxisPlan(size[1], **p))
    n_img = 2
    tiles = _fp16_tiles(plan, n_img, C, seed=size[0] * 1000 + size[1] * 10 + C)
    want = spec.stitch([[t.double() for t in r] for r in tiles], p["e"], p["limit"], crop=(plan.H, plan.W))
    # the tile matrix the encoder / decoder would have written: tile (ty, tx), image n at rows base + n th tw, channels-last, ld = 8;
    # the columns a 3-channel decode leaves unwritten hold NaN
    bases, rows = [], 0
    for th in plan.ay.sizes:
        bases.append([])
        for tw in plan.ax.sizes:
            bases[-1].append(rows)
            rows += n_img * th * tw
    raw = torch.full((rows, 8), float("nan"), dtype=torch.float16)
    for ty, r in enumerate(tiles):
        for tx, t in enumerate(r):
            m = t.shape[0] * t.shape[2] * t.shape[3]
            raw[bases[ty][tx]:bases[ty][tx] + m, :C] = t.permute(0, 2, 3, 1).reshape(m, C)
    # the output inside a frame of NaN bit patterns
    buf, view, frame = gc._framed(1, n_img * C * plan.H * plan.W, rows=1, cols=64)
    out = view[0].view(n_img, C, plan.H, plan.W)
    got = ops.tile_blend(raw.to(gc.DEV), C, plan, bases, n_img, out=out)
    torch.cuda.synchronize()
    assert gc._frame_intact(buf, frame), "a store outside the output"
    got = got.cpu()
    assert torch.isfinite(got.float()).all(), "an output element was not written (or a padding column was read)"
    err = (got.double() - want).abs()
    ulp = spec.fp16_ulp(want)
    worst = float((err / ulp).max())
    print(f"[vae tiling] kernel {name} C={C}: max error {worst:.3f} fp16 ulp of the exact value")
    assert bool((err <= ulp).all())
    e_used = {min(a.sizes[k - 1], a.sizes[k], p["e"]) for a in (plan.ay, plan.ax) for k in range(1, a.n_tiles)}
    if all(e & (e - 1) == 0 for e in e_used):               # every blend extent a power of two: exact arithmetic on both sides
        assert torch.equal(got, spec.to_fp16(want))


@pytest.fixture(scope="module")
def mini():
    """Mini VAE (two levels: 2 pixels per latent) with 32-pixel tiles, the oracle on the same fp16-rounded weights, 2 frames of
    80 x 56 pixels / 40 x 28 latents, and the tiled native results."""
    from anyv2v_amd.vae import AutoencoderKL, VAEConfig
    from oracle import vae_oracle as vo
    cfg = VAEConfig.mini()
    cfg.sample_size = 32
    sd = vo.random_state_dict(vo.VAEConfig.mini(), 11)
    vae = AutoencoderKL(cfg)
    vae.load_state_dict(sd)
    vae.to(gc.DEV)
    oracle = vo.AutoencoderKLOracle(vo.VAEConfig.mini())
    oracle.load_state_dict(sd)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 80, 56, generator=g).clamp(-1, 1).half().float()
    z = torch.randn(2, 4, 40, 28, generator=g).half().float()
    dec, enc = spec.params(32, 2)
    vae.enable_tiling()
    out = dict(vae=vae, oracle=oracle, x=x, z=z, dec=dec, enc=enc, tiled_decode=vae.decode(z.to(gc.DEV)).cpu(),
               tiled_raw=vae.raw_moments(x.to(gc.DEV)).cpu(), tiled_moments=[t.cpu() for t in vae.encode_moments(x.to(gc.DEV))])
    vae.disable_tiling()
    out["whole_decode"] = vae.decode(z.to(gc.DEV)).cpu()
    return out


def test_tiled_decode_is_the_definition_and_not_the_whole_frame_decode(mini):
    """Fails without the feature: ``enable_tiling`` must exist, change the 80 x 56 decode, and give exactly the definition."""
    vae = mini["vae"]
    assert not vae.use_tiling
    want = spec.tiled(mini["z"].to(gc.DEV), lambda zt: vae.decode(zt).cpu(), crop=(80, 56), **mini["dec"])
    got = mini["tiled_decode"]
    assert got.dtype == torch.float32 and tuple(got.shape) == (2, 3, 80, 56)
    assert torch.equal(got, spec.to_fp16(want).float())
    assert not torch.equal(got, mini["whole_decode"])
    assert torch.equal(vae.tiled_decode(mini["z"].to(gc.DEV)).cpu(), got)   # the explicit entry point, tiling flag off


def test_tiled_encode_moments_are_the_definition(mini):
    vae = mini["vae"]
    want = spec.tiled(mini["x"].to(gc.DEV), lambda xt: vae.raw_moments(xt).cpu(), crop=(40, 28), **mini["enc"])
    got = mini["tiled_raw"]
    assert tuple(got.shape) == (2, 8, 40, 28)
    assert torch.equal(got, spec.to_fp16(want).float())
    mean, logvar = mini["tiled_moments"]
    assert torch.equal(mean, got[:, :4]) and torch.equal(logvar, got[:, 4:].clamp(-30.0, 20.0))
    assert not torch.equal(vae.raw_moments(mini["x"].to(gc.DEV)).cpu(), got)   # whole-frame moments differ, by design


def test_tiled_paths_against_the_fp32_oracle(mini):
    oracle = mini["oracle"]
    with torch.no_grad():
        want = spec.tiled(mini["z"], oracle.decode, crop=(80, 56), **mini["dec"])
        wantm = spec.tiled(mini["x"], lambda xt: oracle.quant_conv(oracle.encoder(xt)), crop=(40, 28), **mini["enc"])
    rows = [gc._res("tiled decode vs the definition on the oracle", mini["tiled_decode"], want.float(), DEC_TOL),
            gc._res("tiled posterior mean vs the definition on the oracle", mini["tiled_moments"][0], wantm[:, :4].float(), MEAN_TOL),
            gc._res("tiled posterior log-variance vs the definition on the oracle", mini["tiled_moments"][1],
                    wantm[:, 4:].clamp(-30.0, 20.0).float(), LOGVAR_TOL)]
    for r in rows:
        print(f"[vae tiling] {r['name']}: err {r['err']:.3e} l2 {r['l2']:.3e} tol {r['tol']:.1e}")
    assert all(r["ok"] for r in rows), rows


def test_a_frame_of_at_most_one_tile_is_untouched_by_the_switch(mini):
    vae = mini["vae"]
    z = mini["z"][:, :, :16, :12].contiguous().to(gc.DEV)
    x = mini["x"][:, :, :32, :24].contiguous().to(gc.DEV)
    off = (vae.decode(z), *vae.encode_moments(x))
    vae.enable_tiling()
    try:
        on = (vae.decode(z), *vae.encode_moments(x))
    finally:
        vae.disable_tiling()
    assert all(torch.equal(a, b) for a, b in zip(off, on))


def test_the_default_704x1280_frame_encodes_and_decodes_in_eight_tiles():
    """Full-width VAE, random weights, ONE frame: 88 x 160 latents is 14080 tokens, over the 8192 the mid-block attention takes."""
    from anyv2v_amd.vae import AutoencoderKL, VAEConfig, init_random_weights_
    vae = init_random_weights_(AutoencoderKL(VAEConfig()), 3).to(gc.DEV)
    g = torch.Generator().manual_seed(9)
    z = torch.randn(1, 4, 88, 160, generator=g).half().float().to(gc.DEV)
    x = torch.randn(1, 3, 704, 1280, generator=g).clamp(-1, 1).half().float().to(gc.DEV)
    dec, _enc = spec.params(512, 4)
    calls = []

    def tile(zt):
        calls.append(tuple(zt.shape[-2:]))
        return vae.decode(zt).cpu()
    want = spec.tiled(z, tile, crop=(704, 1280), **dec)     # tiling off: every crop is at most one tile
    assert len(calls) == 8 and max(h * w for h, w in calls) == 64 * 64
    vae.enable_tiling()
    got = vae.decode(z).cpu()
    assert tuple(got.shape) == (1, 3, 704, 1280) and torch.isfinite(got).all()
    assert torch.equal(got, spec.to_fp16(want).float())
    mean, logvar = vae.encode_moments(x)
    assert tuple(mean.shape) == tuple(logvar.shape) == (1, 4, 88, 160)
    assert torch.isfinite(mean).all() and torch.isfinite(logvar).all()
