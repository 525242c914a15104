"""Tiled VAE encode / decode without a GPU: the closed-form gather plan (``anyv2v_amd/vae_tiling.py``) against the sequential definition
(``tests/vae_tiling_spec.py``) on random raw tiles in fp64, the tile grid, the C entry point's host-side table checks, and the pipeline
switches."""
import ctypes
import os
import re

import pytest
import torch

import vae_tiling_spec as spec
from vae_tiling_spec import CASES, DEC
from anyv2v_amd.vae_tiling import AxisPlan, StitchPlan, TilingParams, tile_grid

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

def random_tiles(plan: StitchPlan, lead=(2, 3), seed=0):
    g = torch.Generator().manual_seed(seed)
    return [[torch.randn(*lead, th, tw, generator=g, dtype=torch.float64) for tw in plan.ax.sizes] for th in plan.ay.sizes]


def evaluate_plan(plan: StitchPlan, tiles, dtype=torch.float64):
    """The gather plan, evaluated with torch: at most four (tile, y, x, weight) terms per output element."""
    ky, kx = torch.tensor(plan.ay.tile), torch.tensor(plan.ax.tile)
    lead = tiles[0][0].shape[:-2]
    out = torch.zeros(*lead, plan.H, plan.W, dtype=dtype)
    wsum = torch.zeros(plan.H, plan.W, dtype=dtype)
    nterms = torch.zeros(plan.H, plan.W, dtype=torch.int64)
    for dty, dtx, rows, cols, w in plan.terms(dtype):
        for ty in range(plan.ay.n_tiles):
            for tx in range(plan.ax.n_tiles):
                m = ((ky == ty)[:, None] & (kx == tx)[None, :]) & (w != 0)
                if not m.any():
                    continue
                assert ty - dty >= 0 and tx - dtx >= 0, "a term with weight reads a tile outside the grid"
                src = tiles[ty - dty][tx - dtx].to(dtype)
                yy, xx = m.nonzero(as_tuple=True)
                assert int(rows[yy].max()) < src.shape[-2] and int(cols[xx].max()) < src.shape[-1]
                out[..., yy, xx] += w[yy, xx] * src[..., rows[yy], cols[xx]]
                wsum[yy, xx] += w[yy, xx]
                nterms[yy, xx] += 1
    return out, wsum, nterms


@pytest.mark.parametrize("name,p,size", CASES, ids=[c[0] for c in CASES])
def test_plan_equals_the_sequential_definition_in_fp64(name, p, size):
    plan = StitchPlan(AxisPlan(size[0], **p), AxisPlan(size[1], **p))
    assert (plan.H, plan.W) == (size[0] * p["num"] // p["den"], size[1] * p["num"] // p["den"])
    tiles = random_tiles(plan, seed=size[0] * 100 + size[1])
    want = spec.stitch(tiles, p["e"], p["limit"], crop=(plan.H, plan.W))
    got, wsum, nterms = evaluate_plan(plan, tiles)
    assert got.shape == want.shape
    d = float((got - want).abs().max())
    print(f"[vae tiling] {name}: plan vs sequential definition max |diff| {d:.2e}, at most {int(nterms.max())} terms")
    assert d <= 1e-12
    assert float((wsum - 1).abs().max()) <= 1e-12          # every output element's weights sum to 1
    assert 1 <= int(nterms.min()) and int(nterms.max()) <= 4


@pytest.mark.parametrize("name,p,size", CASES, ids=[c[0] for c in CASES])
def test_tile_grid_is_the_range_enumeration(name, p, size):
    for dim in size:
        want = [(s, min(p["T"], dim - s)) for s in range(0, dim, p["stride"])]
        assert tile_grid(dim, p["T"], p["stride"]) == want
        a = AxisPlan(dim, **p)
        assert list(zip(a.starts, a.in_sizes)) == want
        assert a.sizes == [s * p["num"] // p["den"] for _, s in want]
    # the spec cuts the same crops
    x = torch.zeros(1, 1, *size)
    rows = spec.raw_tiles(x, lambda t: t, p["T"], p["stride"])
    assert [[tuple(t.shape[-2:]) for t in r] for r in rows] == [[(h, w) for _, w in tile_grid(size[1], p["T"], p["stride"])]
                                                                 for _, h in tile_grid(size[0], p["T"], p["stride"])]


def test_corner_is_not_the_separable_bilinear_weight():
    """Where both blends apply the tile above enters with wx^2, not wx: it was blended with ITS left neighbour before."""
    plan = StitchPlan(AxisPlan(14, **DEC), AxisPlan(14, **DEC))
    terms = {(a, b): w for a, b, _r, _c, w in plan.terms()}
    y = x = 7                                               # first kept row / column of tile 1 is 6 (w = 0); 7 has w = 1 / 2
    assert plan.ay.weight[y] == plan.ax.weight[x] == 0.5
    assert float(terms[(0, 0)][y, x]) == 0.25 and float(terms[(0, 1)][y, x]) == 0.25
    assert float(terms[(1, 0)][y, x]) == 0.125 and float(terms[(1, 1)][y, x]) == 0.375


def test_the_definition_constants():
    tp = TilingParams(512, 4)
    assert (tp.T_s, tp.T_l) == (512, 64)
    assert tp.dec == dict(T=64, stride=48, e=128, limit=384, num=8, den=1)
    assert tp.enc == dict(T=512, stride=384, e=16, limit=48, num=1, den=8)
    dec, enc = spec.params(512, 4)
    assert dec == {k: tp.dec[k] for k in dec} and enc == {k: tp.enc[k] for k in enc}
    plan = tp.decode_plan(88, 160)                          # 704 x 1280: 2 x 4 tiles of at most 512 x 512 pixels
    assert (plan.H, plan.W) == (704, 1280) and plan.ay.sizes == [512, 320] and plan.ax.sizes == [512, 512, 512, 128]
    plan = tp.encode_plan(704, 1280)
    assert (plan.H, plan.W) == (88, 160) and plan.ay.in_sizes == [512, 320] and plan.ax.in_sizes == [512, 512, 512, 128]
    mini = TilingParams(32, 2)
    assert mini.dec == dict(T=16, stride=12, e=8, limit=24, num=2, den=1)
    with pytest.raises(ValueError, match="chain"):
        AxisPlan(40, T=8, stride=3, e=4, limit=3)           # stride < 2 e: more than two tiles would meet in one band
    with pytest.raises(ValueError, match="multiples"):
        tp.encode_plan(700, 1280)


def test_tables_layout():
    plan = StitchPlan(AxisPlan(13, **DEC), AxisPlan(31, **DEC))
    bases = [[100 * ty + tx for tx in range(plan.ax.n_tiles)] for ty in range(plan.ay.n_tiles)]
    ph, wh, pd, wd = plan.tables(bases, "cpu")
    nt = plan.ay.n_tiles * plan.ax.n_tiles
    assert ph.dtype == torch.int32 and wh.dtype == torch.float64 and ph.numel() == 4 * nt + 3 * (13 + 31) and wh.numel() == 13 + 31
    rec = ph[:4 * nt].view(nt, 4)
    assert rec[:, 0].tolist() == [b for r in bases for b in r]
    assert rec[:, 1].tolist() == [h for h in plan.ay.sizes for _ in plan.ax.sizes]
    assert rec[:, 2].tolist() == [w for _ in plan.ay.sizes for w in plan.ax.sizes]
    assert ph[4 * nt:4 * nt + 39].view(13, 3)[:, 0].tolist() == plan.ay.tile
    assert plan.tables(bases, "cpu")[0] is ph               # cached


def test_entry_point_is_declared_bound_exported_and_checks_its_tables():
    """The C entry point validates the HOST copy of the tables before it launches: with bad tables it returns ANYV2V_EINVAL without
    touching the device pointers (fake, never dereferenced)."""
    from anyv2v_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "anyv2v_hip.h")).read()
    assert re.search(r"\banyv2v_tile_blend_f16\s*\(", hdr)
    assert "anyv2v_tile_blend_f16" in _lib.SYMBOLS and len(_lib.SYMBOLS["anyv2v_tile_blend_f16"][1]) == 15
    declared = set(re.findall(r"^(?:int|int64_t|const char\*)\s+(anyv2v_[a-z0-9_]+)\s*\(", hdr, flags=re.M))
    assert declared == set(_lib.SYMBOLS)
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "anyv2v_tile_blend_f16")
    lib = _lib.load()
    plan = StitchPlan(AxisPlan(13, **DEC), AxisPlan(31, **DEC))
    n_img, rows, bases = 2, 0, []
    for th in plan.ay.sizes:
        bases.append([])
        for tw in plan.ax.sizes:
            bases[-1].append(rows)
            rows += n_img * th * tw
    ph, wh, _pd, _wd = plan.tables(bases, "cpu")
    P = 4096                                                # fake, aligned device pointer: every call below fails before the launch

    def call(plan_t=ph, weight_t=wh, tile_rows=rows, ld=8, C=3, tiles=P, out=P, n=n_img, H=plan.H, W=plan.W):
        return lib.anyv2v_tile_blend_f16(tiles, tile_rows, ld, C, plan_t.data_ptr(), weight_t.data_ptr(), P, P, plan.ay.n_tiles,
                                         plan.ax.n_tiles, out, n, H, W, None)
    assert call(tile_rows=rows - 1) == -1 and b"leaves the" in lib.anyv2v_last_error()
    assert call(n=3) == -1 and b"leaves the" in lib.anyv2v_last_error()
    assert call(C=9) == -1 and call(C=0) == -1 and call(ld=12) == -1 and call(tiles=P + 8) == -1 and call(out=P + 1) == -1
    assert call(tile_rows=1 << 31) == -1
    nt = plan.ay.n_tiles * plan.ax.n_tiles
    for idx, val, msg in [(4 * nt + 3 * 12 + 1, 5, b"row-table"),           # pos past the 1-row last tile
                          (4 * nt + 0, 7, b"row-table"),                    # tile index out of range
                          (4 * nt + 3 * 13 + 3 * 6 + 2, 99, b"column-table"),   # prev position outside the left tile (x = 6 is in a band)
                          (4 * nt + 3 * 13 + 1, -1, b"column-table")]:
        bad = ph.clone()
        bad[idx] = val
        assert call(plan_t=bad) == -1 and msg in lib.anyv2v_last_error(), (idx, val, lib.anyv2v_last_error())
    badw = wh.clone()
    badw[0] = 0.5                                            # a blend weight in tile 0: there is no tile above
    assert call(weight_t=badw) == -1 and b"row-table" in lib.anyv2v_last_error()
    badw = wh.clone()
    badw[3] = float("nan")
    assert call(weight_t=badw) == -1


def test_pipeline_switch_reaches_the_native_vae_and_is_ignored_by_the_synthetic_one(caplog):
    from anyv2v_amd.encoders import NativeVAE, SyntheticVAE
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.vae import AutoencoderKL, VAEConfig
    assert VAEConfig().sample_size == 512 and VAEConfig(sample_size=256).sample_size == 256
    cfg = VAEConfig.mini()
    cfg.sample_size = 32
    vae = NativeVAE(cfg=cfg, random_init_seed=1)
    assert isinstance(vae.model, AutoencoderKL) and vae.model.use_tiling is False
    pipe = I2VGenXLPipeline(vae=vae)
    with caplog.at_level("WARNING"):
        pipe.enable_vae_tiling()
    assert vae.model.use_tiling is True and vae.use_tiling is True and "decoded whole" not in caplog.text
    pipe.disable_vae_tiling()
    assert vae.model.use_tiling is False
    vae.model.enable_tiling(False)
    assert vae.model.use_tiling is False
    # automatic: only a frame that exceeds a tile AND cannot run whole (more than 8192 latent tokens)
    pipe.auto_vae_tiling(512, 1024)
    assert vae.model.use_tiling is False
    pipe.auto_vae_tiling(704, 1280)
    assert vae.model.use_tiling is True
    # the selection rule of the model
    m = vae.model
    assert m._tiles_decode(torch.empty(1, 4, 17, 16)) and not m._tiles_decode(torch.empty(1, 4, 16, 16))
    assert m._tiles_encode(torch.empty(1, 3, 32, 33)) and not m._tiles_encode(torch.empty(1, 3, 32, 32))
    m.disable_tiling()
    assert not m._tiles_decode(torch.empty(1, 4, 17, 16)) and not m._tiles_encode(torch.empty(1, 3, 64, 64))
    # a VAE without tiling: accepted and ignored, as before
    syn = SyntheticVAE()
    pipe = I2VGenXLPipeline(vae=syn)
    with caplog.at_level("WARNING"):
        pipe.enable_vae_tiling()
    assert "decoded whole" in caplog.text and not hasattr(syn, "use_tiling")
    pipe.auto_vae_tiling(704, 1280)
    pipe.disable_vae_tiling()
    I2VGenXLPipeline().enable_vae_tiling()                  # no VAE loaded
    from anyv2v_amd.consisti2v_pipeline import ConditionalVideoEditingPipeline as CI2V
    assert callable(CI2V.enable_vae_tiling) and callable(CI2V.disable_vae_tiling)
