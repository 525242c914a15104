"""TEST-ONLY restatement of the tiled AutoencoderKL encode / decode (``enable_vae_tiling``) -- a helper, not a test file.

diffusers-0.26.3 ``AutoencoderKL.tiled_encode`` / ``tiled_decode`` / ``blend_v`` / ``blend_h``, literally: the sequential algorithm with
IN-PLACE blends in row-major tile order, in torch, in the dtype of the tiles (use fp64 for a reference).  Parameterised by the per-tile
function, so it runs on random tiles, on the native VAE or on ``oracle/vae_oracle.py``'s modules.  This file is the yardstick of the
host plan (``anyv2v_amd/vae_tiling.py``) and of the stitch kernel (``anyv2v_tile_blend_f16``).

    T_s = sample_size, T_l = int(T_s / 2 ** (len(block_out_channels) - 1)), f = 0.25
    decode: tiles of T_l latents every int(T_l (1 - f)); blend extent e = int(T_s f) pixels, keep limit = T_s - e pixels
    encode: tiles of T_s pixels every int(T_s (1 - f));  blend extent e = int(T_l f) latents, keep limit = T_l - e latents
"""
from __future__ import annotations

import numpy as np
import torch


# the stitch cases the host and the GPU tests share: (name, plan parameters, (H, W) in the INPUT domain); num / den: output per input size
DEC = dict(T=8, stride=6, e=2, limit=6, num=1, den=1)
ENC = dict(T=32, stride=24, e=1, limit=3, num=1, den=8)     # 32 px -> 4 latents, e = 1
CASES = [("8x8 (one tile)", DEC, (8, 8)), ("9x8", DEC, (9, 8)), ("14x20", DEC, (14, 20)), ("13x31", DEC, (13, 31)),
         ("26x7 (H over one tile, W not)", DEC, (26, 7)), ("8x19 (last tile narrower than e)", DEC, (8, 19)),
         ("25x37 (both last tiles 1 wide)", DEC, (25, 37)),
         ("encode 80x56 px", ENC, (80, 56)), ("encode 32x200 px", ENC, (32, 200)), ("encode 104x40 px", ENC, (104, 40)),
         ("e = 3 (not a power of two)", dict(T=12, stride=9, e=3, limit=9, num=1, den=1), (30, 23)),
         ("mini decode 40x28 latents -> 80x56 px", dict(T=16, stride=12, e=8, limit=24, num=2, den=1), (40, 28))]


def blend_v(a: torch.Tensor, b: torch.Tensor, e: int) -> torch.Tensor:
    e = min(a.shape[-2], b.shape[-2], e)
    for y in range(e):
        b[..., y, :] = a[..., a.shape[-2] - e + y, :] * (1 - y / e) + b[..., y, :] * (y / e)
    return b


def blend_h(a: torch.Tensor, b: torch.Tensor, e: int) -> torch.Tensor:
    e = min(a.shape[-1], b.shape[-1], e)
    for x in range(e):
        b[..., :, x] = a[..., :, a.shape[-1] - e + x] * (1 - x / e) + b[..., :, x] * (x / e)
    return b


def raw_tiles(x: torch.Tensor, tile_fn, T: int, stride: int):
    """``tile_fn`` on every crop ``x[..., i:i+T, j:j+T]``, i and j over ``range(0, size, stride)``: a list of rows of tiles."""
    H, W = x.shape[-2:]
    return [[tile_fn(x[..., i:i + T, j:j + T]) for j in range(0, W, stride)] for i in range(0, H, stride)]


def stitch(rows, e: int, limit: int, crop=None) -> torch.Tensor:
    """Blend the raw tiles ``rows[i][j]`` ([..., h, w] each) in place (on clones), in row-major order, keep [:limit, :limit] of each and
    concatenate; ``crop`` = (H, W): the true output size."""
    rows = [[t.clone() for t in row] for row in rows]
    result_rows = []
    for i, row in enumerate(rows):
        result_row = []
        for j, tile in enumerate(row):
            if i > 0:
                tile = blend_v(rows[i - 1][j], tile, e)
            if j > 0:
                tile = blend_h(row[j - 1], tile, e)
            result_row.append(tile[..., :limit, :limit])
        result_rows.append(torch.cat(result_row, dim=-1))
    out = torch.cat(result_rows, dim=-2)
    return out if crop is None else out[..., :crop[0], :crop[1]]


def params(sample_size: int, levels: int):
    """(decode, encode) keyword dicts T / stride / e / limit of the definition for a VAE with ``levels`` resolution levels."""
    T_s, f = sample_size, 0.25
    T_l = int(T_s / 2 ** (levels - 1))
    dec = dict(T=T_l, stride=int(T_l * (1 - f)), e=int(T_s * f), limit=T_s - int(T_s * f))
    enc = dict(T=T_s, stride=int(T_s * (1 - f)), e=int(T_l * f), limit=T_l - int(T_l * f))
    return dec, enc


def tiled(x: torch.Tensor, tile_fn, T: int, stride: int, e: int, limit: int, crop=None, dtype=torch.float64) -> torch.Tensor:
    """The whole definition: raw tiles of ``tile_fn`` (converted to ``dtype``), stitched."""
    rows = [[t.to(dtype) for t in row] for row in raw_tiles(x, tile_fn, T, stride)]
    return stitch(rows, e, limit, crop)


def to_fp16(x: torch.Tensor) -> torch.Tensor:
    """fp64 / fp32 -> fp16 with ONE rounding (numpy converts directly; torch's CPU cast goes through fp32 and rounds twice)."""
    return torch.from_numpy(x.detach().cpu().numpy().astype(np.float16))


def fp16_ulp(x: torch.Tensor) -> torch.Tensor:
    """Spacing of fp16 at |x| (fp64 in, fp64 out): 2^(floor(log2 |x|) - 10), at least the subnormal spacing 2^-24."""
    ex = torch.floor(torch.log2(x.abs().double().clamp_min(2.0 ** -24)))
    return torch.pow(2.0, (ex - 10).clamp_min(-24.0))
