"""Host plan of the tiled AutoencoderKL encode / decode (``enable_vae_tiling``; diffusers-0.26.3 ``tiled_encode`` / ``tiled_decode`` /
``blend_v`` / ``blend_h``, DESIGN.md "VAE tiling").  Pure Python + CPU torch: nothing here touches the GPU.

The definition blends tiles in place, in row-major order: tile (i, j) first with the tile above it (``blend_v``), then with the tile on
its left (``blend_h``), each neighbour ALREADY blended, and keeps ``tile[:limit, :limit]``.  With ``stride >= 2 e`` the rows / columns
a blend reads from a neighbour lie outside that neighbour's own blend bands, so the recursion closes after one step per axis and
every output element is a fixed combination of at most four RAW tiles:

    out[y, x] = wy wx R[py, px] + wy (1 - wx) L[py, qx] + (1 - wy) wx^2 U[qy, px] + (1 - wy) (1 - wx^2) UL[qy, qx]

R / L / U / UL = tiles (ky, kx), (ky, kx - 1), (ky - 1, kx), (ky - 1, kx - 1).  Per axis an output coordinate o lies in tile k at local
position p; inside the blend band (k > 0, p < e' = min(size[k - 1], size[k], e)) it is blended with position q = size[k - 1] - e' + p of
tile k - 1 with weight w = p / e', outside it w = 1.  The weights are NOT the separable bilinear ones: U enters through the tile above,
which has itself been blended with UL over the same columns, hence wx^2.
"""
from __future__ import annotations

from typing import List, Tuple

import torch


def tile_grid(size: int, T: int, stride: int) -> List[Tuple[int, int]]:
    """(start, extent) of every tile along one axis: ``range(0, size, stride)``, edge tiles simply smaller."""
    if size < 1 or T < 1 or stride < 1:
        raise ValueError(f"tile_grid: size = {size}, T = {T}, stride = {stride} must all be >= 1")
    return [(s, min(T, size - s)) for s in range(0, size, stride)]


class AxisPlan:
    """One axis: the tile grid in the INPUT domain (``starts``, ``in_sizes``), the tiles' extents in the OUTPUT domain
    (``sizes`` = in_size * num // den: x8 for a decode, /8 for an encode) and, per output coordinate, ``tile`` k, ``pos`` p, ``prev``
    q (0 outside a blend band) and ``weight`` w (a Python float, ``p / e'``; 1.0 outside a band)."""

    def __init__(self, size: int, T: int, stride: int, e: int, limit: int, num: int = 1, den: int = 1):
        grid = tile_grid(size, T, stride)
        self.starts, self.in_sizes = [g[0] for g in grid], [g[1] for g in grid]
        self.sizes = [s * num // den for s in self.in_sizes]
        self.out_size = size * num // den
        if e < 0 or limit < 1 or min(self.sizes) < 1:
            raise ValueError(f"tiling: e = {e}, limit = {limit}, output tile extents {self.sizes}")
        self.tile, self.pos, self.prev, self.weight = [], [], [], []
        ext_prev = 0   # blend band of the previous tile (what a blend with it must not read)
        for k, n in enumerate(self.sizes):
            ext = min(self.sizes[k - 1], n, e) if k > 0 else 0
            if ext > 0 and self.sizes[k - 1] - ext < ext_prev:
                # the band of tile k would read blended rows of tile k - 1: a chain of more than two tiles per axis (needs stride < 2 e)
                raise ValueError(f"tiling: overlap {e} too large for stride {stride} (tile extents {self.sizes}): blend bands chain")
            for p in range(min(limit, n)):
                band = p < ext
                self.tile.append(k)
                self.pos.append(p)
                self.prev.append(self.sizes[k - 1] - ext + p if band else 0)
                self.weight.append(p / ext if band else 1.0)
            ext_prev = ext
        if len(self.tile) < self.out_size:
            raise ValueError(f"tiling: the kept parts cover {len(self.tile)} of {self.out_size} output positions (limit {limit}, "
                             f"tile extents {self.sizes})")
        for lst in (self.tile, self.pos, self.prev, self.weight):   # the final crop to the true size
            del lst[self.out_size:]

    @property
    def n_tiles(self):
        return len(self.sizes)


class StitchPlan:
    """Both axes of one stitch, and the tables ``ops.tile_blend`` hands to ``anyv2v_tile_blend_f16``."""

    def __init__(self, ay: AxisPlan, ax: AxisPlan):
        self.ay, self.ax = ay, ax
        self.H, self.W = ay.out_size, ax.out_size
        self._tables = {}

    def terms(self, dtype=torch.float64):
        """The gather plan itself, for checking: a list of four ``(dty, dtx, rows, cols, weight [H, W])`` -- the term reads raw tile
        ``(ky - dty, kx - dtx)`` at ``(rows[y], cols[x])`` (index tensors [H] / [W]).  A zero weight means the term is not read."""
        wy = torch.tensor(self.ay.weight, dtype=dtype)[:, None]
        wx = torch.tensor(self.ax.weight, dtype=dtype)[None, :]
        py, qy = torch.tensor(self.ay.pos), torch.tensor(self.ay.prev)
        px, qx = torch.tensor(self.ax.pos), torch.tensor(self.ax.prev)
        return [(0, 0, py, px, wy * wx), (0, 1, py, qx, wy * (1 - wx)), (1, 0, qy, px, (1 - wy) * (wx * wx)),
                (1, 1, qy, qx, (1 - wy) * (1 - wx * wx))]

    def tables(self, bases: List[List[int]], device):
        """(plan_host int32, weight_host fp64, plan_dev, weight_dev): tile records {first row of image 0, height, width, 0} in
        row-major tile order, then the row and the column table.  ``bases[ty][tx]``: first row of tile (ty, tx) of image 0 in the tile
        matrix.  Cached per (bases, device)."""
        key = (tuple(tuple(r) for r in bases), str(device))
        hit = self._tables.get(key)
        if hit is None:
            rec = [[bases[ty][tx], self.ay.sizes[ty], self.ax.sizes[tx], 0] for ty in range(self.ay.n_tiles)
                   for tx in range(self.ax.n_tiles)]
            flat = [v for r in rec for v in r]
            for a in (self.ay, self.ax):
                for k, p, q in zip(a.tile, a.pos, a.prev):
                    flat += [k, p, q]
            plan = torch.tensor(flat, dtype=torch.int32)
            weight = torch.tensor(self.ay.weight + self.ax.weight, dtype=torch.float64)
            hit = self._tables[key] = (plan, weight, plan.to(device), weight.to(device))
        return hit


class TilingParams:
    """The constants of the definition for one AutoencoderKL config: ``T_s = sample_size`` pixels, ``T_l = int(T_s / 2 ** (levels - 1))``
    latents, overlap factor 0.25."""
    OVERLAP = 0.25

    def __init__(self, sample_size: int, levels: int):
        self.scale = 2 ** (levels - 1)
        self.T_s = int(sample_size)
        self.T_l = int(self.T_s / self.scale)
        if self.T_l < 1:
            raise ValueError(f"tiling: sample_size = {sample_size} is smaller than the VAE's down-sampling factor {self.scale}")
        f = self.OVERLAP
        # decode: latent tiles, blended in pixels;  encode: pixel tiles, blended in latents
        self.dec = dict(T=self.T_l, stride=int(self.T_l * (1 - f)), e=int(self.T_s * f), limit=self.T_s - int(self.T_s * f),
                        num=self.scale, den=1)
        self.enc = dict(T=self.T_s, stride=int(self.T_s * (1 - f)), e=int(self.T_l * f), limit=self.T_l - int(self.T_l * f),
                        num=1, den=self.scale)

    def decode_plan(self, h: int, w: int) -> StitchPlan:
        return StitchPlan(AxisPlan(h, **self.dec), AxisPlan(w, **self.dec))

    def encode_plan(self, H: int, W: int) -> StitchPlan:
        if H % self.scale or W % self.scale or self.enc["stride"] % self.scale:
            raise ValueError(f"tiled encode: {H} x {W} pixels and the tile stride {self.enc['stride']} must be multiples of {self.scale}")
        return StitchPlan(AxisPlan(H, **self.enc), AxisPlan(W, **self.enc))
