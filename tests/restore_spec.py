"""TEST-ONLY restatement of the restore definition of ``include/anyv2v_hip.h`` (``anyv2v_restore_paste_u8``) in plain numpy, beside
``resample_spec``: the tables walked one output at a time, then Pillow's 8-bit paste formula; Pillow's own
``S.paste(E.resize(dsize, filter, box), (dx0, dy0), mask=A.resize(dsize, BILINEAR, box))``; the geometry's invariants in exact fractions;
and the shapes the CPU and the GPU tests share.  Never importable from the product."""
from __future__ import annotations

import functools
from fractions import Fraction

import numpy as np
from PIL import Image

import resample_spec as spec

PIL_FILTER = {"box": Image.Resampling.BOX, "bilinear": Image.Resampling.BILINEAR, "bicubic": Image.Resampling.BICUBIC,
              "lanczos": Image.Resampling.LANCZOS}


def paste_byte(d, e, m):
    """Pillow's paste with an L mask for one 8-bit band (``ImagingPaste``: ``BLEND8``)."""
    t = d * (255 - m) + e * m + 128
    return ((t >> 8) + t) >> 8


def pillow_box(box):
    """``box`` the way Pillow's resize takes it: four C floats, and the width formed in float before it is divided in double
    (``ImagingResample(.., float box[4])``, ``precompute_coeffs(inSize, float in0, float in1, ..)``: ``(double)(in1 - in0) / outSize``)."""
    x0, y0, x1, y1 = (np.float32(v) for v in box)
    return float(x0), float(y0), float(x0) + float(np.float32(x1 - x0)), float(y0) + float(np.float32(y1 - y0))


def restore(S, E, dest, box, name, A=None):
    """``S`` uint8 [sh, sw, 3], ``E`` uint8 [h, w, 3], ``A`` uint8 [h, w] or None -> uint8 [sh, sw, 3]."""
    dx0, dy0, dx1, dy1 = dest
    dsize = (dx1 - dx0, dy1 - dy0)
    e = spec.resize(E, dsize, name, box=pillow_box(box)).astype(np.int64)
    m = np.full(e.shape[:2], 255, dtype=np.int64) if A is None else spec.resize(A, dsize, "bilinear", box=pillow_box(box)).astype(np.int64)
    out = np.array(S, dtype=np.uint8, copy=True)
    d = out[dy0:dy1, dx0:dx1].astype(np.int64)
    out[dy0:dy1, dx0:dx1] = paste_byte(d, e, m[:, :, None]).astype(np.uint8)
    return out


def pillow_restore(S, E, dest, box, name, A=None):
    """Pillow itself."""
    dx0, dy0, dx1, dy1 = dest
    dsize = (dx1 - dx0, dy1 - dy0)
    out = Image.fromarray(np.ascontiguousarray(S)).copy()
    e = Image.fromarray(np.ascontiguousarray(E)).resize(dsize, PIL_FILTER[name], box=box)
    if A is None:
        out.paste(e, (dx0, dy0))
    else:
        out.paste(e, (dx0, dy0), mask=Image.fromarray(np.ascontiguousarray(A), mode="L").resize(dsize, Image.Resampling.BILINEAR, box=box))
    return np.asarray(out)


def footprint(src_size, size, fit, x_offset, y_offset):
    """The window's footprint in source pixels as exact fractions (x0, y0, x1, y1), from the reference's arithmetic."""
    (sw, sh), (w, h) = src_size, size
    (nw, nh), (ox, oy, _, _) = spec.fit_geometry(src_size, size, fit, x_offset, y_offset)
    nw, nh = max(nw, w), max(nh, h)     # (``prepare.fit_geometry``'s guard where the quotient falls just below the target)
    return Fraction(ox * sw, nw), Fraction(oy * sh, nh), Fraction((ox + w) * sw, nw), Fraction((oy + h) * sh, nh)


# ------------------------------------------------------------------------------------------------ the shared cases
def geometry(src_size, size, fit, x_offset=0.0, y_offset=0.0):
    from anyv2v_amd.prepare import restore_geometry
    return restore_geometry(src_size, size, fit, x_offset, y_offset)


# name -> (source (sw, sh), edit (w, h), dest, box): through the geometry where a fit is named, direct otherwise
CASES = {
    "crop-left": ((53, 37), (16, 16)) + geometry((53, 37), (16, 16), "crop", -1, 0.37),       # dest touches the left edge
    "crop-right": ((53, 37), (16, 16)) + geometry((53, 37), (16, 16), "crop", 1, -1),         # dx0 = 15: starts at an odd byte
    "crop-tall": ((37, 53), (16, 16)) + geometry((37, 53), (16, 16), "crop", 0.37, 0.37),     # rows above and below dest
    "stretch": ((53, 37), (16, 16)) + geometry((53, 37), (16, 16), "stretch"),
    "up-3.75": ((67, 61), (16, 16), (5, 1, 65, 61), (0.0, 0.0, 16.0, 16.0)),                  # strictly inside on three sides
    "down": ((37, 29), (64, 64)) + geometry((37, 29), (64, 64), "stretch"),
    "identity": ((24, 16), (24, 16)) + geometry((24, 16), (24, 16), "crop"),                  # both passes skipped
    "one-wide": ((53, 37), (16, 16), (7, 3, 8, 30), (0.0, 0.0, 16.0, 16.0)),
    "one-high": ((53, 37), (16, 16), (2, 36, 51, 37), (0.25, 0.5, 15.75, 15.5)),
    "h-only": ((53, 16), (16, 16), (3, 0, 50, 16), (0.0, 0.0, 16.0, 16.0)),                   # the vertical pass skipped alone
    "v-only": ((16, 37), (16, 16), (0, 2, 16, 35), (0.0, 0.0, 16.0, 16.0)),                   # the horizontal pass skipped alone
}
FILTER_CASE = {"lanczos": "crop-right", "bicubic": "crop-left", "bilinear": "crop-tall", "box": "crop-right"}
ALPHAS = ("zero", "full", "random", "step")


@functools.lru_cache(maxsize=None)
def operands(case, F=2, seed=0):
    """Random bytes: (S uint8 [F, sh, sw, 3], E uint8 [F, h, w, 3]), read-only."""
    (sw, sh), (w, h), _, _ = CASES[case]
    rng = np.random.default_rng(1000 + seed + sorted(CASES).index(case))
    S, E = rng.integers(0, 256, (F, sh, sw, 3), dtype=np.uint8), rng.integers(0, 256, (F, h, w, 3), dtype=np.uint8)
    S.setflags(write=False)
    E.setflags(write=False)
    return S, E


@functools.lru_cache(maxsize=None)
def alpha(kind, h, w, frames=1):
    """uint8 [frames, h, w]: all 0, all 255, random bytes, or a 0 / 255 step down the middle column (the second frame's across the rows)."""
    if kind == "zero":
        a = np.zeros((frames, h, w), dtype=np.uint8)
    elif kind == "full":
        a = np.full((frames, h, w), 255, dtype=np.uint8)
    elif kind == "random":
        a = np.random.default_rng(7 + frames).integers(0, 256, (frames, h, w), dtype=np.uint8)
    else:
        a = np.zeros((frames, h, w), dtype=np.uint8)
        a[0, :, w // 2:] = 255
        a[1:, h // 2:, :] = 255
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def expected(case, name="lanczos", alpha_kind=None, alpha_frames=1, F=2):
    """Pillow's result for a shared case: uint8 [F, sh, sw, 3], read-only, computed once."""
    _, (w, h), dest, box = CASES[case]
    S, E = operands(case, F)
    A = None if alpha_kind is None else alpha(alpha_kind, h, w, alpha_frames)
    out = np.stack([pillow_restore(S[f], E[f], dest, box, name, None if A is None else A[f % alpha_frames]) for f in range(F)])
    out.setflags(write=False)
    return out
