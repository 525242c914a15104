"""TEST-ONLY restatement of the detail-preserving restore of ``include/anyv2v_hip.h`` (``anyv2v_detail_gate_u8``,
``anyv2v_restore_detail_u8``) in plain numpy, on top of ``resample_spec.resize``, ``restore_spec.paste_byte`` and
``restore_spec.pillow_box``: the gate as the window sum it is defined as (not the separable form the kernels use), the paste one formula
line per line of the header; and the operand sets the CPU and the GPU tests share, on the shapes of ``restore_spec.CASES``.  Random bytes
alone close the gate everywhere, so three structured sets stand beside them.  Never importable from the product."""
from __future__ import annotations

import functools

import numpy as np

import resample_spec as spec
import restore_spec as rs

RADII = (0, 1, 2, 16)                       # at 16 the window is wider than the 16 x 16 frames: every clamp fires
THRESHOLDS = ((0, 1), (8, 32), (254, 255))
SETS = ("equal", "ramp", "clamp")


def gate(E, P, lo=8, hi=32, radius=2):
    """``E``, ``P`` uint8 [h, w, 3] -> ``G`` uint8 [h, w]."""
    c = np.abs(E.astype(np.int64) - P.astype(np.int64)).max(axis=2)
    h, w = c.shape
    ys, xs = np.clip(np.arange(-radius, h + radius), 0, h - 1), np.clip(np.arange(-radius, w + radius), 0, w - 1)
    padded = c[np.ix_(ys, xs)]                                                       # replicate edge
    b = sum(padded[dy:dy + h, dx:dx + w] for dy in range(2 * radius + 1) for dx in range(2 * radius + 1))
    n = (2 * radius + 1) ** 2
    mean = (b + n // 2) // n
    ramp = (255 * (hi - mean) + (hi - lo) // 2) // (hi - lo)
    return np.where(mean <= lo, 255, np.where(mean >= hi, 0, ramp)).astype(np.uint8)


def terms(S, E, P, G, dest, box, name, A=None):
    """The operands of the paste inside dest, int64: ``(d, e, p, g, m)``, ``g`` and ``m`` [dh, dw, 1]."""
    dx0, dy0, dx1, dy1 = dest
    dsize, pbox = (dx1 - dx0, dy1 - dy0), rs.pillow_box(box)
    e = spec.resize(E, dsize, name, box=pbox).astype(np.int64)
    p = spec.resize(P, dsize, name, box=pbox).astype(np.int64)
    g = spec.resize(G, dsize, "bilinear", box=pbox).astype(np.int64)[:, :, None]
    m = np.full(g.shape, 255, dtype=np.int64) if A is None else spec.resize(A, dsize, "bilinear", box=pbox).astype(np.int64)[:, :, None]
    return S[dy0:dy1, dx0:dx1].astype(np.int64), e, p, g, m


def restore_detail(S, E, P, G, dest, box, name, A=None):
    """``S`` uint8 [sh, sw, 3], ``E`` / ``P`` uint8 [h, w, 3], ``G`` uint8 [h, w], ``A`` uint8 [h, w] or None -> uint8 [sh, sw, 3]."""
    dx0, dy0, dx1, dy1 = dest
    d, e, p, g, m = terms(S, E, P, G, dest, box, name, A)
    wt = g + (g >> 7)
    add = ((d - p) * wt + 128) >> 8                                                  # (numpy's >> of a signed integer is arithmetic)
    e2 = np.clip(e + add, 0, 255)
    out = np.array(S, dtype=np.uint8, copy=True)
    out[dy0:dy1, dx0:dx1] = rs.paste_byte(d, e2, m).astype(np.uint8)
    return out


# ------------------------------------------------------------------------------------------------ the shared operands
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays if len(arrays) > 1 else arrays[0]


@functools.lru_cache(maxsize=None)
def prepared(case, F=2):
    """Random bytes for ``P`` beside ``restore_spec.operands(case)``: uint8 [F, h, w, 3], read-only."""
    _, (w, h), _, _ = rs.CASES[case]
    return _frozen(np.random.default_rng(2000 + sorted(rs.CASES).index(case)).integers(0, 256, (F, h, w, 3), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def random_gate(case, frames=2):
    _, (w, h), _, _ = rs.CASES[case]
    return _frozen(np.random.default_rng(3000 + frames + sorted(rs.CASES).index(case)).integers(0, 256, (frames, h, w), dtype=np.uint8))


@functools.lru_cache(maxsize=None)
def structured(case, kind, F=2):
    """``(E, P)`` uint8 [F, h, w, 3], read-only, beside the source of ``restore_spec.operands(case)``:
    equal  E == P (random bytes): the gate is 255 everywhere
    ramp   E = P +- {0 .. 3} on the left, unrelated bytes in the right quarter, and between them columns whose difference grows by 3 a column,
           so that the box means pass through the ramp's interior
    clamp  P in runs of 0 and 255 (4 pixels each, along the rows), E random: under an open gate ``e + add`` leaves [0, 255] at both ends"""
    _, (w, h), _, _ = rs.CASES[case]
    rng = np.random.default_rng(4000 + SETS.index(kind) + 10 * sorted(rs.CASES).index(case))
    P = rng.integers(0, 256, (F, h, w, 3), dtype=np.uint8)
    if kind == "equal":
        E = P.copy()
    elif kind == "ramp":
        P = rng.integers(64, 192, (F, h, w, 3), dtype=np.uint8)
        step = np.clip((np.arange(w) - w // 8) * 3, 0, 48)                             # 0 on the left, growing by 3 a column from there
        delta = rng.integers(-3, 4, (F, h, w, 3)) + step[None, None, :, None] * rng.choice((-1, 1), (F, h, w, 1))
        E = np.clip(P.astype(np.int64) + delta, 0, 255).astype(np.uint8)
        E[:, :, w - w // 4:] = rng.integers(0, 256, (F, h, w // 4, 3), dtype=np.uint8)
    else:
        P = np.broadcast_to((((np.arange(w) // 4) & 1) * 255).astype(np.uint8)[None, None, :, None], (F, h, w, 3)).copy()
        P[1:] = 255 - P[1:]
        E = rng.integers(0, 256, (F, h, w, 3), dtype=np.uint8)
    return _frozen(E, P)


@functools.lru_cache(maxsize=None)
def expected_gate(case, kind, lo=8, hi=32, radius=2, F=2):
    E, P = structured(case, kind, F)
    return _frozen(np.stack([gate(E[f], P[f], lo, hi, radius) for f in range(F)]))


@functools.lru_cache(maxsize=None)
def expected(case, name="lanczos", alpha_kind=None, alpha_frames=1, gate_frames=2, F=2):
    """The definition's result for random operands under a random gate: uint8 [F, sh, sw, 3], read-only, computed once."""
    _, (w, h), dest, box = rs.CASES[case]
    S, E = rs.operands(case, F)
    P, G = prepared(case, F), random_gate(case, gate_frames)
    A = None if alpha_kind is None else rs.alpha(alpha_kind, h, w, alpha_frames)
    return _frozen(np.stack([restore_detail(S[f], E[f], P[f], G[f % gate_frames], dest, box, name, None if A is None else A[f % alpha_frames])
                             for f in range(F)]))
