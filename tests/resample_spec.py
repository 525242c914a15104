"""TEST-ONLY restatement of the resampling definition of ``include/anyv2v_hip.h`` (Pillow's ``ImagingResample`` for 8-bit bands) and of
``anyv2v_amd.prepare.fit_geometry``, in plain Python: the tables in Python floats (IEEE double) one output at a time, the samples in int64
numpy one output column at a time.  ``tests/test_resample_host.py`` holds it against Pillow itself, byte for byte; the planner, the
emulation and the kernels are held against it.  Never importable from the product."""
from __future__ import annotations

import math

import numpy as np

PRECISION_BITS = 22


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


def _bicubic(x):
    a = -0.5
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


FILTERS = {"box": (0.5, _box), "bilinear": (1.0, _bilinear), "bicubic": (2.0, _bicubic), "lanczos": (3.0, _lanczos)}


def table(in_size, in0, in1, out_size, name):
    """-> (ksize, bounds [(xmin, n)] per output, coeffs [[k] * ksize] per output, zero past n)."""
    support, f = FILTERS[name]
    scale = (in1 - in0) / out_size
    fs = max(scale, 1.0)
    sup = support * fs
    ss = 1.0 / fs
    ksize = int(math.ceil(sup)) * 2 + 1
    bounds, coeffs = [], []
    for xx in range(out_size):
        center = in0 + (xx + 0.5) * scale
        xmin = max(int(center - sup + 0.5), 0)
        n = min(int(center + sup + 0.5), in_size) - xmin
        w = [f((x + xmin - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        k = [int(v * (1 << PRECISION_BITS) + 0.5) if v >= 0 else int(v * (1 << PRECISION_BITS) - 0.5) for v in w]
        bounds.append((xmin, n))
        coeffs.append(k + [0] * (ksize - n))
    return ksize, bounds, coeffs


def needs_pass(in_size, in0, in1, out_size):
    return out_size != in_size or in0 != 0 or in1 != in_size


def _one_pass(a, bounds, coeffs, stats):
    """a: int64 [N, in, C]; resamples axis 1 -> uint8 [N, out, C]."""
    out = np.empty((a.shape[0], len(bounds), a.shape[2]), dtype=np.uint8)
    for xx, ((xmin, n), k) in enumerate(zip(bounds, coeffs)):
        acc = (1 << (PRECISION_BITS - 1)) + (a[:, xmin:xmin + n, :] * np.asarray(k[:n], dtype=np.int64)[None, :, None]).sum(axis=1)
        assert abs(acc).max(initial=0) < (1 << 31)
        v = acc >> PRECISION_BITS
        if stats is not None:
            stats["clamped"] = stats.get("clamped", 0) + int(((v < 0) | (v > 255)).sum())
        out[:, xx, :] = np.clip(v, 0, 255)
    return out


def resize(a, size, name, box=None, window=None, stats=None):
    """``a``: uint8 [H, W] or [H, W, C] -> Pillow's ``Image.resize(size, name, box)``, or only the rectangle ``window = (wx, wy, ww, wh)`` of
    it, computed from the window's rows of the tables alone.  ``stats["clamped"]`` counts the samples that left [0, 255] before the clamp."""
    a = np.asarray(a)
    flat = a.ndim == 2
    if flat:
        a = a[:, :, None]
    H, W, _ = a.shape
    out_w, out_h = size
    x0, y0, x1, y1 = (0, 0, W, H) if box is None else box
    wx, wy, ww, wh = (0, 0, out_w, out_h) if window is None else window
    assert 0 <= wx and 0 <= wy and ww >= 1 and wh >= 1 and wx + ww <= out_w and wy + wh <= out_h
    row0, rows = wy, wh
    vb = vc = None
    if needs_pass(H, y0, y1, out_h):
        _, vb, vc = table(H, y0, y1, out_h, name)
        vb, vc = vb[wy:wy + wh], vc[wy:wy + wh]
        row0 = vb[0][0]
        rows = vb[-1][0] + vb[-1][1] - row0
        vb = [(xmin - row0, n) for xmin, n in vb]
    x = a[row0:row0 + rows]
    if needs_pass(W, x0, x1, out_w):
        _, hb, hc = table(W, x0, x1, out_w, name)
        x = _one_pass(x.astype(np.int64), hb[wx:wx + ww], hc[wx:wx + ww], stats)
    else:
        x = x[:, wx:wx + ww]
    if vb is not None:
        x = _one_pass(x.astype(np.int64).transpose(1, 0, 2), vb, vc, stats).transpose(1, 0, 2)
    x = np.ascontiguousarray(x)
    return x[:, :, 0] if flat else x


def fit_geometry(src_size, size, fit, x_offset=0.0, y_offset=0.0):
    """The reference's ``crop_and_resize_video`` arithmetic -> (resize_to, (x, y, w, h))."""
    (sw, sh), (w, h) = src_size, size
    if fit == "stretch":
        return (w, h), (0, 0, w, h)
    assert fit == "crop"
    scale = min(sw / w, sh / h)
    new_w, new_h = int(sw / scale), int(sh / scale)
    off_x = max(0, min(new_w - w, int(((x_offset + 1) / 2) * (new_w - w))))
    off_y = max(0, min(new_h - h, int(((y_offset + 1) / 2) * (new_h - h))))
    return (new_w, new_h), (off_x, off_y, w, h)
