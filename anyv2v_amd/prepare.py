"""Source clips of any size: cover-resize and crop, or plain resize, to the working size on the GPU -- the native counterpart of the
reference's top-level ``prepare_video.py`` (``crop_and_resize_video``).  The resize is Pillow's ``Image.resize`` byte for byte
(``ops.resample_u8``; the definition is in ``include/anyv2v_hip.h``), so a prepared frame equals
``img.resize(resize_to, LANCZOS).crop(window)`` and an edit mask drawn on a source-size frame lands on the same pixels.

``fit_geometry`` is the reference's arithmetic; ``prepare_frames`` / ``prepare_mask`` run it (``I2VGenXLPipeline`` has them as methods on
its own device); ``restore_geometry`` is its inverse and ``restore_frames`` the way back to the source's own size, Pillow's
``paste(resize(.., box), xy, mask)`` byte for byte (``ops.restore_u8``); ``plan_from_config`` is the only reader of the OPTIONAL keys
``source_fit`` / ``source_x_offset`` / ``source_y_offset`` / ``source_resample`` / ``source_size`` / ``source_restore`` /
``source_restore_resample`` / ``source_restore_detail`` (with ``_lo`` / ``_hi`` / ``_radius``), which the reference's files do not have:
absent, nothing here runs.  ``restore_frames_detail`` is ``restore_frames`` with the source's fine detail carried into the upscaled edit
where the edit left the content alone (``ops.detail_gate_u8``, ``ops.restore_detail_u8``)."""
from __future__ import annotations

import os
from dataclasses import dataclass
from typing import Optional

import numpy as np
import torch
from PIL import Image

from . import _lib, ops

FITS = ("crop", "stretch")


def _offset(name, v):
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not -1.0 <= float(v) <= 1.0:   # (also refuses NaN)
        raise ValueError(f"{name}={v!r}: a number, -1 <= {name} <= 1")
    return float(v)


def _size(name, v):
    try:
        w, h = v
        ok = not isinstance(w, bool) and not isinstance(h, bool) and int(w) == w and int(h) == h and 1 <= w <= _lib.RESAMPLE_MAX_SIDE \
            and 1 <= h <= _lib.RESAMPLE_MAX_SIDE
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{name}={v!r}: (width, height), two integers in 1 .. {_lib.RESAMPLE_MAX_SIDE}")
    return int(w), int(h)


def fit_geometry(src_size, size, fit, x_offset=0.0, y_offset=0.0):
    """Source ``(sw, sh)`` and target ``(w, h)`` -> ``(resize_to, window)``: the size the whole frame is resized to and the rectangle
    ``(x, y, w, h)`` of it that is kept.  ``fit="crop"`` is ``prepare_video.py:50-77`` with ``center_crop``: the frame is scaled until it
    covers the target (``scale = min(sw / w, sh / h)``, ``new = int(side / scale)``) and the window sits at
    ``clamp(int((offset + 1) / 2 * (new - target)), 0, new - target)``: offsets -1 / 0 / 1 are left or top / centre / right or bottom.
    ``fit="stretch"`` is its plain resize (``:78-80``).  (``longest_to_width`` crops outside the resized frame and is not offered.  Where
    the quotient ``side / scale`` falls just below the target in floating point, the side is the target: the reference's crop would leave
    the frame.)"""
    sw, sh = _size("src_size", src_size)
    w, h = _size("size", size)
    if fit not in FITS:
        raise ValueError(f"fit={fit!r}: one of {FITS}")
    x_offset, y_offset = _offset("x_offset", x_offset), _offset("y_offset", y_offset)
    if fit == "stretch":
        return (w, h), (0, 0, w, h)
    scale = min(sw / w, sh / h)
    new_w, new_h = max(int(sw / scale), w), max(int(sh / scale), h)
    off_x = max(0, min(new_w - w, int(((x_offset + 1) / 2) * (new_w - w))))
    off_y = max(0, min(new_h - h, int(((y_offset + 1) / 2) * (new_h - h))))
    return (new_w, new_h), (off_x, off_y, w, h)


def restore_geometry(src_size, size, fit, x_offset=0.0, y_offset=0.0):
    """The inverse of ``fit_geometry``: source ``(sw, sh)`` and working size ``(w, h)`` -> ``(dest, box)``.  The window ``(ox, oy, w, h)``
    of the frame resized to ``(nw, nh)`` covers the real rectangle ``[ox sw / nw, (ox + w) sw / nw] x [oy sh / nh, (oy + h) sh / nh]`` of the
    source.  ``dest = (dx0, dy0, dx1, dy1)`` is the largest integer rectangle inside it (``ceil`` / ``floor`` in exact integer arithmetic)
    and ``box = (dx0 nw / sw - ox, ..)``, doubles clamped to ``[0, w] x [0, h]``, is its pre-image in the edited clip's coordinates: with them
    ``E.resize((dx1 - dx0, dy1 - dy0), resample, box=box)`` samples the edited frame where ``prepare_frames`` sampled the source, and source
    pixels that lie only partly inside the footprint stay the source's.  ``fit="stretch"``: the whole frame and ``(0, 0, w, h)``.  An empty
    ``dest`` (a tiny source blown up to the working size) is a ``ValueError``."""
    (nw, nh), (ox, oy, w, h) = fit_geometry(src_size, size, fit, x_offset, y_offset)
    sw, sh = (int(v) for v in src_size)
    dx0, dx1 = -((-ox * sw) // nw), min(((ox + w) * sw) // nw, sw)
    dy0, dy1 = -((-oy * sh) // nh), min(((oy + h) * sh) // nh, sh)
    if dx1 <= dx0 or dy1 <= dy0:
        raise ValueError(f"restore_geometry: no whole pixel of the {sw} x {sh} source lies inside the window {w} x {h} at ({ox}, {oy}) of the "
                         f"frame resized to {nw} x {nh}")
    back = lambda d, n, s, o, hi: min(max((d * n - o * s) / s, 0.0), float(hi))   # (the numerator is an exact integer: one rounding)
    return (dx0, dy0, dx1, dy1), (back(dx0, nw, sw, ox, w), back(dy0, nh, sh, oy, h), back(dx1, nw, sw, ox, w), back(dy1, nh, sh, oy, h))


def _frames_tensor(frames, device, what="prepare_frames"):
    """A list of PIL images of one size, or a uint8 [F, H, W, 3] tensor -> contiguous uint8 [F, H, W, 3] on ``device``."""
    if isinstance(frames, torch.Tensor):
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
            raise ValueError(f"{what}: a uint8 [F, H, W, 3] tensor expected, got {tuple(frames.shape)} {frames.dtype}")
        return frames.to(device).contiguous()
    frames = list(frames)
    if not frames or not all(isinstance(f, Image.Image) for f in frames):
        raise ValueError(f"{what}: a non-empty list of PIL images or a uint8 [F, H, W, 3] tensor expected")
    sizes = {f.size for f in frames}
    if len(sizes) != 1:
        raise ValueError(f"{what}: the frames have unequal sizes {sorted(sizes)}")
    return torch.from_numpy(np.stack([np.asarray(f.convert("RGB"), dtype=np.uint8) for f in frames])).to(device)


def prepare_frames(frames, height, width, fit="crop", x_offset=0.0, y_offset=0.0, resample="lanczos", device="cuda"):
    """Frames of any one size -> uint8 [F, height, width, 3] on ``device``, per frame equal to
    ``img.resize(resize_to, resample).crop(window)`` of ``fit_geometry`` byte for byte; only the window is computed."""
    x = _frames_tensor(frames, device)
    resize_to, (wx, wy, ww, wh) = fit_geometry((x.shape[2], x.shape[1]), (width, height), fit, x_offset, y_offset)
    return ops.resample_u8(x, resize_to, resample, window=(wx, wy, ww, wh))


def prepare_mask(mask, height, width, fit="crop", x_offset=0.0, y_offset=0.0, device="cuda"):
    """An edit mask at the source's size, [1 or F, H, W] (uint8 0 / 255, or bool) -> uint8 [1 or F, height, width] of 0 / 255 as
    ``load_edit_mask`` returns it, through the geometry of ``prepare_frames``: resampled as one band with ``bilinear``, then set where the
    result is at least 128."""
    if not isinstance(mask, torch.Tensor) or mask.dtype not in (torch.uint8, torch.bool) or mask.dim() != 3 or mask.shape[0] < 1:
        got = f"{tuple(mask.shape)} {mask.dtype}" if isinstance(mask, torch.Tensor) else type(mask).__name__
        raise ValueError(f"prepare_mask: a uint8 (0 / 255) or bool [1 or F, H, W] tensor expected, got {got}")
    x = mask.to(device)
    x = (x.to(torch.uint8) * 255 if x.dtype == torch.bool else x)[..., None].contiguous()
    resize_to, window = fit_geometry((x.shape[2], x.shape[1]), (width, height), fit, x_offset, y_offset)
    out = ops.resample_u8(x, resize_to, "bilinear", window=window)[..., 0]
    return (out >= 128).to(torch.uint8) * 255


def restore_frames(edited, source_frames, fit="crop", x_offset=0.0, y_offset=0.0, resample="lanczos", alpha=None, device="cuda"):
    """The way back: ``edited`` (uint8 [F, h, w, 3] or F PIL images at the working size) resized into the footprint it was prepared from
    and pasted over ``source_frames`` (at the source's own size, any) -> uint8 [F, sh, sw, 3] on ``device``, per frame Pillow's
    ``S.paste(E.resize(dsize, resample, box), (dx0, dy0), mask=A.resize(dsize, BILINEAR, box))`` of ``restore_geometry`` byte for byte
    (``ops.restore_u8``).  ``alpha``: None (the whole footprint is replaced) or fp32 [1 or F, h, w] in [0, 1], converted once by
    ``rint(255 alpha)``: where it is 0 the result holds the source's bytes, where it is 1 the upscaled edit's."""
    e = _frames_tensor(edited, device, "restore_frames: edited")
    s = _frames_tensor(source_frames, device, "restore_frames: source_frames")
    F, h, w, _ = (int(v) for v in e.shape)
    if s.shape[0] != F:
        raise ValueError(f"restore_frames: {F} edited frames against {s.shape[0]} source frames")
    dest, box = restore_geometry((int(s.shape[2]), int(s.shape[1])), (w, h), fit, x_offset, y_offset)
    return ops.restore_u8(e, s, dest, box, resample, _alpha_u8(alpha, F, h, w, device, "restore_frames"))


def _alpha_u8(alpha, F, h, w, device, what):
    """The alpha of the way back: None, or fp32 [1 or F, h, w] in [0, 1] -> uint8 on ``device`` by ``rint(255 alpha)``."""
    if alpha is None:
        return None
    if not isinstance(alpha, torch.Tensor) or not alpha.is_floating_point() or alpha.dim() != 3 or alpha.shape[0] not in (1, F) \
            or tuple(alpha.shape[1:]) != (h, w):
        got = f"{tuple(alpha.shape)} {alpha.dtype}" if isinstance(alpha, torch.Tensor) else type(alpha).__name__
        raise ValueError(f"{what}: alpha: a float [1 or {F}, {h}, {w}] tensor expected, got {got}")
    a = alpha.to(device=device, dtype=torch.float32)
    if not bool(((a >= 0.0) & (a <= 1.0)).all()):   # (false for NaN)
        raise ValueError(f"{what}: alpha must lie in [0, 1]")
    return torch.round(a * 255.0).to(torch.uint8).contiguous()


def restore_frames_detail(edited, source_frames, prepared=None, fit="crop", x_offset=0.0, y_offset=0.0, resample="lanczos", alpha=None,
                          source_resample="lanczos", gate_lo=8, gate_hi=32, gate_radius=2, device="cuda"):
    """``restore_frames`` that gives the source's fine detail back: with ``P`` the prepared source (the frames the model saw), ``S - up(P)``
    is the detail the trip down and up destroys, and it is added to the upscaled edit wherever the edit stayed close to ``P``
    (``ops.detail_gate_u8``: the mean over a ``(2 gate_radius + 1)^2`` box of ``max_c |E - P|``, full at ``gate_lo`` and below, none at
    ``gate_hi`` and above), so that old texture does not ghost into new content.  An edit that changes nothing restores the source byte
    for byte.  ``prepared``: uint8 [F, h, w, 3] or F PIL images of the edit's size, or None: the source is prepared on the spot with
    ``source_resample``.  Everything else as in ``restore_frames`` -> uint8 [F, sh, sw, 3] on ``device``."""
    what = "restore_frames_detail"
    e = _frames_tensor(edited, device, f"{what}: edited")
    s = _frames_tensor(source_frames, device, f"{what}: source_frames")
    F, h, w, _ = (int(v) for v in e.shape)
    if s.shape[0] != F:
        raise ValueError(f"{what}: {F} edited frames against {s.shape[0]} source frames")
    lo, hi, radius = ops.detail_parameters(gate_lo, gate_hi, gate_radius, f"{what}: gate: ")
    if prepared is None:
        p = prepare_frames(s, h, w, fit, x_offset, y_offset, source_resample, device=device)
    else:
        p = _frames_tensor(prepared, device, f"{what}: prepared")
        if p.shape != e.shape:
            raise ValueError(f"{what}: prepared frames of {tuple(p.shape)} against edited frames of {tuple(e.shape)}: the same clip at the same "
                             "working size expected")
    dest, box = restore_geometry((int(s.shape[2]), int(s.shape[1])), (w, h), fit, x_offset, y_offset)
    a = _alpha_u8(alpha, F, h, w, device, what)
    return ops.restore_detail_u8(e, p, ops.detail_gate_u8(e, p, lo, hi, radius), s, dest, box, resample, a)


# ------------------------------------------------------------------------------------------------ the configuration keys
@dataclass(frozen=True)
class PreparePlan:
    """What the ``source_*`` keys of one configuration ask for, resolved and checked once (``plan_from_config``).  ``source_size``:
    ``(w, h)`` the clip is prepared to where the configuration has no ``image_size`` of its own (``api``'s ``inverse_config``), else None."""
    fit: str
    x_offset: float = 0.0
    y_offset: float = 0.0
    resample: str = "lanczos"
    source_size: Optional[tuple] = None
    restore: bool = False               # ``source_restore``: the result goes back to the source clip's own size (``restored``)
    restore_resample: str = "lanczos"
    restore_detail: bool = False        # ``source_restore_detail``: the way back carries the source's fine detail (``restore_frames_detail``)
    detail_lo: int = 8
    detail_hi: int = 32
    detail_radius: int = 2

    def frames(self, pipe, frames, image_size):
        """PIL frames of any one size -> (uint8 [F, h, w, 3] on the pipeline's device, the same as PIL images)."""
        w, h = image_size
        out = pipe.prepare_frames(frames, h, w, fit=self.fit, x_offset=self.x_offset, y_offset=self.y_offset, resample=self.resample)
        return out, [Image.fromarray(f) for f in out.cpu().numpy()]

    def mask(self, pipe, mask, image_size):
        w, h = image_size
        return pipe.prepare_mask(mask, h, w, fit=self.fit, x_offset=self.x_offset, y_offset=self.y_offset).cpu()

    def restored(self, pipe, edited_u8, source_frames, alpha=None, prepared_from=None, prepared=None):
        """The frames that would be written (uint8 [F, h, w, 3] or PIL images at the working size) back over the source clip at its own
        size -> PIL images of the source's size (``pipe.restore_frames`` with this plan's geometry).  ``prepared_from``: the ``(w, h)``
        the clip was prepared from; source frames of another size are refused (the geometry would point elsewhere).  ``prepared``: the
        frames the inversion saw, looked at only with ``source_restore_detail`` (``pipe.restore_frames_detail``; None: prepared again)."""
        if prepared_from is not None:
            sizes = {tuple(f.size) for f in source_frames} if not isinstance(source_frames, torch.Tensor) else \
                {(int(source_frames.shape[2]), int(source_frames.shape[1]))}
            if sizes != {tuple(prepared_from)}:
                raise ValueError(f"source_restore: source frames of {sorted(sizes)} against a clip prepared from {tuple(prepared_from)}")
        if self.restore_detail:
            out = pipe.restore_frames_detail(edited_u8, source_frames, prepared, fit=self.fit, x_offset=self.x_offset, y_offset=self.y_offset,
                                             resample=self.restore_resample, alpha=alpha, source_resample=self.resample,
                                             gate_lo=self.detail_lo, gate_hi=self.detail_hi, gate_radius=self.detail_radius)
        else:
            out = pipe.restore_frames(edited_u8, source_frames, fit=self.fit, x_offset=self.x_offset, y_offset=self.y_offset,
                                      resample=self.restore_resample, alpha=alpha)
        return [Image.fromarray(f) for f in out.cpu().numpy()]

    def tag(self):
        """What ``source_restore`` adds to the name of an output directory ("" when it is off)."""
        if not self.restore:
            return ""
        tag = "_restored" + ("" if self.restore_resample == "lanczos" else f"-{self.restore_resample}")
        if self.restore_detail:
            params = (self.detail_lo, self.detail_hi, self.detail_radius)
            tag += "_detail" + ("" if params == (8, 32, 2) else "-%d-%d-%d" % params)
        return tag


def plan_from_config(config, restore_config=None) -> Optional[PreparePlan]:
    """The ``PreparePlan`` of a configuration (template YAML merged with a JSON entry, ``api``'s ``inverse_config``, or any plain
    namespace), or None when it has no ``source_fit``: then nothing is prepared and every name, file and error is what it was before the
    keys existed.  A tuning key without ``source_fit`` has nothing to act on and is refused, not dropped.  ``source_restore`` (a bool)
    and ``source_restore_resample`` are read from ``restore_config`` where one is given (``api``'s ``pnp_config``), else from ``config``;
    so are ``source_restore_detail`` (a bool, valid only beside ``source_restore``) and its tuning keys ``source_restore_detail_lo`` /
    ``_hi`` / ``_radius`` (integers, 0 <= lo < hi <= 255, 0 <= radius <= 16; refused without the switch)."""
    opt = lambda key, c=config: c.get(key, None) if hasattr(c, "get") else getattr(c, key, None)
    ropt = lambda key: opt(key, config if restore_config is None else restore_config)
    fit = opt("source_fit")
    tuning = ("source_x_offset", "source_y_offset", "source_resample", "source_size")
    restore, restore_resample = ropt("source_restore"), ropt("source_restore_resample")
    if restore is not None and not isinstance(restore, bool):
        raise ValueError(f"source_restore={restore!r}: true or false")
    if restore_resample is not None and not restore:
        raise ValueError("source_restore_resample without source_restore: there is no way back to tune")
    if restore_resample is not None and restore_resample not in _lib.RESAMPLE_FILTERS:
        raise ValueError(f"source_restore_resample={restore_resample!r}: one of {sorted(_lib.RESAMPLE_FILTERS)}")
    detail = ropt("source_restore_detail")
    if detail is not None and not isinstance(detail, bool):
        raise ValueError(f"source_restore_detail={detail!r}: true or false")
    if detail and not restore:
        raise ValueError("source_restore_detail without source_restore: there is no way back to carry the detail on")
    params = {}
    for k, default in (("lo", 8), ("hi", 32), ("radius", 2)):
        v = ropt(f"source_restore_detail_{k}")
        if v is not None and not detail:
            raise ValueError(f"source_restore_detail_{k} without source_restore_detail: there is no gate to tune")
        if v is not None and (isinstance(v, bool) or not isinstance(v, int)):
            raise ValueError(f"source_restore_detail_{k}={v!r}: an integer")
        params[k] = default if v is None else v
    if detail:
        if not 0 <= params["lo"] < params["hi"] <= 255:
            raise ValueError(f"source_restore_detail_lo={params['lo']}, source_restore_detail_hi={params['hi']}: 0 <= lo < hi <= 255")
        if not 0 <= params["radius"] <= _lib.DETAIL_MAX_RADIUS:
            raise ValueError(f"source_restore_detail_radius={params['radius']}: 0 <= radius <= {_lib.DETAIL_MAX_RADIUS}")
    if fit is None:
        for k in tuning:
            if opt(k) is not None:
                raise ValueError(f"{k} without source_fit: there is no preparation to tune")
        if restore:
            raise ValueError("source_restore without source_fit: nothing was prepared, there is no size to go back to")
        return None
    if fit not in FITS:
        raise ValueError(f"source_fit={fit!r}: one of {FITS}")
    x, y, resample, size = (opt(k) for k in tuning)
    x = _offset("source_x_offset", 0.0 if x is None else x)
    y = _offset("source_y_offset", 0.0 if y is None else y)
    if fit == "stretch" and (x != 0.0 or y != 0.0):
        raise ValueError("source_x_offset / source_y_offset with source_fit=stretch: nothing is cropped")
    resample = "lanczos" if resample is None else resample
    if resample not in _lib.RESAMPLE_FILTERS:
        raise ValueError(f"source_resample={resample!r}: one of {sorted(_lib.RESAMPLE_FILTERS)}")
    if size is not None:
        size = _size("source_size", size)
        if size[0] % 8 or size[1] % 8:
            raise ValueError(f"source_size={list(size)}: width and height must be multiples of 8")
    return PreparePlan(fit, x, y, resample, size, bool(restore), "lanczos" if restore_resample is None else restore_resample, bool(detail),
                       params["lo"], params["hi"], params["radius"])


def load_source_frames(frames_path, n_frames):
    """``utils.load_video_frames`` without its size check: the first ``n_frames`` ``%05d.png`` files at their own size."""
    from .utils import load_image
    paths = [f"{frames_path}/%05d.png" % i for i in range(n_frames)]
    return paths, [load_image(p) for p in paths]


def load_source_clip(frames_path, video_path, n_frames):
    """The runners' source clip at its own size: the ``%05d.png`` directory, else the mp4 beside it (``anyv2v_amd.mp4``)."""
    try:
        return load_source_frames(frames_path, n_frames)[1]
    except Exception:
        from .mp4 import read_mp4
        return list(read_mp4(video_path)[0])[:n_frames]


def load_source_mask(mask_path, n_frames):
    """``utils.load_edit_mask`` without its size check -> uint8 [1 or n_frames, H, W] at the files' own (equal) size."""
    paths = [os.path.join(mask_path, "%05d.png" % i) for i in range(n_frames)] if os.path.isdir(mask_path) else [mask_path]
    planes = []
    for p in paths:
        if not os.path.isfile(p):
            raise ValueError(f"edit mask {p} not found")
        planes.append(torch.from_numpy(np.array(Image.open(p).convert("L"), dtype=np.uint8)))
    if len({tuple(p.shape) for p in planes}) != 1:
        raise ValueError(f"edit mask {mask_path}: the files have unequal sizes")
    return torch.stack(planes)


def save_frames(frames, out_dir):
    """PIL frames -> ``<out_dir>/%05d.png``."""
    os.makedirs(out_dir, exist_ok=True)
    for i, f in enumerate(frames):
        f.save(os.path.join(out_dir, f"{i:05d}.png"))

