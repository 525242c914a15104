"""Source clips of any size: cover-resize and crop, or plain resize, to the working size on the GPU -- the native counterpart of the
reference's top-level ``prepare_video.py`` (``crop_and_resize_video``).  The resize is Pillow's ``Image.resize`` byte for byte
(``ops.resample_u8``; the definition is in ``include/anyv2v_hip.h``), so a prepared frame equals
``img.resize(resize_to, LANCZOS).crop(window)`` and an edit mask drawn on a source-size frame lands on the same pixels.

``fit_geometry`` is the reference's arithmetic; ``prepare_frames`` / ``prepare_mask`` run it (``I2VGenXLPipeline`` has them as methods on
its own device); ``plan_from_config`` is the only reader of the OPTIONAL keys ``source_fit`` / ``source_x_offset`` / ``source_y_offset`` /
``source_resample`` / ``source_size``, which the reference's files do not have: absent, nothing here runs."""
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


def _frames_tensor(frames, device):
    """A list of PIL images of one size, or a uint8 [F, H, W, 3] tensor -> contiguous uint8 [F, H, W, 3] on ``device``."""
    if isinstance(frames, torch.Tensor):
        if frames.dtype != torch.uint8 or frames.dim() != 4 or frames.shape[3] != 3 or frames.shape[0] < 1:
            raise ValueError(f"prepare_frames: a uint8 [F, H, W, 3] tensor expected, got {tuple(frames.shape)} {frames.dtype}")
        return frames.to(device).contiguous()
    frames = list(frames)
    if not frames or not all(isinstance(f, Image.Image) for f in frames):
        raise ValueError("prepare_frames: a non-empty list of PIL images or a uint8 [F, H, W, 3] tensor expected")
    sizes = {f.size for f in frames}
    if len(sizes) != 1:
        raise ValueError(f"prepare_frames: the frames have unequal sizes {sorted(sizes)}")
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

    def frames(self, pipe, frames, image_size):
        """PIL frames of any one size -> (uint8 [F, h, w, 3] on the pipeline's device, the same as PIL images)."""
        w, h = image_size
        out = pipe.prepare_frames(frames, h, w, fit=self.fit, x_offset=self.x_offset, y_offset=self.y_offset, resample=self.resample)
        return out, [Image.fromarray(f) for f in out.cpu().numpy()]

    def mask(self, pipe, mask, image_size):
        w, h = image_size
        return pipe.prepare_mask(mask, h, w, fit=self.fit, x_offset=self.x_offset, y_offset=self.y_offset).cpu()


def plan_from_config(config) -> Optional[PreparePlan]:
    """The ``PreparePlan`` of a configuration (template YAML merged with a JSON entry, ``api``'s ``inverse_config``, or any plain
    namespace), or None when it has no ``source_fit``: then nothing is prepared and every name, file and error is what it was before the
    keys existed.  A tuning key without ``source_fit`` has nothing to act on and is refused, not dropped."""
    opt = lambda key: config.get(key, None) if hasattr(config, "get") else getattr(config, key, None)
    fit = opt("source_fit")
    tuning = ("source_x_offset", "source_y_offset", "source_resample", "source_size")
    if fit is None:
        for k in tuning:
            if opt(k) is not None:
                raise ValueError(f"{k} without source_fit: there is no preparation to tune")
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
    return PreparePlan(fit, x, y, resample, size)


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

