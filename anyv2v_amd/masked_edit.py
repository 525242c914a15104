"""Masked PnP editing, host side, in one place ("Masked edit" .. "Mask tracking"): what the ``edit_mask_*`` configuration
keys mean (``plan_from_config`` -> ``MaskedEditPlan``), the pipeline methods that make, shape and apply a mask (``MaskedEditMixin``,
inherited by ``I2VGenXLPipeline``) and the three steps both runners take around ``sample_with_pnp`` (``make_edit_mask``, ``masked``,
``finish_frames``).  The kernels are ``csrc/mask.hip``, ``automask.hip``, ``composite.hip`` and ``track.hip`` behind ``ops``; the blend
itself runs inside the step engines of ``step_engine.py``."""
from __future__ import annotations

import contextlib
import copy
import math
import numbers
import os
from dataclasses import dataclass
from typing import Optional, Union

import torch
from PIL import Image

from . import _lib, ops, pnp_utils
from .schedulers import DDIMScheduler
from .utils import LatentTrajectory, capture_hip_graph, load_ddim_latents_at_t, release_graphs

FIRST_FRAME_MASK_DEFAULTS = dict(threshold=24, min_count=8)                  # ``first_frame_edit_mask``'s
TRACK_DEFAULTS = dict(radius=16, median=True)                                # ``propagate_edit_mask``'s
AUTO_MASK_DEFAULTS = dict(maps=10, strength=0.5, ratio=3.0, threshold=0.5)   # ``generate_edit_mask``'s (diffusers' generate_mask)
COMPOSITE_DEFAULTS = dict(grow_px=0, feather_px=0.0, match_color=False)      # ``composite_over_source``'s


def _int_in(name, v, lo, hi, unit=""):
    """``v`` as an int in [lo, hi]; ``hi`` None: any integer >= lo that a C int holds.  A bool, a fraction and NaN are refused."""
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not lo <= v <= (2 ** 31 - 1 if hi is None else hi) or int(v) != v:
        raise ValueError(f"{name}={v}: an integer" + (f" >= {lo}" if hi is None else f", {lo} <= {name} <= {hi}") + (f" {unit}" if unit else ""))
    return int(v)


def _float_in(name, v, lo, hi, unit=""):
    v = float(v)
    if not lo <= v <= hi:   # (also refuses NaN)
        raise ValueError(f"{name}={v}: {lo} <= {name} <= {hi}" + (f" {unit}" if unit else ""))
    return v


def _grow_feather(grow, feather, prefix="", unit=""):
    """The dilation (latent pixels) and the feather sigma of ``ops.latent_mask``, as a method argument or as a configuration key."""
    return (_int_in(prefix + "grow", grow, 0, _lib.MASK_MAX_GROW, unit),
            _float_in(prefix + "feather", feather, 0, _lib.MASK_MAX_RADIUS // 3, unit))


def edit_mask_timestep(timesteps, num_inference_steps: int, mask_encode_strength: float) -> int:
    """The timestep ``generate_edit_mask`` noises the source to, as diffusers' ``get_timesteps`` of the DiffEdit pipeline: with
    ``num_inference_steps`` set on the forward scheduler, ``init = min(int(steps * strength), steps)`` and ``t = timesteps[steps - init]``;
    a strength so small that ``init`` is 0 takes the last (least noisy) timestep."""
    steps = int(num_inference_steps)
    init = min(int(steps * float(mask_encode_strength)), steps)
    return int(timesteps[min(steps - init, steps - 1)])


# ------------------------------------------------------------------------------------------------ the configuration keys
@dataclass(frozen=True)
class MaskedEditPlan:
    """What the ``edit_mask_*`` keys of one PnP-edit configuration ask for, resolved and range-checked once (``plan_from_config``).
    ``source``: where the mask comes from -- "path" (``path``: one PNG or a directory of them), "auto" (``auto``: maps / strength / ratio /
    threshold of ``generate_edit_mask``) or "first_frame" (``first_frame``: threshold / min_count of ``first_frame_edit_mask``); the other
    two are None.  ``grow`` / ``feather`` shape the latent mask whatever its source.  ``track`` (radius / median of ``propagate_edit_mask``)
    and ``composite`` (grow_px / feather_px / match_color of ``composite_over_source``): None when off."""
    source: str
    path: Optional[str] = None
    grow: int = 0
    feather: float = 0.0
    auto: Optional[dict] = None
    first_frame: Optional[dict] = None
    track: Optional[dict] = None
    composite: Optional[dict] = None

    def tag(self) -> str:
        """The ``_mask-...`` part of an output directory's name: the source, then every parameter that is not its default, so that two
        entries that differ in a mask key alone do not overwrite each other."""
        tuned = lambda vals, defaults: "".join(f"_{k}{vals[k]}" for k in defaults if vals[k] != defaults[k])
        if self.source == "path":
            name = os.path.splitext(os.path.basename(os.path.normpath(self.path)))[0]
        else:
            name = "auto" + tuned(self.auto, AUTO_MASK_DEFAULTS) if self.source == "auto" else "ff" + tuned(self.first_frame, FIRST_FRAME_MASK_DEFAULTS)
        t, c = self.track, self.composite
        return ("_mask-" + name + ("" if t is None else "-track" + tuned(t, dict(radius=TRACK_DEFAULTS["radius"])) + ("" if t["median"] else "_nomedian"))
                + (f"_grow{self.grow}" if self.grow > 0 else "") + (f"_feather{self.feather}" if self.feather > 0 else "")
                + ("" if c is None else "_comp" + (f"_grow{c['grow_px']}" if c["grow_px"] > 0 else "")
                   + (f"_feather{c['feather_px']}" if c["feather_px"] > 0 else "") + ("_match" if c["match_color"] else "")))


def plan_from_config(config) -> Optional[MaskedEditPlan]:
    """The ``MaskedEditPlan`` of a PnP-edit configuration (template YAML merged with a JSON entry, a front-end's ``pnp_config``, or any
    plain namespace), or None when it names no mask: the only reader of the OPTIONAL ``edit_mask_*`` keys, which the reference's files do
    not have.  Absent, null or false means off, and an entry that names none runs and writes exactly what it did before the keys existed.
    A key that has nothing to act on (a tuning key without its switch, grow / feather / tracking / composite without a mask) is refused,
    not dropped.  ``config.masked_edit_options`` .. ``composite_options`` document the keys and return their parts of the plan."""
    opt = lambda key: config.get(key, None) if hasattr(config, "get") else getattr(config, key, None)
    value = lambda v, default: default if v is None else v

    def switch(key):
        v = opt(key)
        if v is not None and not isinstance(v, bool):
            raise ValueError(f"{key}={v!r}: true or false")
        return v

    def tuning(key, on, what, *keys):
        vals = [opt(k) for k in keys]
        for k, v in zip(keys, vals):
            if not on and v is not None:
                raise ValueError(f"{k} without {key}: there is no {what}")
        return vals

    # the one source of the mask
    path, auto_on, ff_on = opt("edit_mask_path"), switch("edit_mask_auto"), switch("edit_mask_first_frame")
    if path is not None and auto_on:
        raise ValueError("edit_mask_auto together with edit_mask_path: the mask is either generated or loaded")
    if path is not None and ff_on:
        raise ValueError("edit_mask_first_frame together with edit_mask_path: the mask is either derived from the first frames or loaded")
    if auto_on and ff_on:
        raise ValueError("edit_mask_first_frame together with edit_mask_auto: the mask is either derived from the first frames or generated")
    source = "path" if path is not None else "auto" if auto_on else "first_frame" if ff_on else None
    grow, feather = opt("edit_mask_grow"), opt("edit_mask_feather")
    if source is None and (grow is not None or feather is not None):
        raise ValueError("edit_mask_grow / edit_mask_feather without edit_mask_path: there is no mask to grow or feather")
    # its tuning and its shape (the automatic mask's tuning is checked before the shape, the first-frame mask's behind it)
    auto = first_frame = track = composite = None
    vals = tuning("edit_mask_auto", auto_on, "automatic mask to tune", *("edit_mask_auto_" + k for k in AUTO_MASK_DEFAULTS))
    if auto_on:
        maps, *num = (value(v, d) for v, d in zip(vals, AUTO_MASK_DEFAULTS.values()))
        strength, ratio, threshold = (float(v) for v in num)
        maps = _int_in("edit_mask_auto_maps", maps, 1, None)
        if not 0.0 < strength <= 1.0:   # (also refuses NaN)
            raise ValueError(f"edit_mask_auto_strength={strength}: 0 < edit_mask_auto_strength <= 1")
        if not (ratio > 0.0 and math.isfinite(ratio)):
            raise ValueError(f"edit_mask_auto_ratio={ratio}: finite and > 0")
        if not 0.0 < threshold < 1.0:
            raise ValueError(f"edit_mask_auto_threshold={threshold}: 0 < edit_mask_auto_threshold < 1")
        auto = dict(maps=maps, strength=strength, ratio=ratio, threshold=threshold)
    if source is not None:
        grow, feather = _grow_feather(value(grow, 0), value(feather, 0.0), prefix="edit_mask_")
    vals = tuning("edit_mask_first_frame", ff_on, "first-frame mask to tune", *("edit_mask_first_frame_" + k for k in FIRST_FRAME_MASK_DEFAULTS))
    if ff_on:
        first_frame = dict(threshold=_int_in("edit_mask_first_frame_threshold", value(vals[0], FIRST_FRAME_MASK_DEFAULTS["threshold"]), 0, 255),
                           min_count=_int_in("edit_mask_first_frame_min_count", value(vals[1], FIRST_FRAME_MASK_DEFAULTS["min_count"]), 1, 64))
    # tracking: it needs a one-frame mask (the runner refuses a directory of per-frame masks)
    track_on, median = switch("edit_mask_track"), switch("edit_mask_track_median")
    radius, median = tuning("edit_mask_track", track_on, "tracking to tune", "edit_mask_track_radius", "edit_mask_track_median")
    if track_on:
        if source == "auto":
            raise ValueError("edit_mask_track together with edit_mask_auto: the generated mask already has every frame")
        if source is None:
            raise ValueError("edit_mask_track without edit_mask_first_frame or edit_mask_path: there is no frame-0 mask to carry")
        track = dict(radius=_int_in("edit_mask_track_radius", value(radius, TRACK_DEFAULTS["radius"]), 0, _lib.TRACK_MAX_RADIUS),
                     median=value(median, TRACK_DEFAULTS["median"]))
    # the pixel-space composite
    comp_on, match = switch("edit_mask_composite"), switch("edit_mask_match_color")
    grow_px, feather_px, match = tuning("edit_mask_composite", comp_on, "composite to shape", "edit_mask_composite_grow",
                                        "edit_mask_composite_feather", "edit_mask_match_color")
    if comp_on:
        if source is None:
            raise ValueError("edit_mask_composite without edit_mask_path or edit_mask_auto: there is no mask to composite by")
        composite = dict(grow_px=_int_in("edit_mask_composite_grow", value(grow_px, COMPOSITE_DEFAULTS["grow_px"]), 0, _lib.COMPOSITE_MAX_GROW),
                         feather_px=_float_in("edit_mask_composite_feather", value(feather_px, COMPOSITE_DEFAULTS["feather_px"]), 0,
                                              _lib.COMPOSITE_MAX_RADIUS // 3), match_color=bool(match))
    return None if source is None else MaskedEditPlan(source, None if path is None else str(path), grow, feather, auto, first_frame, track, composite)


# ------------------------------------------------------------------------------------------------ the runners' three steps
def make_edit_mask(pipe, plan, *, loaded=None, generate=None, source_first_frame=None, edited_first_frame=None, source_frames=None):
    """The edit mask ``plan`` asks for: ``loaded`` (the mask read from ``plan.path``; a caller that loads no files has none),
    ``generate(plan.auto)`` (the caller's ``pipe.generate_edit_mask`` call, with its own conditioning, seeding and trajectory) or
    ``pipe.first_frame_edit_mask`` of the two first frames; then carried along ``source_frames`` when the plan tracks it (a loaded PNG:
    every non-black pixel is carried as "edit" -- a grey level has no position to follow)."""
    if plan.source == "path":
        mask = loaded
    elif plan.source == "auto":
        mask = generate(plan.auto)
    else:
        mask = pipe.first_frame_edit_mask(source_first_frame, edited_first_frame, **plan.first_frame)
    if plan.track is not None:
        mask = pipe.propagate_edit_mask(source_frames, mask, **plan.track)
    return mask


@contextlib.contextmanager
def masked(pipe, plan, mask, source_latents):
    """``sample_with_pnp`` inside this block keeps the source outside ``mask``; the setting is cleared behind it, also when the call raises:
    the mask belongs to the clip, not to the pipeline.  Without a plan: nothing."""
    if plan is not None:
        pipe.enable_masked_edit(mask, source_latents, grow=plan.grow, feather=plan.feather)   # (refuses a frame-parallel clip)
    try:
        yield
    finally:
        if plan is not None:
            pipe.disable_masked_edit()


def finish_frames(pipe, plan, video, source_frames, mask):
    """The decoded ``video`` composited over the source frames as PIL images -- outside the mask they carry the source frames' bytes, not
    ``decode(encode(source))``; inside, the bytes ``to_pil`` forms -- or None when the plan has no composite."""
    if plan is None or plan.composite is None:
        return None
    frames_u8 = pipe.composite_over_source(video, source_frames, mask, grow=plan.grow, feather=plan.feather, **plan.composite)
    return [Image.fromarray(fr) for fr in frames_u8.cpu().numpy()]


# ------------------------------------------------------------------------------------------------ the pipeline's methods
class MaskedEditMixin:
    """The masked-edit methods of ``I2VGenXLPipeline``.  Of the pipeline they use ``_execution_device``, ``vae_scale_factor``, ``unet``, the
    ``_masked_edit`` setting (``sample_with_pnp`` reads it) and, in ``generate_edit_mask``, the scheduler and the conditioning assembly."""

    def enable_masked_edit(self, mask, source_latents, grow: int = 0, feather: float = 0.0):
        """Local editing: ``sample_with_pnp`` keeps the source clip outside ``mask``, bit for bit.  After every DDIM update the edit latent
        is blended against the source at the same noise level -- the inversion trajectory's entry, after the last step ``source_latents``
        (``encode_vae_video`` of the source frames: the trajectory does not hold the clean latent) -- by ``ops.masked_blend`` inside the
        captured step ("Masked edit").  ``mask``: [Fm, H, W] or [H, W] at the PIXEL size of the call, Fm 1 (every frame) or
        the frame count; bool, uint8 (image scale: 255 = edit) or float in [0, 1]; 1 = edit, 0 = keep.  ``grow``: latent pixels (0 .. 8) the
        edit region is dilated by; ``feather``: sigma (0 .. 8 latent pixels) of the Gaussian that softens its border.  A property of the
        clip, not of the pipeline: set it per edit and clear it (``disable_masked_edit``) afterwards; ``__call__`` and ``invert`` refuse to
        run while it is set.  A setter, not a call argument: the reference's signatures have none."""
        if getattr(self.unet, "frame_parallel", None) is not None:
            raise NotImplementedError("masked edit on a frame-parallel clip: every rank would need its frames of the mask and of the partner latents")
        m = self._edit_mask_fp16(mask)
        if not torch.is_tensor(source_latents) or source_latents.dim() != 5 or source_latents.shape[0] != 1 or \
                source_latents.shape[1] != 4 or tuple(source_latents.shape[3:]) != (m.shape[1] // 8, m.shape[2] // 8) or \
                m.shape[0] not in (1, source_latents.shape[2]):
            raise ValueError("source_latents: [1, 4, F, h, w] expected for a mask of "
                             f"{tuple(m.shape)} (h = H / 8, w = W / 8, Fm = 1 or F), got "
                             f"{tuple(source_latents.shape) if torch.is_tensor(source_latents) else type(source_latents).__name__}")
        grow, feather = _grow_feather(grow, feather, unit="latent pixels")
        self._masked_edit = dict(mask=m, source_latents=source_latents, grow=grow, feather=feather)

    def _edit_mask_fp16(self, mask):
        """An edit mask as ``enable_masked_edit`` / ``composite_over_source`` take it -> contiguous fp16 [Fm, H, W] in [0, 1]."""
        if not torch.is_tensor(mask) or mask.dim() not in (2, 3):
            raise ValueError(f"edit mask: a [Fm, H, W] or [H, W] tensor expected, got {type(mask).__name__}"
                             + (f" of shape {tuple(mask.shape)}" if torch.is_tensor(mask) else ""))
        if mask.dtype == torch.bool:
            m = mask.to(torch.float16)
        elif mask.dtype == torch.uint8:
            m = (mask.float() / 255.0).to(torch.float16)
        elif mask.is_floating_point():
            m = mask.float()
            if not bool(((m >= 0.0) & (m <= 1.0)).all()):   # (false for NaN)
                raise ValueError("edit mask: float values must lie in [0, 1] (1 = edit, 0 = keep the source)")
            m = m.to(torch.float16)
        else:
            raise ValueError(f"edit mask: bool, uint8 or float expected, got {mask.dtype}")
        m = (m[None] if m.dim() == 2 else m).contiguous()
        if m.shape[1] % self.vae_scale_factor or m.shape[2] % self.vae_scale_factor or m.shape[0] < 1 or m.shape[1] < 8 or m.shape[2] < 8:
            raise ValueError(f"edit mask: H x W = {m.shape[1]} x {m.shape[2]} must be positive multiples of {self.vae_scale_factor}")
        return m

    def disable_masked_edit(self):
        self._masked_edit = None

    @torch.no_grad()
    def composite_over_source(self, video, source_frames, mask, grow: int = 0, feather: float = 0.0, grow_px: int = 0,
                              feather_px: float = 0.0, match_color: bool = False):
        """The pixel-space finish of a masked edit: ``video`` ([1, 3, F, H, W] in [-1, 1], what ``decode_latents`` returns) pasted over
        ``source_frames`` (a list of F PIL images of the video's size, or a uint8 [F, H, W, 3] tensor) -> uint8 [F, H, W, 3] on the video's
        device.  Outside the edit region the decode is ``decode(encode(source))``, not the source; here those pixels are the source's
        bytes, whatever the decode holds, and fully edited pixels are the bytes ``vae.to_pil`` forms from the video as an fp16 tensor (the
        native decode hands its fp16 values over in fp32, where ``to_pil``'s own arithmetic may land one level away; DESIGN.md 5, "Composite").
        ``mask`` / ``grow`` / ``feather``: exactly what ``enable_masked_edit`` was given -- the latent mask is rebuilt by
        ``ops.latent_mask`` and alpha follows the region the latent blend used (every latent cell with mask > 0).  ``grow_px`` (0 .. 64
        pixels) dilates that region, ``feather_px`` (sigma, 0 .. 16 pixels) lets alpha fall off outside it, ``match_color`` first carries
        the edit's per-channel mean and deviation over the kept region to the source's (one gain and bias per clip).  A method called
        behind the decode, not an argument of the sampling calls: the reference's signatures have none."""
        if getattr(self.unet, "frame_parallel", None) is not None:
            raise NotImplementedError("composite on a frame-parallel clip: the masked edit it finishes is refused there")
        if not torch.is_tensor(video) or video.dim() != 5 or video.shape[0] != 1 or video.shape[1] != 3 or not video.is_floating_point():
            raise ValueError("video: a float [1, 3, F, H, W] tensor expected (decode_latents), got "
                             f"{tuple(video.shape) if torch.is_tensor(video) else type(video).__name__}")
        F, H, W = (int(v) for v in video.shape[2:])
        m = self._edit_mask_fp16(mask)
        if tuple(m.shape[1:]) != (H, W) or m.shape[0] not in (1, F):
            raise ValueError(f"edit mask {tuple(m.shape)} does not match the video: [Fm, H, W] = [1 or {F}, {H}, {W}] expected")
        if isinstance(source_frames, (list, tuple)) and len(source_frames) > 0 and all(hasattr(f, "convert") for f in source_frames):
            sizes = {tuple(f.size) for f in source_frames}
            if sizes != {(W, H)}:
                raise ValueError(f"source_frames: images of {sorted(sizes)} against a video of {W} x {H} (nothing is resized here)")
        elif not torch.is_tensor(source_frames):
            raise ValueError(f"source_frames: a list of PIL images or a uint8 [F, H, W, 3] tensor expected, got {type(source_frames).__name__}")
        src = self._frames_u8("source_frames", source_frames)
        if tuple(src.shape) != (F, H, W, 3):
            raise ValueError(f"source_frames {tuple(src.shape)} do not match the video: [F, H, W, 3] = [{F}, {H}, {W}, 3] expected")
        grow, feather, grow_px, feather_px = self._alpha_arguments(grow, feather, grow_px, feather_px)
        if not isinstance(match_color, bool):
            raise ValueError(f"match_color={match_color!r}: True or False")
        device = video.device
        alpha = self._composite_alpha(m.to(device), grow, feather, grow_px, feather_px)
        return ops.composite(video.to(torch.float16).contiguous(), src.to(device).contiguous(), alpha, match_color)

    @staticmethod
    def _alpha_arguments(grow, feather, grow_px, feather_px):
        grow, feather = _grow_feather(grow, feather, unit="latent pixels")
        grow_px = _int_in("grow_px", grow_px, 0, _lib.COMPOSITE_MAX_GROW, "pixels")
        feather_px = _float_in("feather_px", feather_px, 0, _lib.COMPOSITE_MAX_RADIUS // 3, "pixels")
        return grow, feather, grow_px, feather_px

    @staticmethod
    def _composite_alpha(m, grow, feather, grow_px, feather_px):
        """``m``: fp16 [Fm, H, W] of ``_edit_mask_fp16`` on the device -> the alpha ``ops.composite`` takes (``ops.pixel_alpha``'s)."""
        return ops.pixel_alpha(ops.latent_mask(m, grow, feather), grow_px, feather_px)

    @torch.no_grad()
    def composite_alpha(self, mask, grow: int = 0, feather: float = 0.0, grow_px: int = 0, feather_px: float = 0.0):
        """The alpha ``composite_over_source`` builds from the same arguments, on its own: fp32 [Fm, H, W] in [0, 1] on this pipeline's
        device, Fm 1 or the mask's frame count (1 = the edit, 0 = the source).  ``restore_frames`` takes it to paste a composited edit over
        the source clip at its own size."""
        if getattr(self.unet, "frame_parallel", None) is not None:
            raise NotImplementedError("composite on a frame-parallel clip: the masked edit it finishes is refused there")
        m = self._edit_mask_fp16(mask)
        return self._composite_alpha(m.to(self._execution_device), *self._alpha_arguments(grow, feather, grow_px, feather_px)).float()

    @staticmethod
    def _frames_u8(name, frames):
        """A PIL image, a list of PIL images of one size, or a uint8 [H, W, 3] / [F, H, W, 3] tensor -> uint8 [F, H, W, 3] with H and W
        positive multiples of 8 (nothing is resized, nothing is quantised)."""
        if hasattr(frames, "convert"):
            frames = [frames]
        if torch.is_tensor(frames):
            if frames.dtype != torch.uint8:
                raise ValueError(f"{name}: a uint8 tensor expected, got {frames.dtype} (nothing is quantised here)")
            t = frames[None] if frames.dim() == 3 else frames
        elif isinstance(frames, (list, tuple)) and len(frames) > 0 and all(hasattr(f, "convert") for f in frames):
            import numpy as np
            sizes = {tuple(f.size) for f in frames}
            if len(sizes) != 1:
                raise ValueError(f"{name}: images of different sizes {sorted(sizes)} (nothing is resized here)")
            t = torch.from_numpy(np.stack([np.asarray(f.convert("RGB"), dtype=np.uint8) for f in frames]))
        else:
            raise ValueError(f"{name}: PIL images or a uint8 [F, H, W, 3] tensor expected, got {type(frames).__name__}")
        if t.dim() != 4 or t.shape[3] != 3 or t.shape[0] < 1 or t.shape[1] < 8 or t.shape[2] < 8 or t.shape[1] % 8 or t.shape[2] % 8:
            raise ValueError(f"{name}: uint8 [F, H, W, 3] with H and W positive multiples of 8 expected, got {tuple(t.shape)}")
        return t

    @torch.no_grad()
    def first_frame_edit_mask(self, source_first_frame, edited_first_frame, threshold: int = 24, min_count: int = 8):
        """The one edit mask an AnyV2V job has for free: where the edited first frame differs from the source's -> bool [1, H, W] on the
        execution device, constant on the 8 x 8 cells of the latent grid.  A pixel changed when ``max_c |edited - source| > threshold``
        (strict, on the uint8 values, 0 .. 255); a cell is set when at least ``min_count`` (1 .. 64) of its 64 pixels changed.  Both frames:
        a PIL image or a uint8 [H, W, 3] tensor of the same size, H and W multiples of 8.  Alone it is a static mask like a single PNG;
        ``propagate_edit_mask`` carries it through the clip.  The result goes to ``enable_masked_edit`` / ``composite_over_source``
        unchanged; ``edit_mask_grow`` remains the remedy for a border that is a cell too tight."""
        src, ed = self._frames_u8("source_first_frame", source_first_frame), self._frames_u8("edited_first_frame", edited_first_frame)
        if src.shape[0] != 1 or ed.shape[0] != 1:
            raise ValueError(f"first_frame_edit_mask: one frame each expected, got {src.shape[0]} and {ed.shape[0]}")
        if src.shape != ed.shape:
            raise ValueError(f"edited_first_frame {tuple(ed.shape[1:])} does not match source_first_frame {tuple(src.shape[1:])} "
                             "(nothing is resized here)")
        threshold, min_count = _int_in("threshold", threshold, 0, 255), _int_in("min_count", min_count, 1, 64)
        device = self._execution_device
        return ops.first_frame_mask(src[0].to(device).contiguous(), ed[0].to(device).contiguous(), threshold, min_count)

    @torch.no_grad()
    def propagate_edit_mask(self, source_frames, mask, radius: int = 16, median: bool = True, return_flow: bool = False):
        """Carry a frame-0 edit mask through the clip along the motion of the SOURCE frames -> bool [F, H, W] on the execution device
        (with ``return_flow`` also the int16 [F, H / 8, W / 8, 2] displacement field, (dy, dx) per frame and 8 x 8 cell).  Classical
        full-search block matching on the luma (``ops.block_match``: per cell the displacement in [-radius, radius]^2 of its 16 x 16
        window against the previous frame with the least sum of absolute differences; ties go to the shortest vector, so flat and
        periodic regions stay put), a 3 x 3 median over the cells (``median``), then ``mask_k[p] = mask_{k-1}[clamp(p + D_k[cell(p)])]``.
        All integers: bit-reproducible, no model involved, once per clip.  ``source_frames``: a list of F PIL images or a uint8
        [F, H, W, 3] tensor; ``mask``: [H, W] or [1, H, W], bool or uint8 (non-zero = edit); ``radius``: an integer 0 .. 32 pixels per
        frame.  Occlusions, sub-pixel motion and a coarse-to-fine search are outside the definition: motion beyond ``radius`` per frame is
        not followed, and ``grow`` of ``enable_masked_edit`` (``edit_mask_grow``) is the remedy for a border that drifts by a cell.  The
        result goes to ``enable_masked_edit`` / ``composite_over_source`` unchanged; no step engine, engine key or ``_masked_edit`` is
        touched here."""
        src = self._frames_u8("source_frames", source_frames)
        if not torch.is_tensor(mask) or mask.dim() not in (2, 3):
            raise ValueError(f"edit mask: a [H, W] or [1, H, W] tensor expected, got {type(mask).__name__}"
                             + (f" of shape {tuple(mask.shape)}" if torch.is_tensor(mask) else ""))
        if mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"edit mask: bool or uint8 expected (a soft mask has no position to carry), got {mask.dtype}")
        if mask.dim() == 3 and mask.shape[0] != 1:
            raise ValueError(f"edit mask {tuple(mask.shape)}: it already has {mask.shape[0]} frames; a frame-0 mask [H, W] or [1, H, W] expected")
        m0 = mask[0] if mask.dim() == 3 else mask
        if tuple(m0.shape) != tuple(src.shape[1:3]):
            raise ValueError(f"edit mask {tuple(m0.shape)} does not match the frames: [H, W] = {list(src.shape[1:3])} expected")
        radius = _int_in("radius", radius, 0, _lib.TRACK_MAX_RADIUS, "pixels")
        if not isinstance(median, bool):
            raise ValueError(f"median={median!r}: True or False")
        device = self._execution_device
        flow = ops.block_match(ops.luma_u8(src.to(device).contiguous()), radius)
        if median:
            flow = ops.flow_median(flow)
        tracked = ops.mask_propagate(m0.to(device).contiguous(), flow)
        return (tracked, flow) if return_flow else tracked

    def _refuse_masked_edit(self, what):
        """``__call__`` / ``invert``: no source branch, no trajectory to blend against -- a mask left set would be silently dropped."""
        if getattr(self, "_masked_edit", None) is not None:
            raise ValueError(f"an edit mask is set (enable_masked_edit): {what} has no source to keep -- only sample_with_pnp blends; call "
                             "disable_masked_edit() first")

    def _masked_edit_buffers(self, height, width, num_frames, latents):
        """-> (partner buffer, latent mask, clean source latent) for this ``sample_with_pnp`` call, or None without a mask.  The latent
        mask is built here, once per clip (three small launches outside any graph)."""
        me = getattr(self, "_masked_edit", None)
        if me is None:
            return None
        if getattr(self.unet, "frame_parallel", None) is not None:
            raise NotImplementedError("masked edit on a frame-parallel clip: every rank would need its frames of the mask and of the partner latents")
        m, src = me["mask"], me["source_latents"]
        if tuple(m.shape[1:]) != (height, width) or m.shape[0] not in (1, num_frames):
            raise ValueError(f"edit mask {tuple(m.shape)} does not match the call: [Fm, H, W] = [1 or {num_frames}, {height}, {width}] expected")
        if tuple(src.shape) != tuple(latents.shape):
            raise ValueError(f"source_latents {tuple(src.shape)} do not match the call's latents {tuple(latents.shape)}")
        device = latents.device
        lm = ops.latent_mask(m.to(device), me["grow"], me["feather"])
        return torch.zeros_like(latents), lm, src.to(device=device, dtype=torch.float16).contiguous()

    @torch.no_grad()
    def generate_edit_mask(self, prompt=None, image=None, ddim_inv_prompt=None, ddim_inv_1st_frame=None, source_latents=None,
                           ddim_inv_latents_path: Union[str, LatentTrajectory, None] = None, height: Optional[int] = 704,
                           width: Optional[int] = 1280, num_frames: int = 16, target_fps: Optional[int] = 16, num_inference_steps: int = 50,
                           num_maps_per_mask: int = 10, mask_encode_strength: float = 0.5, mask_thresholding_ratio: float = 3.0,
                           threshold: float = 0.5, generator=None, clip_skip: Optional[int] = 1, trace: Optional[dict] = None,
                           prompt_embeds=None, image_embeddings=None, image_latents=None, ddim_inv_prompt_embeds=None,
                           ddim_inv_image_embeddings=None, ddim_inv_image_latents=None):
        """The edit mask of a masked PnP edit from the model itself (DiffEdit, arXiv 2210.11427; parameter names and defaults of diffusers'
        ``StableDiffusionDiffEditPipeline.generate_mask``): the source latents are noised to a middle timestep, the UNet predicts once
        under the source conditioning (``ddim_inv_prompt`` / ``ddim_inv_1st_frame``, the "ddim_inv" set of ``sample_with_pnp``) and once
        under the edit conditioning (``prompt`` / ``image``), the channel sum of the absolute difference is accumulated over
        ``num_maps_per_mask`` noise draws, normalised by ITS MEAN OVER THE CLIP, scaled by ``mask_thresholding_ratio``, clamped and
        thresholded ("Automatic edit mask").  -> bool [F, H, W] on the device, each latent pixel over its 8 x 8 block: the
        ``mask`` of ``enable_masked_edit``, which the CALLER hands over -- this method does not touch the setting.

        Exactly one of ``source_latents`` ([1, 4, F, h, w] clean latents, noised by ``scheduler.add_noise`` with one ``scheduler.draw_noise``
        from ``generator`` per map) and ``ddim_inv_latents_path`` (a ``LatentTrajectory`` or its directory: the deterministic variant --
        x_t is the inversion's entry at the scheduled timestep nearest to the chosen one, ONE map, no noise).  No classifier-free
        guidance: two branches [source, edit] of the same x_t.  With HIP graphs one captured graph (forward + accumulate) is replayed
        for every map; ``ANYV2V_NO_GRAPH=1`` runs the same launches eagerly.  ``trace``: a dict that receives ``map`` (fp16 [F, h, w]),
        ``timestep``, ``acc`` (fp32 [F, h, w]) and ``x_t`` (one per map)."""
        from .pipeline import _use_graphs
        height = height or self.unet.config.sample_size * self.vae_scale_factor
        width = width or self.unet.config.sample_size * self.vae_scale_factor
        if getattr(self.unet, "frame_parallel", None) is not None:
            raise NotImplementedError("generate_edit_mask on a frame-parallel clip: the clip mean spans all frames and would need a collective")
        if pnp_utils.has_foreign_hooks(self.unet):
            raise ValueError("generate_edit_mask: foreign hooks are plugged into the UNet; they slice the batch in thirds and this forward has "
                             "two branches [source, edit]")
        if any(pnp_utils.injection_state(self)):
            raise ValueError("generate_edit_mask: PnP injection is left registered for the current timestep; the hooks assume the 3-way batch "
                             "[source, negative, editing] and this forward has two branches -- call pnp_utils.clear_time(pipe) first")
        if isinstance(prompt, (list, tuple)) or isinstance(ddim_inv_prompt, (list, tuple)):
            raise ValueError("generate_edit_mask: got a list of prompts: one clip per call")
        if (source_latents is None) == (ddim_inv_latents_path is None):
            raise ValueError("generate_edit_mask: exactly one of source_latents (noise draws) and ddim_inv_latents_path (the inversion "
                             "trajectory, deterministic) must be given")
        if height % 8 != 0 or width % 8 != 0 or height < 8 or width < 8:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        N = _int_in("num_maps_per_mask", num_maps_per_mask, 1, None)
        strength, ratio, threshold = float(mask_encode_strength), float(mask_thresholding_ratio), float(threshold)
        if not 0.0 < strength <= 1.0:   # (also refuses NaN)
            raise ValueError(f"mask_encode_strength={mask_encode_strength}: 0 < mask_encode_strength <= 1")
        if not (ratio > 0.0 and math.isfinite(ratio)):
            raise ValueError(f"mask_thresholding_ratio={mask_thresholding_ratio}: finite and > 0")
        if not 0.0 < threshold < 1.0:
            raise ValueError(f"threshold={threshold}: 0 < threshold < 1")
        if not isinstance(self.scheduler, DDIMScheduler):
            raise ValueError(f"generate_edit_mask takes its timestep from the forward DDIMScheduler, not {type(self.scheduler).__name__}")
        device = self._execution_device
        F_, h, w = int(num_frames), height // self.vae_scale_factor, width // self.vae_scale_factor
        shape = (1, 4, F_, h, w)
        sched = copy.copy(self.scheduler)   # (a copy: the pipeline's own timesteps stay as the caller set them)
        sched.set_timesteps(int(num_inference_steps))
        t = edit_mask_timestep(sched.timesteps, int(num_inference_steps), strength)
        if source_latents is not None:
            if not torch.is_tensor(source_latents) or tuple(source_latents.shape) != shape:
                raise ValueError(f"source_latents: {list(shape)} expected for this call, got "
                                 f"{tuple(source_latents.shape) if torch.is_tensor(source_latents) else type(source_latents).__name__}")
            x0, traj_x = source_latents.to(device=device, dtype=torch.float16).contiguous(), None
        else:
            traj = ddim_inv_latents_path if isinstance(ddim_inv_latents_path, LatentTrajectory) else \
                LatentTrajectory.load(ddim_inv_latents_path, device=device)
            if len(traj) == 0:
                raise ValueError(f"generate_edit_mask: no inverted latents in {ddim_inv_latents_path}")
            t = min(traj.keys(), key=lambda k: (abs(int(k) - t), int(k)))   # the scheduled timestep nearest to t (a tie: the lower one)
            traj_x = load_ddim_latents_at_t(t, traj)
            if tuple(traj_x.shape) != shape:
                raise ValueError(f"the inversion trajectory's latents {tuple(traj_x.shape)} do not match the call: {list(shape)} expected")
            x0, traj_x, N = None, traj_x.to(device=device, dtype=torch.float16).contiguous(), 1
        # conditioning: the edit's by ``_conditioning`` without a negative branch (no guidance here), the source's as in ``sample_with_pnp``
        saved, self._guidance_scale = self._guidance_scale, 1.0
        try:
            pe, _npe, ie, il = self._conditioning(prompt, image, height, width, F_, None, prompt_embeds, None, target_fps, clip_skip,
                                                  image_embeddings, image_latents)
        finally:
            self._guidance_scale = saved
        self._single_clip(pe, 1)
        spe, sie, sil = self._source_conditioning(ddim_inv_prompt, ddim_inv_1st_frame, height, width, F_, clip_skip, ddim_inv_prompt_embeds,
                                                  ddim_inv_image_embeddings, ddim_inv_image_latents)
        for name, a, b in (("prompt embeddings", spe, pe), ("image embeddings", sie, ie), ("image latents", sil, il)):
            if tuple(a.shape) != tuple(b.shape):
                raise ValueError(f"generate_edit_mask: the source's {name} {tuple(a.shape)} do not match the edit's {tuple(b.shape)}")
        if tuple(il.shape) != shape:
            raise ValueError(f"image latents {tuple(il.shape)} do not match the call: {list(shape)} expected")
        ehs, ie_all, il_all = torch.cat([spe, pe]).contiguous(), torch.cat([sie, ie]).contiguous(), torch.cat([sil, il]).contiguous()
        fps = torch.tensor([target_fps] * 2, device=device)
        unet = self.unet
        if not unet._packed:
            unet.pack()
        sample = torch.zeros((2,) + shape[1:], dtype=torch.float16, device=device)   # static: both slots hold the same x_t
        acc = torch.empty(F_ * h * w, dtype=torch.float32, device=device)             # (never read before the first map overwrites it)
        first = torch.ones(1, dtype=torch.int32, device=device)                       # the accumulate launch's device flag
        use_graphs, graph, xs = _use_graphs() and sample.is_cuda, None, []
        with ops.workspace_slot(getattr(self, "ws_slot", 0)):
            ctx = unet._prepare_clip(2, F_, h, w, ehs, fps, il_all, ie_all)
            ctx.shared_stem = False   # (the two branches differ in their image latents)
            ctx.t_buf.fill_(float(t))

            def body():
                vtok = unet._forward_core(ctx, sample)   # the raw prediction, whatever ``prediction_type`` the model has
                ops.diff_map_accum(vtok, shape[1], F_, h * w, acc, first)

            for k in range(N):
                # x_t OUTSIDE the graph, in torch: one draw per map from the caller's generator (a draw recorded inside a graph would
                # replay the same noise), and the same rounded x_t into both batch slots
                x = traj_x if traj_x is not None else sched.add_noise(x0, sched.draw_noise(x0, generator), torch.tensor([t]))
                sample[0].copy_(x[0])
                sample[1].copy_(x[0])
                first.fill_(1 if k == 0 else 0)
                if trace is not None:
                    xs.append(x.clone())
                if not use_graphs:
                    body()
                    continue
                if graph is None:
                    unet._forward_core(ctx, sample)   # warm up eagerly on the side (pure), then capture
                    torch.cuda.synchronize()
                    graph = torch.cuda.CUDAGraph()
                    with capture_hip_graph(graph):
                        body()
                graph.replay()
            soft, pixel = ops.diff_map_finish(acc, F_, h, w, ratio, threshold)
        if graph is not None:
            torch.cuda.current_stream().synchronize()   # once per clip: the graph and its pool go back before the edit's engines capture
            release_graphs([graph])
            del graph
        if trace is not None:
            trace.update(map=soft, timestep=int(t), acc=acc.view(F_, h, w).clone(), x_t=xs)
        return pixel
