"""YAML-template + JSON-override configs with ``${...}`` interpolation: the subset of OmegaConf the reference's
runners use (``OmegaConf.load`` / ``create`` / ``merge`` / ``to_yaml``, attribute access, nested groups, lazy
``${key}`` / ``${group.key}`` interpolation -- ``i2vgen-xl/run_group_pnp_edit.py:81,195`` and
``configs/group_*/template.yaml``).  OmegaConf itself is not installed here; PyYAML is."""
from __future__ import annotations

import copy
import re
from typing import Any

import yaml

_PAT = re.compile(r"\$\{([^{}]+)\}")


class Config:
    """Nested dict with attribute access; string values are interpolated lazily against the ROOT config."""

    def __init__(self, data=None, root: "Config" = None):
        object.__setattr__(self, "_data", {})
        object.__setattr__(self, "_root", root if root is not None else self)
        for k, v in (data or {}).items():
            self._data[k] = self._wrap(v)

    def _wrap(self, v):
        if isinstance(v, Config):
            return Config(v.to_container(resolve=False), self._root)
        if isinstance(v, dict):
            return Config(v, self._root)
        return v

    # -- access
    def _resolve(self, v, depth=0):
        if isinstance(v, str) and "${" in v:
            if depth > 32:
                raise ValueError(f"interpolation cycle in {v!r}")
            m = _PAT.fullmatch(v)
            if m:  # whole value is one reference: keep the referenced type (e.g. a list)
                return self._resolve(self._root._lookup(m.group(1)), depth + 1)
            return _PAT.sub(lambda mm: str(self._resolve(self._root._lookup(mm.group(1)), depth + 1)), v)
        return v

    def _lookup(self, dotted: str):
        node: Any = self
        for part in dotted.strip().split("."):
            if not isinstance(node, Config) or part not in node._data:
                raise KeyError(f"interpolation key '{dotted}' not found")
            node = node._data[part]
        return node

    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(f"Missing key {k}")

    def __getitem__(self, k):
        return self._resolve(self._data[k])

    def __setattr__(self, k, v):
        self._data[k] = self._wrap(v)

    __setitem__ = __setattr__

    def __contains__(self, k):
        return k in self._data

    def get(self, k, default=None):
        return self[k] if k in self._data else default

    def keys(self):
        return self._data.keys()

    def items(self):
        return [(k, self[k]) for k in self._data]

    def __iter__(self):
        return iter(self._data)

    def to_container(self, resolve=True):
        out = {}
        for k, v in self._data.items():
            if isinstance(v, Config):
                out[k] = v.to_container(resolve)
            else:
                out[k] = self._resolve(v) if resolve else v
        return out

    def __repr__(self):
        return f"Config({self.to_container(resolve=False)!r})"


def sampler_options(config) -> tuple:
    """(eta, guidance_rescale) of a PnP-edit configuration (template YAML merged with a JSON entry, or a front-end's ``pnp_config``):
    two OPTIONAL keys the reference's files do not have -- ``eta`` (stochastic DDIM, 0 <= eta <= 1) and ``guidance_rescale`` (Lin et
    al.'s rescale, 0 <= phi <= 1).  Absent (or null) means off, and a job whose files name neither runs and writes exactly what it
    did before the keys existed."""
    def one(key):
        v = config.get(key, None) if hasattr(config, "get") else getattr(config, key, None)   # (a ``Config`` or any plain namespace)
        if v is None:
            return 0.0
        v = float(v)
        if not 0.0 <= v <= 1.0:
            raise ValueError(f"{key}={v}: 0 <= {key} <= 1")
        return v
    return one("eta"), one("guidance_rescale")


def _option(config, key):
    return config.get(key, None) if hasattr(config, "get") else getattr(config, key, None)   # (a ``Config`` or any plain namespace)


def _auto_mask_on(config) -> bool:
    v = _option(config, "edit_mask_auto")
    if v is not None and not isinstance(v, bool):
        raise ValueError(f"edit_mask_auto={v!r}: true or false")
    return bool(v)


def _grow_feather(grow, feather):
    grow = 0 if grow is None else grow
    feather = 0.0 if feather is None else float(feather)
    if isinstance(grow, bool) or not 0 <= grow <= 8 or int(grow) != grow:   # (the range check also refuses NaN)
        raise ValueError(f"edit_mask_grow={grow}: an integer, 0 <= edit_mask_grow <= 8")
    if not 0.0 <= feather <= 8.0:   # (also refuses NaN)
        raise ValueError(f"edit_mask_feather={feather}: 0 <= edit_mask_feather <= 8")
    return int(grow), feather


def masked_edit_options(config):
    """(edit_mask_path, grow, feather) of a PnP-edit configuration, or None: three OPTIONAL keys the reference's files do not have --
    ``edit_mask_path`` (one PNG, or a directory of ``%05d.png`` files; white = edit, black = keep the source), ``edit_mask_grow`` (latent
    pixels, integer 0 .. 8) and ``edit_mask_feather`` (sigma in latent pixels, 0 .. 8) -- for ``I2VGenXLPipeline.enable_masked_edit``.
    Without ``edit_mask_path`` (absent or null) the entry runs and writes exactly what it did before the keys existed; grow / feather
    without a path are refused, not dropped -- unless the mask is an automatic one (``auto_mask_options``), which they then shape."""
    path, grow, feather = _option(config, "edit_mask_path"), _option(config, "edit_mask_grow"), _option(config, "edit_mask_feather")
    if path is None:
        if (grow is not None or feather is not None) and not _auto_mask_on(config) and not _first_frame_mask_on(config):
            raise ValueError("edit_mask_grow / edit_mask_feather without edit_mask_path: there is no mask to grow or feather")
        return None
    if _auto_mask_on(config):
        raise ValueError("edit_mask_auto together with edit_mask_path: the mask is either generated or loaded")
    if _first_frame_mask_on(config):
        raise ValueError("edit_mask_first_frame together with edit_mask_path: the mask is either derived from the first frames or loaded")
    grow, feather = _grow_feather(grow, feather)
    return str(path), grow, feather


def _first_frame_mask_on(config) -> bool:
    v = _option(config, "edit_mask_first_frame")
    if v is not None and not isinstance(v, bool):
        raise ValueError(f"edit_mask_first_frame={v!r}: true or false")
    return bool(v)


def _int_option(key, v, default, lo, hi):
    v = default if v is None else v
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not lo <= v <= hi or int(v) != v:   # (also refuses NaN)
        raise ValueError(f"{key}={v}: an integer, {lo} <= {key} <= {hi}")
    return int(v)


FIRST_FRAME_MASK_DEFAULTS = dict(threshold=24, min_count=8)   # ``I2VGenXLPipeline.first_frame_edit_mask``'s


def first_frame_mask_options(config):
    """The first-frame difference mask of a PnP-edit configuration (``I2VGenXLPipeline.first_frame_edit_mask``), or None: OPTIONAL keys the
    reference's files do not have -- ``edit_mask_first_frame`` (bool) switches it on, ``edit_mask_first_frame_threshold`` (integer 0 .. 255)
    and ``edit_mask_first_frame_min_count`` (integer 1 .. 64) tune it; ``edit_mask_grow`` / ``edit_mask_feather`` shape the mask as they
    shape a loaded one.  -> dict(threshold, min_count, grow, feather).  A third source of the mask, exclusive with ``edit_mask_path`` and
    ``edit_mask_auto``; alone it is a static [1, H, W] mask like a single PNG, ``edit_mask_track`` (``track_options``) carries it through the
    clip.  Absent, null or false: None, and the entry runs and writes exactly what it did before the keys existed; the tuning keys without
    the switch are refused, not dropped."""
    vals = {k: _option(config, "edit_mask_first_frame_" + k) for k in FIRST_FRAME_MASK_DEFAULTS}
    if not _first_frame_mask_on(config):
        given = [k for k, v in vals.items() if v is not None]
        if given:
            raise ValueError(f"edit_mask_first_frame_{given[0]} without edit_mask_first_frame: there is no first-frame mask to tune")
        return None
    if _option(config, "edit_mask_path") is not None:
        raise ValueError("edit_mask_first_frame together with edit_mask_path: the mask is either derived from the first frames or loaded")
    if _auto_mask_on(config):
        raise ValueError("edit_mask_first_frame together with edit_mask_auto: the mask is either derived from the first frames or generated")
    grow, feather = _grow_feather(_option(config, "edit_mask_grow"), _option(config, "edit_mask_feather"))
    return dict(threshold=_int_option("edit_mask_first_frame_threshold", vals["threshold"], FIRST_FRAME_MASK_DEFAULTS["threshold"], 0, 255),
                min_count=_int_option("edit_mask_first_frame_min_count", vals["min_count"], FIRST_FRAME_MASK_DEFAULTS["min_count"], 1, 64),
                grow=grow, feather=feather)


TRACK_DEFAULTS = dict(radius=16, median=True)   # ``I2VGenXLPipeline.propagate_edit_mask``'s


def track_options(config):
    """The mask tracking of a PnP-edit configuration (``I2VGenXLPipeline.propagate_edit_mask``), or None: OPTIONAL keys the reference's
    files do not have -- ``edit_mask_track`` (bool) carries a one-frame mask through the clip along the block-matched motion of the source
    frames, ``edit_mask_track_radius`` (pixels per frame, integer 0 .. 32) and ``edit_mask_track_median`` (bool) tune it.
    -> dict(radius, median).  It needs a one-frame mask: ``edit_mask_first_frame``, or an ``edit_mask_path`` that is a single file (the
    runner refuses a directory of per-frame masks); an automatic mask already has every frame, so ``edit_mask_auto`` is refused.  Absent,
    null or false: None; the tuning keys without the switch are refused, not dropped."""
    on, median, radius = _option(config, "edit_mask_track"), _option(config, "edit_mask_track_median"), _option(config, "edit_mask_track_radius")
    for key, v in (("edit_mask_track", on), ("edit_mask_track_median", median)):
        if v is not None and not isinstance(v, bool):
            raise ValueError(f"{key}={v!r}: true or false")
    if not on:
        for key, v in (("edit_mask_track_radius", radius), ("edit_mask_track_median", median)):
            if v is not None:
                raise ValueError(f"{key} without edit_mask_track: there is no tracking to tune")
        return None
    if _auto_mask_on(config):
        raise ValueError("edit_mask_track together with edit_mask_auto: the generated mask already has every frame")
    if _option(config, "edit_mask_path") is None and not _first_frame_mask_on(config):
        raise ValueError("edit_mask_track without edit_mask_first_frame or edit_mask_path: there is no frame-0 mask to carry")
    return dict(radius=_int_option("edit_mask_track_radius", radius, TRACK_DEFAULTS["radius"], 0, 32),
                median=TRACK_DEFAULTS["median"] if median is None else median)


AUTO_MASK_DEFAULTS = dict(maps=10, strength=0.5, ratio=3.0, threshold=0.5)   # ``I2VGenXLPipeline.generate_edit_mask``'s (diffusers' generate_mask)


def auto_mask_options(config):
    """The automatic edit mask of a PnP-edit configuration (``I2VGenXLPipeline.generate_edit_mask``), or None: OPTIONAL keys the reference's
    files do not have -- ``edit_mask_auto`` (bool) switches it on, ``edit_mask_auto_maps`` (noise draws, integer >= 1),
    ``edit_mask_auto_strength`` (0 < s <= 1: how far the source is noised), ``edit_mask_auto_ratio`` (> 0) and ``edit_mask_auto_threshold``
    (in (0, 1)) tune it; ``edit_mask_grow`` / ``edit_mask_feather`` shape the generated mask as they shape a loaded one.
    -> dict(maps, strength, ratio, threshold, grow, feather).  Absent, null or false: None, and the entry runs and writes exactly what it
    did before the keys existed; the tuning keys without ``edit_mask_auto``, and ``edit_mask_auto`` with ``edit_mask_path``, are refused."""
    import math
    vals = {k: _option(config, "edit_mask_auto_" + k) for k in AUTO_MASK_DEFAULTS}
    if not _auto_mask_on(config):
        given = [k for k, v in vals.items() if v is not None]
        if given:
            raise ValueError(f"edit_mask_auto_{given[0]} without edit_mask_auto: there is no automatic mask to tune")
        return None
    if _option(config, "edit_mask_path") is not None:
        raise ValueError("edit_mask_auto together with edit_mask_path: the mask is either generated or loaded")
    if _first_frame_mask_on(config):
        raise ValueError("edit_mask_first_frame together with edit_mask_auto: the mask is either derived from the first frames or generated")
    maps = AUTO_MASK_DEFAULTS["maps"] if vals["maps"] is None else vals["maps"]
    if isinstance(maps, bool) or not isinstance(maps, (int, float)) or not 1 <= maps < 2 ** 31 or int(maps) != maps:   # (refuses NaN)
        raise ValueError(f"edit_mask_auto_maps={maps}: an integer >= 1")
    num = {k: float(AUTO_MASK_DEFAULTS[k] if vals[k] is None else vals[k]) for k in ("strength", "ratio", "threshold")}
    if not 0.0 < num["strength"] <= 1.0:
        raise ValueError(f"edit_mask_auto_strength={num['strength']}: 0 < edit_mask_auto_strength <= 1")
    if not (num["ratio"] > 0.0 and math.isfinite(num["ratio"])):
        raise ValueError(f"edit_mask_auto_ratio={num['ratio']}: finite and > 0")
    if not 0.0 < num["threshold"] < 1.0:
        raise ValueError(f"edit_mask_auto_threshold={num['threshold']}: 0 < edit_mask_auto_threshold < 1")
    grow, feather = _grow_feather(_option(config, "edit_mask_grow"), _option(config, "edit_mask_feather"))
    return dict(maps=int(maps), grow=grow, feather=feather, **num)


COMPOSITE_DEFAULTS = dict(grow_px=0, feather_px=0.0, match_color=False)   # ``I2VGenXLPipeline.composite_over_source``'s


def composite_options(config):
    """The pixel-space composite of a masked PnP-edit configuration (``I2VGenXLPipeline.composite_over_source``), or None: OPTIONAL keys the
    reference's files do not have -- ``edit_mask_composite`` (bool) switches it on, ``edit_mask_composite_grow`` (pixels, integer 0 .. 64),
    ``edit_mask_composite_feather`` (sigma in pixels, 0 .. 16) and ``edit_mask_match_color`` (bool) shape it.
    -> dict(grow_px, feather_px, match_color).  Absent, null or false: None, and the entry runs and writes exactly what it did before the
    keys existed; the shaping keys without ``edit_mask_composite``, and ``edit_mask_composite`` without a mask (``edit_mask_path`` or
    ``edit_mask_auto``), are refused, not dropped."""
    on, match = _option(config, "edit_mask_composite"), _option(config, "edit_mask_match_color")
    for key, v in (("edit_mask_composite", on), ("edit_mask_match_color", match)):
        if v is not None and not isinstance(v, bool):
            raise ValueError(f"{key}={v!r}: true or false")
    grow, feather = _option(config, "edit_mask_composite_grow"), _option(config, "edit_mask_composite_feather")
    if not on:
        for key, v in (("edit_mask_composite_grow", grow), ("edit_mask_composite_feather", feather), ("edit_mask_match_color", match)):
            if v is not None:
                raise ValueError(f"{key} without edit_mask_composite: there is no composite to shape")
        return None
    if _option(config, "edit_mask_path") is None and not _auto_mask_on(config) and not _first_frame_mask_on(config):
        raise ValueError("edit_mask_composite without edit_mask_path or edit_mask_auto: there is no mask to composite by")
    grow = 0 if grow is None else grow
    feather = 0.0 if feather is None else float(feather)
    if isinstance(grow, bool) or not isinstance(grow, (int, float)) or not 0 <= grow <= 64 or int(grow) != grow:   # (also refuses NaN)
        raise ValueError(f"edit_mask_composite_grow={grow}: an integer, 0 <= edit_mask_composite_grow <= 64")
    if not 0.0 <= feather <= 16.0:   # (also refuses NaN)
        raise ValueError(f"edit_mask_composite_feather={feather}: 0 <= edit_mask_composite_feather <= 16")
    return dict(grow_px=int(grow), feather_px=feather, match_color=bool(match))


def _rebind(cfg: Config, root: Config):
    object.__setattr__(cfg, "_root", root)
    for v in cfg._data.values():
        if isinstance(v, Config):
            _rebind(v, root)


class OmegaConf:
    """Drop-in for the four OmegaConf calls the reference makes."""

    @staticmethod
    def load(path) -> Config:
        with open(path) as f:
            return Config(yaml.safe_load(f) or {})

    @staticmethod
    def create(obj=None) -> Config:
        return Config(copy.deepcopy(obj) if obj is not None else {})

    @staticmethod
    def merge(*cfgs) -> Config:
        def merge2(a: dict, b: dict):
            for k, v in b.items():
                if isinstance(v, dict) and isinstance(a.get(k), dict):
                    merge2(a[k], v)
                else:
                    a[k] = copy.deepcopy(v)
            return a
        acc: dict = {}
        for c in cfgs:
            merge2(acc, c.to_container(resolve=False) if isinstance(c, Config) else dict(c))
        out = Config(acc)
        _rebind(out, out)
        return out

    @staticmethod
    def from_dotlist(items) -> Config:
        """``["a.b=1", "c=text"]`` -> nested config; values parsed as YAML scalars (``consisti2v/run_pnp_edit.py:138-140``)."""
        acc: dict = {}
        for it in items:
            key, _, val = str(it).partition("=")
            node = acc
            parts = key.strip().split(".")
            for part in parts[:-1]:
                node = node.setdefault(part, {})
            node[parts[-1]] = yaml.safe_load(val) if val != "" else None
        return Config(acc)

    @staticmethod
    def to_yaml(cfg: Config, resolve: bool = False) -> str:
        return yaml.safe_dump(cfg.to_container(resolve=resolve), sort_keys=False)

    @staticmethod
    def to_container(cfg: Config, resolve: bool = False):
        return cfg.to_container(resolve=resolve)
