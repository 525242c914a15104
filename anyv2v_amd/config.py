"""YAML-template + JSON-override configs with ``${...}`` interpolation: the subset of OmegaConf the reference's
runners use (``OmegaConf.load`` / ``create`` / ``merge`` / ``to_yaml``, attribute access, nested groups, lazy
``${key}`` / ``${group.key}`` interpolation -- ``i2vgen-xl/run_group_pnp_edit.py:81,195`` and
``configs/group_*/template.yaml``).  OmegaConf itself is not installed here; PyYAML is."""
from __future__ import annotations

import copy
import re
from typing import Any

import yaml

from .masked_edit import AUTO_MASK_DEFAULTS, COMPOSITE_DEFAULTS, FIRST_FRAME_MASK_DEFAULTS, TRACK_DEFAULTS, plan_from_config  # noqa: F401

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


# The OPTIONAL ``edit_mask_*`` keys (the reference's files have none) are read, checked against each other and range-checked in ONE place,
# ``masked_edit.plan_from_config``.  The five functions below document them and return their part of that plan, or None when it is off
# (absent, null or false: the entry runs and writes exactly what it did before the keys existed).  A key with nothing to act on is refused.
def masked_edit_options(config):
    """-> (edit_mask_path, grow, feather) for ``I2VGenXLPipeline.enable_masked_edit``: ``edit_mask_path`` (one PNG, or a directory of
    ``%05d.png`` files; white = edit, black = keep the source), ``edit_mask_grow`` (latent pixels, integer 0 .. 8) and ``edit_mask_feather``
    (sigma in latent pixels, 0 .. 8).  Grow / feather without a path are refused -- unless the mask is an automatic or a first-frame one,
    which they then shape."""
    plan = plan_from_config(config)
    return (plan.path, plan.grow, plan.feather) if plan is not None and plan.source == "path" else None


def first_frame_mask_options(config):
    """-> dict(threshold, min_count, grow, feather) for ``I2VGenXLPipeline.first_frame_edit_mask``: ``edit_mask_first_frame`` (bool) switches
    the first-frame difference mask on, ``edit_mask_first_frame_threshold`` (integer 0 .. 255) and ``edit_mask_first_frame_min_count``
    (integer 1 .. 64) tune it; ``edit_mask_grow`` / ``edit_mask_feather`` shape it like a loaded one.  A third source of the mask, exclusive with
    ``edit_mask_path`` and ``edit_mask_auto``; alone it is a static [1, H, W] mask like a single PNG, ``edit_mask_track`` carries it on."""
    plan = plan_from_config(config)
    return None if plan is None or plan.first_frame is None else dict(plan.first_frame, grow=plan.grow, feather=plan.feather)


def track_options(config):
    """-> dict(radius, median) for ``I2VGenXLPipeline.propagate_edit_mask``: ``edit_mask_track`` (bool) carries a one-frame mask through the
    clip along the block-matched motion of the source frames, ``edit_mask_track_radius`` (pixels per frame, integer 0 .. 32) and
    ``edit_mask_track_median`` (bool) tune it.  It needs a one-frame mask: ``edit_mask_first_frame``, or an ``edit_mask_path`` that is a single
    file (the runner refuses a directory of per-frame masks); an automatic mask already has every frame, so ``edit_mask_auto`` is refused."""
    plan = plan_from_config(config)
    return None if plan is None or plan.track is None else dict(plan.track)


def auto_mask_options(config):
    """-> dict(maps, strength, ratio, threshold, grow, feather) for ``I2VGenXLPipeline.generate_edit_mask``: ``edit_mask_auto`` (bool) switches
    the automatic mask on, ``edit_mask_auto_maps`` (noise draws, integer >= 1), ``edit_mask_auto_strength`` (0 < s <= 1: how far the source is
    noised), ``edit_mask_auto_ratio`` (> 0) and ``edit_mask_auto_threshold`` (in (0, 1)) tune it; ``edit_mask_grow`` / ``edit_mask_feather``
    shape the generated mask like a loaded one.  Refused together with another source of the mask."""
    plan = plan_from_config(config)
    return None if plan is None or plan.auto is None else dict(plan.auto, grow=plan.grow, feather=plan.feather)


def composite_options(config):
    """-> dict(grow_px, feather_px, match_color) for ``I2VGenXLPipeline.composite_over_source``: ``edit_mask_composite`` (bool) switches the
    pixel-space composite on, ``edit_mask_composite_grow`` (pixels, integer 0 .. 64), ``edit_mask_composite_feather`` (sigma in pixels,
    0 .. 16) and ``edit_mask_match_color`` (bool) shape it.  Refused without a mask (``edit_mask_path``, ``_auto`` or ``_first_frame``)."""
    plan = plan_from_config(config)
    return None if plan is None or plan.composite is None else dict(plan.composite)


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
