"""What the I2VGen-XL loops of ``pipeline.py`` step with: one denoising step on static buffers, captured into a HIP graph and replayed
(``_StepEngine``); the engines a pipeline keeps across clips (``cached_engine``); the source features a multi-edit job keeps
(``SourceFeatureCache``); which engine runs a PnP step under which graph key (``pnp_step_plan``).  ``pipeline.py`` re-exports them."""
from __future__ import annotations

import os
from contextlib import contextmanager, nullcontext
from typing import Dict, Optional

import torch

from . import ops, pnp_utils
from .utils import capture_hip_graph, release_graphs


def _use_graphs() -> bool:
    return os.environ.get("ANYV2V_NO_GRAPH", "0") != "1"


class SourceFeatureCache:
    """Job-level exact saving for several edits of ONE clip (``configs/group_pnp_edit/group_config.json`` holds 8 edits of one
    clip): the source branch of ``sample_with_pnp`` is only a feature generator -- its v-prediction is discarded
    (``pipeline_i2vgen_xl.py:1136,1160-1162``) and it depends on the clip, its inversion and the step, not on the edit.  The first
    edit runs the three-branch steps and RECORDS, per step and injected hook site, what the other branches read from the source
    branch (Q | K of the 16 attention sites, the conv features of ``up_blocks[1].resnets[1]``); every further edit of the same
    clip REPLAYS them and runs [negative, editing] only.  Kept in HBM (~0.85 GB per fully injected step at 16 f x 512^2).

    ``signature``: what the recorded features depend on; a different one (next clip, other weights) empties the cache."""

    def __init__(self, max_bytes: Optional[int] = None):
        self.signature = None
        self.steps: Dict[tuple, Dict[str, torch.Tensor]] = {}   # (t, injection state) -> site -> features
        self.recorded_steps = self.replayed_steps = 0
        # byte budget (``ANYV2V_SOURCE_CACHE_GB``, default 96 GB of the 288): a step that would exceed it is simply not recorded and
        # runs as a three-branch step in every edit -- same results, no saving for that step
        self.max_bytes = int(float(os.environ.get("ANYV2V_SOURCE_CACHE_GB", "96")) * 2 ** 30) if max_bytes is None else int(max_bytes)
        self.skipped_steps = 0
        self.sites = []   # the hook sites of the current run: ``begin_run`` (the site buffers stay with the run's engine)

    def store(self, t, state, feats: Dict[str, torch.Tensor]) -> bool:
        need = sum(v.numel() * v.element_size() for v in feats.values())
        if self.nbytes() + need > self.max_bytes:
            self.skipped_steps += 1
            return False
        self.steps[(int(t), tuple(state))] = {n: v.clone() for n, v in feats.items()}
        return True

    def bind(self, signature):
        if signature != self.signature:
            self.steps.clear()
            self.signature = signature

    def has(self, t, state) -> bool:
        """Features of step ``t`` recorded under exactly this injection ``state`` (which sites are on).  The same state, not a
        superset: the source branch's own arithmetic depends on it at the rounding level (on a conv-injection step its main path
        runs as a one-branch launch with its own split-K plan, at an injected attention site its Q | K | V come from a one-branch
        projection), so only a same-state record reproduces the uncached edit bit for bit."""
        return (int(t), tuple(state)) in self.steps

    def nbytes(self) -> int:
        return sum(v.numel() * v.element_size() for d in self.steps.values() for v in d.values())

    def begin_run(self, pipe, eng, source, ts, first_latent, source_cond, target_fps, latents_shape):
        """One ``sample_with_pnp`` call: binds the run's signature (trajectory, timesteps, source conditioning, weights, FreeU), takes the
        hook sites and gives the three-branch engine its static site buffers (captured steps write and read THEM; the cache holds clones)."""
        fp_ = lambda x: (tuple(x.shape), float(x.float().sum()), float(x.float().abs().sum()))
        self.bind((source, tuple(ts), fp_(first_latent)) + tuple(fp_(x) for x in source_cond)
                  + (int(target_fps), pipe.unet._pack_gen, id(pipe.unet), tuple(latents_shape), getattr(pipe.unet, "freeu", None)))
        self.sites = pnp_utils.injection_sites(pipe)
        if eng.site_bufs is None:
            # rows of ONE branch at the site's level: up_blocks[1] works at 1/16 of the 64x64 level's pixels, [2] at 1/4, [3] at 1/1
            _, _, F, h, w = eng.sample.shape
            level_div = {"1": 16, "2": 4, "3": 1}
            eng.site_bufs = {name: torch.empty((F * h * w // level_div[name.split(".up")[1][0]], cols), dtype=torch.float16,
                                               device=eng.sample.device) for name, _obj, cols in self.sites}

    def _set_io(self, mode, bufs=None, names=()):
        for name, obj, _ in self.sites:
            obj.src_io = (mode, bufs[name]) if (mode is not None and name in names) else None

    @contextmanager
    def step_io(self, eng, kind, t, state):
        """Around a "record" / "replay" step at ``t`` of the run ``begin_run`` opened on ``eng``: "replay" fills the engine's site
        buffers from the cache and lets the sites that are on read them; "record" lets them write and stores the buffers afterwards."""
        bufs, names = eng.site_bufs, [n for (n, _, _), on in zip(self.sites, state) if on]
        if kind == "replay":
            for n in names:
                bufs[n].copy_(self.steps[(int(t), state)][n], non_blocking=True)
        self._set_io(kind, bufs, names)
        yield
        self._set_io(None)
        if kind == "replay":
            self.replayed_steps += 1
        else:
            self.recorded_steps += bool(self.store(t, state, {n: bufs[n] for n in names}))


def pnp_step_plan(nb, skip_src, state, cached):
    """The step at the registered time -> (kind, graph key).  ``state``: the injection decision of every hook site; ``cached``: None
    without a source-feature cache, else whether this step's features are recorded.  "nosrc" (no site on: nothing reads the source
    branch) and "replay" run on the [negative, editing] twin, "record" and "pnp" on the three-branch engine."""
    if any(state) and nb != 3:
        # the hooks slice the batch in thirds (pnp_utils.py:111,166,272); with guidance_scale <= 1 the reference
        # builds a 2-way batch and silently injects the wrong rows -- refuse instead
        raise ValueError("PnP feature injection needs classifier-free guidance (guidance_scale > 1): the hooks "
                         "assume the 3-way batch [source, negative, editing]")
    if skip_src and not any(state):
        return "nosrc", ("pnp-nosrc",)
    if cached:
        return "replay", ("pnp-replay",) + state
    if cached is not None:
        return "record", ("pnp-record",) + state
    return "pnp", ("pnp",) + state


class _StepEngine:
    """One denoising step = UNet forward on ``sample[B,4,F,h,w]`` + fused CFG/DDIM update of the latent slot.

    ``sample`` is a static buffer: slot ``lat_slot`` (the last one) IS the latent being denoised and is updated in
    place; ``dup_slots`` are re-filled from it after the update (CFG feeds the same latent twice); slot 0 of a PnP
    step is overwritten by the caller with the source trajectory before each step.
    """

    def __init__(self, pipe, sample, cond, b_unc, b_cond, guidance, dup_slots, shared_stem=False, batch_hint=None, lat_slots=None,
                 stochastic=False, rescale=0.0, blend=None, drop_src_tail=False):
        self.pipe, self.unet = pipe, pipe.unet
        # masked edit (``enable_masked_edit``): static buffers (partner latent [1, 4, F, h, w], latent mask [Fm, h, w]) the captured step
        # blends the latent slot against, behind the update.  The caller owns them -- the three-branch engine and its [negative, editing]
        # twins step the SAME latent and share one pair -- and refills the partner before every step.  None: nothing is launched
        self.blend = None if blend is None else tuple(blend)
        assert not (self.blend is not None and lat_slots is not None), "the batched inversion has no masked edit"
        # sampler options (``_SamplerOptions``): with either one on, the step is ``ops.cfg_ddim_step_ex`` on an 8-float coefficient row
        # (+ ``ops.guidance_stats`` in front of it under the rescale); with both off, nothing below differs from the default engine
        self.stochastic, self.rescale = bool(stochastic), float(rescale)
        self.options = self.stochastic or self.rescale > 0.0
        assert not (self.options and lat_slots is not None), "the batched inversion has no sampler options"
        # (num, den): this engine runs a subset of another engine's branches ([negative, editing] of a three-branch edit step) and
        # must make the same launch choices -- ops.batch_hint
        self.batch_hint = batch_hint
        # slot 0 is the PnP source branch, never read by the update: its forward stops behind the last hook site (unet._forward_core)
        self.drop_src_tail = bool(drop_src_tail)
        self.sample, self.cond = sample, cond
        self.b_unc, self.b_cond, self.guidance = b_unc, b_cond, float(guidance)
        self.lat_slot = sample.shape[0] - 1
        # several clips inverted in one batch (``invert_clips``): every slot is a latent of its own, stepped without guidance
        self.lat_slots = None if lat_slots is None else list(lat_slots)
        self.dup_slots = list(dup_slots)
        self.coef = torch.zeros(8 if self.options else 4, dtype=torch.float32, device=sample.device)
        # static operands of the captured step: the variance noise of THIS step (copied in before every replay -- drawn outside the
        # graph, from the caller's generator) and the records of the rescale statistics
        self.noise = torch.zeros_like(sample[:1]) if self.stochastic else None
        self.gstats = (torch.zeros(ops.GUIDANCE_STATS_FLOATS, dtype=torch.float32, device=sample.device)
                       if self.rescale > 0.0 and b_unc >= 0 else None)   # (no guidance, no rescale: pipeline_video_editing.py:685)
        self.graphs: Dict[tuple, torch.cuda.CUDAGraph] = {}
        # (a frame-parallel forward contains collectives: run eagerly -- at 128 frames launch overhead is irrelevant)
        # (likewise with foreign hooks on the seams B1 / B2: torch-style code that may sync, e.g. ``t in cuda_tensor``)
        self.use_graphs = (_use_graphs() and sample.is_cuda and getattr(pipe.unet, "frame_parallel", None) is None
                           and not pnp_utils.has_foreign_hooks(pipe.unet))
        # built on demand: the [negative, editing] engine of a PnP edit (``bind_nosrc``), the source features' buffers (``begin_run``)
        self.nosrc = self.site_bufs = None
        if not self.unet._packed:
            self.unet.pack()
        self.ctx = self._prepare_clip(cond)
        # CFG batches [.., negative, positive]: the last two slots hold the same latent (dup_slots) and -- checked here,
        # once -- the same image latents and fps, so the UNet may share their stem (exact; unet._forward_core)
        self._shared_stem_requested = bool(shared_stem)
        self.ctx.shared_stem = self._stem_shared(cond)

    def _prepare_clip(self, cond):
        B, _, F, H, W = self.sample.shape
        with ops.batch_hint(*(self.batch_hint or (1, 1))):
            return self.unet._prepare_clip(B, F, H, W, cond["encoder_hidden_states"], cond["fps"], cond["image_latents"],
                                           cond["image_embeddings"])

    def _stem_shared(self, cond) -> bool:
        B = self.sample.shape[0]
        return bool(self._shared_stem_requested and B >= 2 and os.environ.get("ANYV2V_SHARED_STEM", "1") == "1"
                    and torch.equal(cond["image_latents"][B - 2], cond["image_latents"][B - 1])
                    and torch.equal(cond["fps"][B - 2], cond["fps"][B - 1]))

    def rebind(self, sample_init, cond) -> bool:
        """Point this engine (its static buffers and captured graphs) at another clip of the same geometry: the new latents go
        into ``self.sample``, the new clip's step-invariant tensors are computed by ``_prepare_clip`` and copied INTO the
        context tensors the graphs were captured on.  False if the clip cannot run on this engine (different shared-stem
        decision): the caller then builds a fresh one."""
        if self._stem_shared(cond) != self.ctx.shared_stem:
            return False
        if sample_init.data_ptr() != self.sample.data_ptr():
            self.sample.copy_(sample_init)
        fresh = self._prepare_clip(cond)
        if fresh is not self.ctx:
            if (fresh.Sk, fresh.F) != (self.ctx.Sk, self.ctx.F):
                return False
            for name, new in vars(fresh).items():
                old = getattr(self.ctx, name, None)
                if torch.is_tensor(new) and name not in ("stats", "t_buf"):
                    if not torch.is_tensor(old) or old.shape != new.shape or old.dtype != new.dtype:
                        return False
                    old.copy_(new)
            self.ctx.key, self.ctx._keepalive = fresh.key, fresh._keepalive
            self.unet._ctx = self.ctx
        self.cond = cond
        return True

    def bind_nosrc(self) -> "_StepEngine":
        """The [negative, editing] twin of this three-branch engine, pointed at this engine's clip: built once per engine (on
        ``sample[1:]`` and the blend buffers, so the two can alternate freely), re-pointed once per ``sample_with_pnp`` call."""
        cond = {k: v[1:].contiguous() for k, v in self.cond.items()}
        if self.nosrc is None or not self.nosrc.rebind(self.sample[1:], cond):
            self.nosrc = _StepEngine(self.pipe, self.sample[1:], cond, b_unc=0, b_cond=1, guidance=self.guidance, dup_slots=[0], shared_stem=True,
                                     batch_hint=(3, 2), stochastic=self.stochastic, rescale=self.rescale, blend=self.blend)
        return self.nosrc

    def _forward(self):
        """The UNet forward under this engine's batch hint and tail setting: the warm-up and the captured body run the same one."""
        if self.batch_hint is not None:
            self.ctx.batch_hint = self.batch_hint   # (the forward switches between the stem's and the full batch's ratio)
        with (nullcontext() if self.batch_hint is None else ops.batch_hint(*self.batch_hint)):
            return self.unet._forward_core(self.ctx, self.sample, drop_source_tail=self.drop_src_tail)

    def _body(self):
        vtok = self._forward()
        if self.lat_slots is not None:
            for L in self.lat_slots:
                lat = self.sample[L:L + 1]
                ops.cfg_ddim_step(vtok, -1, L, 1.0, self.coef, lat, lat)
            return
        L = self.lat_slot
        lat = self.sample[L:L + 1]
        off = 1 if vtok.shape[0] != self.sample.shape[0] * self.sample.shape[2] * self.sample.shape[3] * self.sample.shape[4] else 0
        b_unc, b_cond = self.b_unc - off if self.b_unc >= 0 else self.b_unc, self.b_cond - off
        if self.options:
            if self.gstats is not None:
                ops.guidance_stats(vtok, b_unc, b_cond, self.guidance, lat.shape, out=self.gstats)
            ops.cfg_ddim_step_ex(vtok, b_unc, b_cond, self.guidance, self.coef, lat, lat, prediction=self.pipe.scheduler.prediction,
                                 stats=self.gstats, phi=self.rescale if self.gstats is not None else 0.0, noise=self.noise)
        else:
            ops.cfg_ddim_step(vtok, b_unc, b_cond, self.guidance, self.coef, lat, lat)
        if self.blend is not None:
            ops.masked_blend(lat, self.blend[0], self.blend[1], out=lat)   # in place, before the copies: every slot gets the blended latent
        for s in self.dup_slots:
            self.sample[s].copy_(self.sample[L])

    def step(self, t_row: torch.Tensor, coef_row: torch.Tensor, key: tuple, noise: Optional[torch.Tensor] = None,
             partner: Optional[torch.Tensor] = None):
        """``noise``: this step's variance noise (a stochastic engine needs a fresh draw for every step).  ``partner``: the latent a
        masked edit keeps outside the mask after THIS step (the source at the level the step arrives at)."""
        with ops.workspace_slot(getattr(self.pipe, "ws_slot", 0)):
            if partner is None:
                self._step(t_row, coef_row, key, noise)   # (the call of an engine without a mask, as it always was)
            else:
                self._step(t_row, coef_row, key + ("blend",), noise, partner)   # (the graph of a masked step holds the blend launch)

    def _step(self, t_row: torch.Tensor, coef_row: torch.Tensor, key: tuple, noise=None, partner=None):
        self.ctx.t_buf.copy_(t_row, non_blocking=True)
        self.coef.copy_(coef_row, non_blocking=True)
        if getattr(self, "blend", None) is not None:
            if partner is None:
                raise ValueError("a masked step engine needs the step's partner latent: replaying the buffer would blend against the last step's")
            self.blend[0].copy_(partner.reshape(self.blend[0].shape), non_blocking=True)
        if self.stochastic:
            if noise is None:
                raise ValueError("a stochastic step engine needs the step's variance noise: replaying the buffer would repeat the last draw")
            self.noise.copy_(noise.reshape(self.noise.shape), non_blocking=True)
        if not self.use_graphs:
            self._body()
            return
        g = self.graphs.get(key)
        if g is None:
            # warm up eagerly on the side (pure: the UNet forward does not touch the latents), then capture
            self._forward()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with capture_hip_graph(g):
                self._body()
            self.graphs[key] = g
            # capture does not execute: fall through to the replay below
        g.replay()


# ------------------------------------------------ the engines a pipeline keeps across clips: ``pipe._engines``, a dict in LRU order
def engine_key(unet, tag, sample, cond, kw) -> tuple:
    """What a captured engine is good for: the loop (``tag``), the weights, the geometry, the guidance, the launches a graph holds."""
    key = (tag, unet._pack_gen, tuple(sample.shape), str(sample.device), tuple(cond["encoder_hidden_states"].shape), kw.get("b_unc"),
           kw.get("b_cond"), float(kw.get("guidance")), tuple(kw.get("dup_slots")), bool(kw.get("shared_stem", False)),
           _use_graphs(), pnp_utils.has_foreign_hooks(unet), id(unet), kw.get("lat_slots"),
           getattr(unet, "freeu", None))   # (a captured graph holds the FreeU launches of the setting it was captured under)
    if kw.get("stochastic") or kw.get("rescale"):
        # ... and the launches of its sampler options; with both off the key is the default engine's, unchanged
        key += (("sampler", bool(kw.get("stochastic")), float(kw.get("rescale") or 0.0)),)
    if kw.get("blend") is not None:
        # ... and the blend launch of a masked edit, on buffers of this mask geometry; without a mask the key is unchanged
        key += (("blend", tuple(kw["blend"][1].shape)),)
    return key


def cached_engine(pipe, tag, sample, cond, **kw) -> _StepEngine:
    """A step engine for this loop: a new one, or -- for the next clip of the same geometry in a multi-clip job -- the one captured for
    the previous clip, re-pointed at the new clip (``_StepEngine.rebind``): graph capture and its warm-up forward (~0.25 s per
    16 x 512^2 clip) are paid once per process instead of once per clip.  ANYV2V_ENGINE_CACHE=0 switches it off."""
    unet, engines = pipe.unet, pipe._engines
    if os.environ.get("ANYV2V_ENGINE_CACHE", "1") != "1" or getattr(unet, "frame_parallel", None) is not None:
        return _StepEngine(pipe, sample, cond, **kw)
    if not unet._packed:
        unet.pack()  # (weights loaded / moved since the last call: new packed tensors, engines of the old ones are stale)
    key = engine_key(unet, tag, sample, cond, kw)
    eng = engines.pop(key, None)
    if eng is None or not eng.rebind(sample, cond):
        eng = _StepEngine(pipe, sample, cond, **kw)
    engines[key] = eng  # most recently used last
    # Every engine pins a private graph pool holding a whole forward's activations (and a nested one for the source-free
    # steps), so the cache is small and evicts eagerly: one engine per loop kind (a new guidance value or geometry replaces
    # the old engine of that loop -- a slider in a long-lived front-end must not accumulate pools), at most
    # ANYV2V_ENGINE_CACHE_MAX (3 = inversion + CFG + PnP) overall; an evicted engine drops its graphs and returns the memory.
    evict = [k for k in engines if k[0] == tag and k != key]
    limit = max(1, int(os.environ.get("ANYV2V_ENGINE_CACHE_MAX", "3")))
    evict += [k for k in list(engines)[: max(0, len(engines) - len(evict) - limit)] if k not in evict]
    for k in evict:
        old = engines.pop(k)
        release_graphs(old.graphs)   # (parked, not destroyed, while another engine / thread is capturing: utils.release_graphs)
        if old.nosrc is not None:
            release_graphs(old.nosrc.graphs)
            old.nosrc = None
    if evict and sample.is_cuda:
        torch.cuda.empty_cache()
    return eng
