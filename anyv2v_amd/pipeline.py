"""``I2VGenXLPipeline`` with the reference's call surface (seam B5; ``i2vgen-xl/pipelines/pipeline_i2vgen_xl.py:133``):
``from_pretrained``, ``.to``, ``register_modules``, ``encode_vae_video`` (:565), ``invert`` (:1197), ``__call__``
(:652), ``sample_with_pnp`` (:892) -- driving the MI355X-native UNet.

The three denoising loops (inversion :1385-1433, PnP sampling :1131-1179, CFG sampling :839-874) are the hot path.
What changed relative to the reference, all exact:
  * the inversion trajectory stays in HBM (``LatentTrajectory``); ``ddim_latents_{t}.pt`` files are still written
    (background thread, after the loop) and still readable, but no step blocks on disk or H2D;
  * no per-step ``t.item()`` sync: timesteps / DDIM coefficients live in small device tables;
  * CFG combine + scheduler step + the two permutes are one kernel reading the UNet's channels-last output;
  * a whole step (UNet forward + CFG/DDIM step) is captured once per injection state into a HIP graph and replayed.
VAE / CLIP encoders are optional components: without them the pipeline takes precomputed
``prompt_embeds`` / ``image_embeddings`` / ``image_latents`` and returns latents.
"""
from __future__ import annotations

import logging
import os
from contextlib import nullcontext
from types import SimpleNamespace
from typing import Dict, Optional, Union

import torch

from . import pnp_utils
from .masked_edit import MaskedEditMixin, edit_mask_timestep  # noqa: F401  (``edit_mask_timestep`` stays importable from here)
from .schedulers import DDIMScheduler
from .step_engine import SourceFeatureCache, _StepEngine, _use_graphs, cached_engine, pnp_step_plan  # noqa: F401  (re-exported)
from .unet import I2VGenXLUNet, I2VGenXLUNetConfig
from .utils import LatentTrajectory, load_ddim_latents_at_t

logger = logging.getLogger(__name__)


class I2VGenXLPipelineOutput:
    def __init__(self, frames):
        self.frames = frames


class StableVideoDiffusionInversionPipelineOutput:
    def __init__(self, inverted_latents):
        self.inverted_latents = inverted_latents


def _vae_config(root):
    """``VAEConfig`` with the tile size (``sample_size``) of ``<root>/vae/config.json`` when the checkpoint has one, else None."""
    path = os.path.join(root, "vae", "config.json")
    if not os.path.isfile(path):
        return None
    import json

    from .vae import VAEConfig
    with open(path) as f:
        js = json.load(f)
    return VAEConfig(sample_size=int(js["sample_size"])) if "sample_size" in js else None


class I2VGenXLPipeline(MaskedEditMixin):
    def __init__(self, vae=None, text_encoder=None, tokenizer=None, image_encoder=None, feature_extractor=None,
                 unet: Optional[I2VGenXLUNet] = None, scheduler=None):
        self.vae, self.text_encoder, self.tokenizer = vae, text_encoder, tokenizer
        self.image_encoder, self.feature_extractor = image_encoder, feature_extractor
        self.unet, self.scheduler = unet, scheduler
        self.vae_scale_factor = 8
        self._guidance_scale = 1.0
        self._guidance_rescale = 0.0   # ``enable_guidance_rescale``
        self._masked_edit = None       # ``enable_masked_edit``: the mask and clean latent of the clip being edited
        self._device = torch.device("cpu")
        self._engines: Dict[tuple, _StepEngine] = {}  # step engines (static buffers + HIP graphs) kept across clips, LRU
        # pacing hooks of the clip pipeline (run_group_anyv2v): ``pace_record(i, n)`` is called when edit step i of n is about to be
        # enqueued, ``pace_wait(i, n)`` before inversion step i of n -- stream events, outside the captured graphs
        self.pace_record = self.pace_wait = None
        self.ws_slot = 0   # split-K scratch buffer of this pipeline's launches (``sibling``: a second stream needs its own)
        self.source_cache: Optional[SourceFeatureCache] = None   # set (``enable_source_cache``) by multi-edit jobs

    # ------------------------------------------------------------------ construction / plumbing
    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, torch_dtype=torch.float16, variant="fp16",
                        unet_config: Optional[I2VGenXLUNetConfig] = None, random_init_seed: Optional[int] = None, **kw):
        """Loads ``<path>/unet/diffusion_pytorch_model[.fp16].safetensors`` and ``<path>/vae/...`` (diffusers key naming) when
        present.
        There is no network here: for the hub id ``"ali-vilab/i2vgen-xl"`` without a local copy, random weights of
        the exact architecture are used when ``random_init_seed`` (or ANYV2V_RANDOM_INIT_SEED) is given."""
        if torch_dtype != torch.float16:
            raise ValueError("the HIP kernels compute in fp16 (fp32 accumulate); torch_dtype must be torch.float16")
        root = str(pretrained_model_name_or_path)
        cfg_json = os.path.join(root, "unet", "config.json")
        if unet_config is None and os.path.isfile(cfg_json):
            unet_config = I2VGenXLUNetConfig.from_json(cfg_json)
        unet = I2VGenXLUNet(unet_config)
        cands = [os.path.join(root, "unet", f"diffusion_pytorch_model.{variant}.safetensors"),
                 os.path.join(root, "unet", "diffusion_pytorch_model.safetensors")]
        path = next((c for c in cands if os.path.isfile(c)), None)
        if path is not None:
            from safetensors.torch import load_file
            unet.load_state_dict(load_file(path), strict=True)
        else:
            seed = random_init_seed
            if seed is None and os.environ.get("ANYV2V_RANDOM_INIT_SEED") is not None:
                seed = int(os.environ["ANYV2V_RANDOM_INIT_SEED"])
            if seed is None:
                raise FileNotFoundError(
                    f"no UNet weights under {root!r} (expected unet/diffusion_pytorch_model.{variant}.safetensors) and no "
                    "network; pass random_init_seed= (or ANYV2V_RANDOM_INIT_SEED) to run with random weights")
            unet._random_seed = seed
        scheduler = DDIMScheduler.from_pretrained(root, subfolder="scheduler")
        pipe = cls(unet=unet, scheduler=scheduler)
        # the VAE of the checkpoint, when a local copy exists: native AutoencoderKL on the HIP kernels (same key naming)
        vcands = [os.path.join(root, "vae", f"diffusion_pytorch_model.{variant}.safetensors"),
                  os.path.join(root, "vae", "diffusion_pytorch_model.safetensors")]
        vpath = next((c for c in vcands if os.path.isfile(c)), None)
        if vpath is not None:
            from safetensors.torch import load_file

            from .encoders import NativeVAE
            pipe.vae = NativeVAE(state_dict=load_file(vpath), cfg=_vae_config(root))
        if os.path.isdir(os.path.join(root, "text_encoder")):
            # CLIP towers of a local checkpoint on the HIP kernels (anyv2v_amd.clip)
            from .encoders import attach_native_clip_encoders
            attach_native_clip_encoders(pipe, root)
        return pipe

    def sibling(self, ws_slot: int = 1):
        """A second pipeline object around the SAME components (no weights copied) with its own scheduler slot, step engines,
        conditioning cache and scratch buffer: ``run_group_anyv2v`` edits clip k on one stream with it while this pipeline
        inverts clip k + 1 on another."""
        p = type(self)(vae=self.vae, text_encoder=self.text_encoder, tokenizer=self.tokenizer, image_encoder=self.image_encoder,
                       feature_extractor=self.feature_extractor, unet=self.unet, scheduler=self.scheduler)
        p._device, p.ws_slot = self._device, int(ws_slot)
        p._guidance_rescale = self._guidance_rescale
        return p

    def to(self, device):
        device = torch.device(device)
        self._device = device
        self.unet.to(device)
        seed = getattr(self.unet, "_random_seed", None)
        if seed is not None:
            init_random_weights_(self.unet, seed)
            self.unet._random_seed = None
        for m in (self.vae, self.text_encoder, self.image_encoder):
            if m is not None and hasattr(m, "to"):
                m.to(device)
        return self

    def register_modules(self, **kwargs):
        for k, v in kwargs.items():
            setattr(self, k, v)

    @property
    def device(self):
        return self._device

    @property
    def _execution_device(self):
        return self._device

    @property
    def guidance_scale(self):
        return self._guidance_scale

    @property
    def do_classifier_free_guidance(self):
        return self._guidance_scale > 1

    def progress_bar(self, iterable=None, total=None):
        return iterable

    def maybe_free_model_hooks(self):
        pass

    # ------------------------------------------------------------------ input checks (pipeline_i2vgen_xl.py:483-530)
    def check_inputs(self, prompt, image, height, width, negative_prompt=None, prompt_embeds=None,
                     negative_prompt_embeds=None):
        if height % 8 != 0 or width % 8 != 0:
            raise ValueError(f"`height` and `width` have to be divisible by 8 but are {height} and {width}.")
        if prompt is not None and prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `prompt`: {prompt} and `prompt_embeds`: {prompt_embeds}. Please make sure to"
                             " only forward one of the two.")
        elif prompt is None and prompt_embeds is None:
            raise ValueError("Provide either `prompt` or `prompt_embeds`. Cannot leave both `prompt` and `prompt_embeds` undefined.")
        elif prompt is not None and (not isinstance(prompt, str) and not isinstance(prompt, list)):
            raise ValueError(f"`prompt` has to be of type `str` or `list` but is {type(prompt)}")
        if negative_prompt is not None and negative_prompt_embeds is not None:
            raise ValueError(f"Cannot forward both `negative_prompt`: {negative_prompt} and `negative_prompt_embeds`:"
                             f" {negative_prompt_embeds}. Please make sure to only forward one of the two.")
        if prompt_embeds is not None and negative_prompt_embeds is not None:
            if prompt_embeds.shape != negative_prompt_embeds.shape:
                raise ValueError("`prompt_embeds` and `negative_prompt_embeds` must have the same shape when passed directly, but"
                                 f" got: `prompt_embeds` {prompt_embeds.shape} != `negative_prompt_embeds`"
                                 f" {negative_prompt_embeds.shape}.")

    # ------------------------------------------------------------------ encoders (optional components, F1)
    def _need(self, name):
        m = getattr(self, name)
        if m is None:
            raise RuntimeError(
                f"pipeline component `{name}` is not loaded (VAE/CLIP are outside the HIP hot path and no pretrained weights "
                "exist offline); pass the precomputed tensors instead (prompt_embeds / negative_prompt_embeds / "
                "image_embeddings / image_latents / latents, output_type='latent')")
        return m

    def encode_prompt(self, prompt, device, num_videos_per_prompt=1, negative_prompt=None, prompt_embeds=None,
                      negative_prompt_embeds=None, lora_scale=None, clip_skip=None):
        if prompt_embeds is None:
            enc, tok = self._need("text_encoder"), self._need("tokenizer")
            prompt_embeds = _clip_text(enc, tok, prompt, device, clip_skip)
        if self.do_classifier_free_guidance and negative_prompt_embeds is None:
            enc, tok = self._need("text_encoder"), self._need("tokenizer")
            n = negative_prompt if negative_prompt is not None else ""
            if isinstance(n, str):
                n = [n] * prompt_embeds.shape[0]
            negative_prompt_embeds = _clip_text(enc, tok, n, device, clip_skip)
        return prompt_embeds, negative_prompt_embeds

    def prepare_image_latents_from_first_frame_latent(self, first_latent, num_frames):
        """``prepare_image_latents`` (:532-562) after the VAE: first-frame latent + (F-1) frame-position planes."""
        il = first_latent.unsqueeze(2)  # [b,4,1,h,w]
        planes = [torch.ones_like(il[:, :, :1]) * ((i + 1) / (num_frames - 1)) for i in range(num_frames - 1)]
        if planes:
            il = torch.cat([il] + planes, dim=2)
        return il

    def prepare_image_latents(self, image, device, num_frames, num_videos_per_prompt=1):
        """``pipeline_i2vgen_xl.py:532-562``: a pre-processed first frame [1, 3, H, W] in [-1, 1] -> sampled, scaled VAE latent, the
        frame-position planes behind it, doubled under classifier-free guidance."""
        if num_videos_per_prompt not in (None, 1):
            raise ValueError("one clip per call (num_videos_per_prompt = 1)")
        first = self._need("vae").encode_pixels(image, device)
        il = self.prepare_image_latents_from_first_frame_latent(first, num_frames)
        return torch.cat([il] * 2) if self.do_classifier_free_guidance else il

    def prepare_extra_step_kwargs(self, generator, eta):
        """``:466-482``: ``eta`` / ``generator`` for a scheduler whose ``step`` takes them (the forward DDIM scheduler takes both, the
        inverse one neither)."""
        import inspect
        params = set(inspect.signature(self.scheduler.step).parameters)
        extra = {}
        if "eta" in params:
            extra["eta"] = eta
        if "generator" in params:
            extra["generator"] = generator
        return extra

    # memory savers of the reference pipeline (``:192-222``): decoding already runs ``decode_chunk_size`` frames at a time, and a 512^2
    # frame is far below anything that needs tiles on this device -- both switches are accepted and change nothing (the reference's
    # tiled decode blends tile seams, i.e. differs from its own untiled output; this build always gives the untiled one)
    def enable_vae_slicing(self):
        self._vae_slicing = True

    def disable_vae_slicing(self):
        self._vae_slicing = False

    def enable_vae_tiling(self):
        """``pipeline_i2vgen_xl.py:208-214``: frames over the VAE's ``sample_size`` are encoded / decoded in blended tiles
        (``AutoencoderKL.enable_tiling``).  A VAE without tiling (``SyntheticVAE``, none loaded) accepts the call and decodes whole."""
        if hasattr(self.vae, "enable_tiling"):
            self.vae.enable_tiling()
        else:
            logger.warning("enable_vae_tiling: frames are decoded whole on this device; the output equals the reference's UNTILED decode")
        self._vae_tiling = True

    def disable_vae_tiling(self):
        if hasattr(self.vae, "disable_tiling"):
            self.vae.disable_tiling()
        self._vae_tiling = False

    def auto_vae_tiling(self, height, width):
        """Turn tiling on when a ``height`` x ``width`` frame exceeds one tile of a VAE that can tile AND cannot be encoded / decoded
        whole (the mid-block attention takes at most 8192 latent tokens): jobs that could not run now run, the others keep their
        untiled output (a tiled result differs from the untiled one by design).  ``enable_vae_tiling`` itself has no such condition."""
        ts = getattr(self.vae, "tile_sample_size", None)
        if ts is None or not height or not width or self.vae.use_tiling:
            return
        tokens = (int(height) // self.vae_scale_factor) * (int(width) // self.vae_scale_factor)
        if max(int(height), int(width)) > ts and tokens > 8192:
            self.enable_vae_tiling()

    def enable_freeu(self, s1, s2, b1, b2):
        """``:623-648``: forwarded to the UNet (``I2VGenXLUNet.enable_freeu``: FreeU re-weights the decoder's backbone / skip features
        in front of the concats of ``up_blocks[0]`` / ``[1]``).  The four numbers are part of the step engines' cache key, so HIP graphs
        captured under another setting are not replayed, and the multi-edit source-feature cache is dropped: what it recorded depends
        on them.  ConsistI2V / SEINE have no FreeU in the reference and none here."""
        if self.unet is None or not hasattr(self.unet, "enable_freeu"):
            raise NotImplementedError("enable_freeu needs a UNet: this pipeline has none loaded (or one without FreeU support)")
        self.unet.enable_freeu(s1, s2, b1, b2)   # (refuses frame-parallel clips)
        self._freeu_changed()

    def disable_freeu(self):
        if self.unet is not None and hasattr(self.unet, "disable_freeu"):
            self.unet.disable_freeu()
            self._freeu_changed()

    def _freeu_changed(self):
        if self.source_cache is not None:
            self.source_cache.bind(None)   # recorded source features were computed under the other setting

    def prepare_frames(self, frames, height, width, fit="crop", x_offset=0.0, y_offset=0.0, resample="lanczos"):
        """Source frames of any one size (a list of PIL images or a uint8 [F, H, W, 3] tensor) -> uint8 [F, height, width, 3] on this
        pipeline's device: cover-resize and crop (``fit="crop"``, offsets in [-1, 1]) or plain resize (``"stretch"``), Pillow's
        ``resize(...).crop(...)`` byte for byte (``anyv2v_amd.prepare``).  ``encode_vae_video`` takes the result as it is."""
        from . import prepare
        return prepare.prepare_frames(frames, height, width, fit, x_offset, y_offset, resample, device=self._execution_device)

    def prepare_mask(self, mask, height, width, fit="crop", x_offset=0.0, y_offset=0.0):
        """An edit mask at the source frames' size, [1 or F, H, W] -> uint8 0 / 255 [1 or F, height, width] through the same geometry
        (``anyv2v_amd.prepare.prepare_mask``)."""
        from . import prepare
        return prepare.prepare_mask(mask, height, width, fit, x_offset, y_offset, device=self._execution_device)

    def restore_frames(self, edited, source_frames, fit="crop", x_offset=0.0, y_offset=0.0, resample="lanczos", alpha=None):
        """The way back from ``prepare_frames``: ``edited`` (uint8 [F, h, w, 3] or PIL images at the working size) resized into the footprint
        it was prepared from and pasted over ``source_frames`` at their own size -> uint8 [F, sh, sw, 3] on this pipeline's device, Pillow's
        ``paste(resize(.., box), xy, mask)`` byte for byte; ``alpha``: None or fp32 [1 or F, h, w] in [0, 1] (``composite_alpha``), where it
        is 0 the source's bytes stay (``anyv2v_amd.prepare.restore_frames``)."""
        from . import prepare
        if getattr(self.unet, "frame_parallel", None) is not None:
            raise NotImplementedError("restore on a frame-parallel clip: the composite it follows is refused there")
        return prepare.restore_frames(edited, source_frames, fit, x_offset, y_offset, resample, alpha, device=self._execution_device)

    def restore_frames_detail(self, edited, source_frames, prepared=None, fit="crop", x_offset=0.0, y_offset=0.0, resample="lanczos", alpha=None,
                              source_resample="lanczos", gate_lo=8, gate_hi=32, gate_radius=2):
        """``restore_frames`` with the source's fine detail carried into the upscaled edit wherever the edit stayed close to ``prepared``,
        the frames the model saw (None: ``prepare_frames`` of the source with ``source_resample``); an edit that changes nothing gives the
        source back byte for byte (``anyv2v_amd.prepare.restore_frames_detail``).  The gate's defaults are not validated on real edits."""
        from . import prepare
        if getattr(self.unet, "frame_parallel", None) is not None:
            raise NotImplementedError("restore on a frame-parallel clip: the composite it follows is refused there")
        return prepare.restore_frames_detail(edited, source_frames, prepared, fit, x_offset, y_offset, resample, alpha, source_resample, gate_lo,
                                             gate_hi, gate_radius, device=self._execution_device)

    def encode_vae_video(self, video, device, height=576, width=1024):
        vae = self._need("vae")
        return vae.encode_video(video, device, height, width)

    def decode_latents(self, latents, decode_chunk_size=None):
        vae = self._need("vae")
        fp = getattr(self.unet, "frame_parallel", None)
        if fp is not None and latents.shape[2] % fp.world == 0:
            # frame-parallel clip: frames decode independently (``decode_chunk_size=1`` in the reference) -- every rank
            # decodes its own frames, one all_gather of the decoded frames (12 MiB per 16 frames at 512^2)
            f0, f1 = fp.frames(latents.shape[2])
            mine = vae.decode_video(latents[:, :, f0:f1].contiguous(), decode_chunk_size)
            return fp.gather_video(mine)
        return vae.decode_video(latents, decode_chunk_size)

    def prepare_latents(self, batch_size, num_channels_latents, num_frames, height, width, dtype, device, generator,
                        latents=None):
        shape = (batch_size, num_channels_latents, num_frames, height // self.vae_scale_factor,
                 width // self.vae_scale_factor)
        if latents is None:
            latents = torch.randn(shape, generator=generator, dtype=torch.float32).to(device=device, dtype=dtype)
        else:
            latents = latents.to(device)
        return latents * self.scheduler.init_noise_sigma

    @staticmethod
    def _single_clip(prompt_embeds, num_videos_per_prompt):
        """The loops drive ONE clip per call (``nb`` batch slots = its CFG / PnP branches).  The reference computes a real
        batch for a list prompt; here that would silently combine the negative branch of prompt 0 with the positive branch
        of prompt 1, so it is refused."""
        if num_videos_per_prompt not in (None, 1):
            raise ValueError(f"num_videos_per_prompt={num_videos_per_prompt} is not supported: one clip per call (shard clips "
                             "over processes / GPUs instead, anyv2v_amd.parallel)")
        if prompt_embeds.shape[0] != 1:
            raise ValueError(f"got a batch of {prompt_embeds.shape[0]} prompts: one clip per call (the batch dimension holds the "
                             "CFG / PnP branches of that clip)")

    def _forward_sampler_options(self, eta, cross_attention_kwargs):
        """``__call__`` / ``sample_with_pnp`` (``pipeline_i2vgen_xl.py:798,868`` / ``:1095,1173``): ``eta`` goes to ``scheduler.step`` when
        that takes it -- the forward DDIM scheduler does (stochastic DDIM), the inverse one does not (``invert`` drops it, as here).
        This is the check of the DEFAULT step engine, whose fused guidance + DDIM step is the deterministic one: an ``eta`` that reaches it
        would be silently ignored and change the sample, so it is refused.  ``_sampler_options`` routes ``eta`` > 0 to a stochastic engine
        before it gets here."""
        if eta not in (None, 0, 0.0) and isinstance(self.scheduler, DDIMScheduler):
            raise ValueError(f"eta={eta}: the step engines run deterministic DDIM (eta = 0) only")
        if cross_attention_kwargs:
            raise ValueError("cross_attention_kwargs (LoRA scale, ...) are not supported by the native attention processors")

    def enable_guidance_rescale(self, guidance_rescale: float):
        """Lin et al.'s guidance rescale (``rescale_noise_cfg``, ``consisti2v/consisti2v/pipelines/pipeline_video_editing.py:50-61``) in
        ``__call__`` and ``sample_with_pnp``: the guided prediction is scaled by phi std(text) / std(guided) + (1 - phi) before the
        scheduler step (inside the step engine's fused kernel).  A setter, not a call argument: the reference's I2VGen-XL signatures have
        none.  0 switches it off; ``invert`` and ``invert_clips`` never rescale."""
        phi = float(guidance_rescale)
        if not 0.0 <= phi <= 1.0:   # (also refuses NaN)
            raise ValueError(f"guidance_rescale={guidance_rescale}: 0 <= guidance_rescale <= 1")
        if phi > 0.0 and getattr(self.unet, "frame_parallel", None) is not None:
            raise NotImplementedError("guidance rescale on a frame-parallel clip: the statistics span all frames and would need a collective")
        self._guidance_rescale = phi

    def disable_guidance_rescale(self):
        self._guidance_rescale = 0.0

    def _sampler_options(self, eta, cross_attention_kwargs):
        """-> (stochastic, eta, phi) for the step engines of ``__call__`` / ``sample_with_pnp``.  ``eta`` counts when the scheduler is the
        forward ``DDIMScheduler`` (as ``prepare_extra_step_kwargs``: the inverse scheduler's ``step`` takes none); 0 <= eta <= 1."""
        phi = float(getattr(self, "_guidance_rescale", 0.0))
        forward = isinstance(self.scheduler, DDIMScheduler)
        if forward and eta is not None and not 0.0 <= float(eta) <= 1.0:
            raise ValueError(f"eta={eta}: stochastic DDIM takes 0 <= eta <= 1")
        stochastic = bool(forward and eta is not None and float(eta) > 0.0)
        if phi > 0.0 and not forward:
            raise NotImplementedError(f"guidance rescale runs in the forward DDIM step engines, not with {type(self.scheduler).__name__}")
        if (stochastic or phi > 0.0) and getattr(self.unet, "frame_parallel", None) is not None:
            raise NotImplementedError(f"eta={eta} / guidance_rescale={phi} on a frame-parallel clip: the rescale statistics span all frames "
                                      "(they would need a collective) and every rank would have to draw the same noise")
        self._forward_sampler_options(0.0 if stochastic else eta, cross_attention_kwargs)
        return stochastic, (float(eta) if stochastic else 0.0), phi

    def _variance_noise(self, stochastic, like, generator):
        """One draw per step, where diffusers' ``DDIMScheduler.step`` draws its ``variance_noise`` (``randn_tensor`` with the shape and
        dtype of the guided prediction, from the caller's ``generator``), handed to the engine's static buffer OUTSIDE the captured graph:
        a draw recorded inside a graph -- or a buffer filled once -- would replay the same noise at every step."""
        return self.scheduler.draw_noise(like, generator) if stochastic else None

    # ------------------------------------------------------------------ conditioning assembly
    def _conditioning(self, prompt, image, height, width, num_frames, negative_prompt, prompt_embeds,
                      negative_prompt_embeds, target_fps, clip_skip, image_embeddings, image_latents):
        """Returns per-branch lists: cond branch tensors and (when CFG) uncond ones, following :1014-1101."""
        device = self._execution_device
        prompt_embeds, negative_prompt_embeds = self.encode_prompt(
            prompt, device, 1, negative_prompt, prompt_embeds=prompt_embeds,
            negative_prompt_embeds=negative_prompt_embeds, clip_skip=clip_skip)
        if image_embeddings is None:
            image_embeddings = _clip_image(self._need("image_encoder"), self._need("feature_extractor"), image, width, device)
        if image_latents is None:
            first = self._need("vae").encode_image(image, device, height, width)
            image_latents = self.prepare_image_latents_from_first_frame_latent(first, num_frames)
        return (prompt_embeds.to(device, torch.float16), None if negative_prompt_embeds is None else
                negative_prompt_embeds.to(device, torch.float16), image_embeddings.to(device, torch.float16),
                image_latents.to(device, torch.float16))

    def _source_conditioning(self, ddim_inv_prompt, ddim_inv_1st_frame, height, width, num_frames, clip_skip, ddim_inv_prompt_embeds=None,
                             ddim_inv_image_embeddings=None, ddim_inv_image_latents=None):
        """The source (ddim inversion) branch of ``sample_with_pnp``: its own prompt, first frame, positive image embedding (:1027-1091)
        -> (prompt embedding, image embedding, image latents), fp16 on the device."""
        device = self._execution_device
        if ddim_inv_prompt_embeds is None:
            ddim_inv_prompt_embeds = _clip_text(self._need("text_encoder"), self._need("tokenizer"), ddim_inv_prompt,
                                                device, clip_skip)
        if ddim_inv_image_embeddings is None:
            ddim_inv_image_embeddings = _clip_image(self._need("image_encoder"), self._need("feature_extractor"),
                                                    ddim_inv_1st_frame, width, device)
        if ddim_inv_image_latents is None:
            first = self._need("vae").encode_image(ddim_inv_1st_frame, device, height, width)
            ddim_inv_image_latents = self.prepare_image_latents_from_first_frame_latent(first, num_frames)
        return (ddim_inv_prompt_embeds.to(device, torch.float16), ddim_inv_image_embeddings.to(device, torch.float16),
                ddim_inv_image_latents.to(device, torch.float16))

    def enable_source_cache(self, on: bool = True):
        """Several edits of one clip (a group job, the front-end called repeatedly): keep the source branch's injected features of
        the clip in HBM across ``sample_with_pnp`` calls -- ``SourceFeatureCache``.  Off by default: a single edit gains nothing."""
        self.source_cache = SourceFeatureCache() if on else None
        return self.source_cache

    def _step_tables(self, ts, nb, **coef_kw):
        """What the loops share.  -> (timestep rows [n, nb], DDIM coefficient rows [n, 4 or 8]) on the device: a step copies row i, no host sync."""
        t_table = torch.tensor(ts, dtype=torch.float32, device=self._execution_device)[:, None].expand(-1, nb).contiguous()
        return t_table, self.scheduler.coefficient_table(ts, self._execution_device, **coef_kw)

    def _loop_setup(self, kind, prompt, image, height, width, target_fps, num_frames, num_inference_steps, guidance_scale, negative_prompt,
                    eta, num_videos_per_prompt, generator, latents, prompt_embeds, negative_prompt_embeds, cross_attention_kwargs, clip_skip,
                    image_embeddings, image_latents, t_idx=None, source=None):
        """``invert`` ("inv"), ``__call__`` ("cfg") and ``sample_with_pnp`` ("pnp") in front of the step engine: input checks, conditioning,
        the branch batch -- [negative, positive] under classifier-free guidance (:1329-1337; zero negative image embedding, :437-439), the
        source branch (``source``: the ``ddim_inv_*`` arguments) in front of it in a PnP edit (:1044,1093-1094) --, the timesteps from
        ``t_idx`` on (:813,1105; the inversion runs them all and takes no sampler options), latents, step tables, engine keywords."""
        height = height or self.unet.config.sample_size * self.vae_scale_factor
        width = width or self.unet.config.sample_size * self.vae_scale_factor
        self.check_inputs(prompt, image, height, width, negative_prompt, prompt_embeds, negative_prompt_embeds)
        if kind != "pnp":
            self._refuse_masked_edit("invert" if kind == "inv" else "__call__")
        elif isinstance(prompt, list):
            assert len(source[0]) == len(prompt)  # :1000
        device = self._execution_device
        self._guidance_scale = guidance_scale
        pe, npe, ie, il = self._conditioning(prompt, image, height, width, num_frames, negative_prompt, prompt_embeds,
                                             negative_prompt_embeds, target_fps, clip_skip, image_embeddings, image_latents)
        self._single_clip(pe, num_videos_per_prompt)
        stochastic, eta, phi = self._sampler_options(eta, cross_attention_kwargs) if kind != "inv" else (False, 0.0, 0.0)
        opts = dict(stochastic=stochastic, rescale=phi) if (stochastic or phi > 0.0) else {}
        cfg_on = bool(self.do_classifier_free_guidance)
        branches, source_cond = [(pe, ie, il)], None
        if cfg_on:
            branches.insert(0, (npe, torch.zeros_like(ie), il))
        if kind == "pnp":
            source_cond = self._source_conditioning(source[0], source[1], height, width, num_frames, clip_skip, *source[2:])
            branches.insert(0, source_cond)
        else:
            pnp_utils.clear_time(self)  # inversion (stage 1 of the reference) and plain CFG sampling (DDIM reconstruction) run hook-free
        ehs, ie_all, il_all = (torch.cat(x) if len(x) > 1 else x[0] for x in zip(*branches))
        nb = ehs.shape[0]
        self.scheduler.set_timesteps(num_inference_steps, device=device)
        if kind != "inv":
            self.scheduler.timesteps = self.scheduler.timesteps[t_idx:]
        ts = [int(t) for t in self.scheduler.timesteps.tolist()]
        latents = self.prepare_latents(1, self.unet.config.in_channels, num_frames, height, width, torch.float16, device,
                                       generator, latents).to(torch.float16)
        sample = latents.repeat(nb, 1, 1, 1, 1).contiguous()
        cond = dict(encoder_hidden_states=ehs.contiguous(), fps=torch.tensor([target_fps] * nb, device=device),
                    image_latents=il_all.contiguous(), image_embeddings=ie_all.contiguous())
        src = 1 if kind == "pnp" else 0   # slots in front of the CFG pair
        engine_kw = dict(b_unc=src if cfg_on else -1, b_cond=nb - 1, guidance=guidance_scale, dup_slots=range(src, nb - 1),
                         shared_stem=cfg_on and kind != "inv", **opts)
        t_table, coef_table = self._step_tables(ts, nb, **(dict(eta=eta, phi=phi, n=latents.numel()) if opts else {}))
        return SimpleNamespace(nb=nb, ts=ts, sample=sample, cond=cond, t_table=t_table, coef_table=coef_table, engine_kw=engine_kw,
                               latents=latents, height=height, width=width, cfg_on=cfg_on, stochastic=stochastic, source_cond=source_cond)

    # ------------------------------------------------------------------ A1: DDIM inversion (:1197-1451)
    @torch.no_grad()
    def invert(self, prompt=None, image=None, height: Optional[int] = 704, width: Optional[int] = 1280,
               target_fps: Optional[int] = 16, num_frames: int = 16, num_inference_steps: int = 50,
               guidance_scale: float = 9.0, negative_prompt=None, eta: float = 0.0, num_videos_per_prompt: Optional[int] = 1,
               decode_chunk_size: Optional[int] = 1, generator=None, latents: Optional[torch.Tensor] = None,
               prompt_embeds=None, negative_prompt_embeds=None, output_type: Optional[str] = "pil",
               return_dict: bool = True, cross_attention_kwargs=None, clip_skip: Optional[int] = 1,
               output_dir: Optional[str] = None, image_embeddings=None, image_latents=None,
               return_trajectory: bool = False, background_save: bool = False):
        lp = self._loop_setup("inv", prompt, image, height, width, target_fps, num_frames, num_inference_steps, guidance_scale,
                              negative_prompt, eta, num_videos_per_prompt, generator, latents, prompt_embeds, negative_prompt_embeds,
                              cross_attention_kwargs, clip_skip, image_embeddings, image_latents)
        nb, ts = lp.nb, lp.ts
        eng = cached_engine(self, "inv", lp.sample, lp.cond, **lp.engine_kw)
        sample = eng.sample  # (a cached engine keeps its own static buffer; the latents were copied into it)
        traj = LatentTrajectory()
        for i, t in enumerate(ts):
            if self.pace_wait is not None:
                self.pace_wait(i, len(ts))
            eng.step(lp.t_table[i], lp.coef_table[i], key=("inv",))
            traj[t] = sample[nb - 1:nb].clone()
        if output_dir is not None:
            # ddim_latents_{t}.pt, reference format.  Complete when invert() returns (as in the reference, which writes
            # inside the loop) unless the caller opts into the background writer (the CLI runner does; every reader in
            # anyv2v_amd.utils joins it first)
            traj.save(output_dir, background=background_save)
            logger.info(f"saving noisy latents for {len(ts)} timesteps to {output_dir}")
        self._last_trajectory = traj
        inverted = torch.stack([traj[t] for t in reversed(ts)], 1)  # [1, n, 4, F, h, w] (:1436)
        if return_trajectory:
            return traj
        if not return_dict:
            return inverted
        return StableVideoDiffusionInversionPipelineOutput(inverted_latents=inverted)

    @torch.no_grad()
    def invert_clips(self, clips, height: int, width: int, num_frames: int = 16, num_inference_steps: int = 50, target_fps: int = 16,
                     clip_skip: Optional[int] = 1, output_dirs=None, background_save: bool = False):
        """Several clips inverted in ONE batch (guidance 1, the inversion configuration of the reference's runner): ``clips`` = list of
        dicts ``prompt``, ``image`` (first frame), ``latents`` [1, 4, F, h, w] (``encode_vae_video``), optionally ``negative_prompt``.
        The UNet forward runs over B = len(clips) rows -- each row its own clip with its own conditioning --, so every weight is read
        once per step for all of them and the low-resolution launches carry B times the rows: an inversion-bound job (the template's
        500 steps) gains what a B = 1 launch loses against a B = 3 one.  Returns one ``LatentTrajectory`` per clip; the numbers
        differ from ``invert`` at rounding level (other launch plans at other row counts), not bit for bit."""
        self._refuse_masked_edit("invert_clips")
        device = self._execution_device
        self._guidance_scale = 1.0
        pnp_utils.clear_time(self)
        n = len(clips)
        pes, ies, ils, lats = [], [], [], []
        for c in clips:
            pe, _npe, ie, il = self._conditioning(c.get("prompt", ""), c["image"], height, width, num_frames, c.get("negative_prompt"), None, None,
                                                  target_fps, clip_skip, None, None)
            self._single_clip(pe, 1)
            pes.append(pe)
            ies.append(ie)
            ils.append(il)
            lats.append(self.prepare_latents(1, self.unet.config.in_channels, num_frames, height, width, torch.float16, device, None,
                                             c["latents"]).to(torch.float16))
        sample = torch.cat(lats).contiguous()
        cond = dict(encoder_hidden_states=torch.cat(pes).contiguous(), fps=torch.tensor([target_fps] * n, device=device),
                    image_latents=torch.cat(ils).contiguous(), image_embeddings=torch.cat(ies).contiguous())
        self.scheduler.set_timesteps(num_inference_steps, device=device)
        ts = [int(t) for t in self.scheduler.timesteps.tolist()]
        eng = cached_engine(self, f"inv{n}", sample, cond, b_unc=-1, b_cond=n - 1, guidance=1.0, dup_slots=(), lat_slots=tuple(range(n)))
        sample = eng.sample
        t_table, coef_table = self._step_tables(ts, n)
        trajs = [LatentTrajectory() for _ in range(n)]
        for i, t in enumerate(ts):
            eng.step(t_table[i], coef_table[i], key=("inv",))
            for k in range(n):
                trajs[k][t] = sample[k:k + 1].clone()
        if output_dirs is not None:
            for tr, d in zip(trajs, output_dirs):
                if d is not None:
                    tr.save(d, background=background_save)
        return trajs

    # ------------------------------------------------------------------ A3: plain CFG sampling (:652-888)
    @torch.no_grad()
    def __call__(self, prompt=None, image=None, height: Optional[int] = 704, width: Optional[int] = 1280,
                 target_fps: Optional[int] = 16, num_frames: int = 16, num_inference_steps: int = 50,
                 guidance_scale: float = 9.0, negative_prompt=None, eta: float = 0.0, num_videos_per_prompt: Optional[int] = 1,
                 decode_chunk_size: Optional[int] = 1, generator=None, latents: Optional[torch.Tensor] = None,
                 prompt_embeds=None, negative_prompt_embeds=None, output_type: Optional[str] = "pil",
                 return_dict: bool = True, cross_attention_kwargs=None, clip_skip: Optional[int] = 1,
                 ddim_init_latents_t_idx: Optional[int] = 1, image_embeddings=None, image_latents=None,
                 latents_trace: Optional[dict] = None):
        """``latents_trace``: optional dict, filled with t -> latents after the step at t (drift reports; not a reference
        argument)."""
        lp = self._loop_setup("cfg", prompt, image, height, width, target_fps, num_frames, num_inference_steps, guidance_scale,
                              negative_prompt, eta, num_videos_per_prompt, generator, latents, prompt_embeds, negative_prompt_embeds,
                              cross_attention_kwargs, clip_skip, image_embeddings, image_latents, t_idx=ddim_init_latents_t_idx)
        nb = lp.nb
        eng = cached_engine(self, "cfg", lp.sample, lp.cond, **lp.engine_kw)
        sample = eng.sample
        for i, t in enumerate(lp.ts):
            eng.step(lp.t_table[i], lp.coef_table[i], key=("cfg",), noise=self._variance_noise(lp.stochastic, sample[nb - 1:nb], generator))
            if latents_trace is not None:
                latents_trace[t] = sample[nb - 1:nb].clone()
        return self._finish(sample[nb - 1:nb].clone(), output_type, decode_chunk_size, return_dict)

    # ------------------------------------------------------------------ A2: PnP edit (:892-1193)
    @torch.no_grad()
    def sample_with_pnp(self, prompt=None, image=None, height: Optional[int] = 704, width: Optional[int] = 1280,
                        target_fps: Optional[int] = 16, num_frames: int = 16, num_inference_steps: int = 50,
                        guidance_scale: float = 9.0, negative_prompt=None, eta: float = 0.0,
                        num_videos_per_prompt: Optional[int] = 1, decode_chunk_size: Optional[int] = 1, generator=None,
                        latents: Optional[torch.Tensor] = None, prompt_embeds=None, negative_prompt_embeds=None,
                        output_type: Optional[str] = "pil", return_dict: bool = True, cross_attention_kwargs=None,
                        clip_skip: Optional[int] = 1, ddim_init_latents_t_idx: Optional[int] = 1,
                        ddim_inv_latents_path: Union[str, LatentTrajectory, None] = None, ddim_inv_prompt=None,
                        ddim_inv_1st_frame=None, image_embeddings=None, image_latents=None,
                        ddim_inv_prompt_embeds=None, ddim_inv_image_embeddings=None, ddim_inv_image_latents=None,
                        latents_trace: Optional[dict] = None):
        lp = self._loop_setup("pnp", prompt, image, height, width, target_fps, num_frames, num_inference_steps, guidance_scale,
                              negative_prompt, eta, num_videos_per_prompt, generator, latents, prompt_embeds, negative_prompt_embeds,
                              cross_attention_kwargs, clip_skip, image_embeddings, image_latents, t_idx=ddim_init_latents_t_idx,
                              source=(ddim_inv_prompt, ddim_inv_1st_frame, ddim_inv_prompt_embeds, ddim_inv_image_embeddings,
                                      ddim_inv_image_latents))
        nb, ts, device = lp.nb, lp.ts, self._execution_device
        # masked edit (``enable_masked_edit``): the latent mask of this clip and the buffer of the per-step partner; one more engine option
        masked = self._masked_edit_buffers(lp.height, lp.width, num_frames, lp.latents)
        engine_kw = lp.engine_kw if masked is None else dict(lp.engine_kw, blend=masked[:2])
        # the source branch's prediction is never read (:1136,1160-1162): its forward may stop behind the last hook site (exact)
        drop_tail = lp.cfg_on and nb == 3 and os.environ.get("ANYV2V_DROP_SRC_TAIL", "1") == "1"
        eng = cached_engine(self, "pnp-droptail" if drop_tail else "pnp", lp.sample, lp.cond, drop_src_tail=drop_tail, **engine_kw)
        sample = eng.sample
        if masked is not None and eng.blend[1] is not masked[1]:
            # a cached engine: its graphs were captured on ITS buffers -- this clip's latent mask goes into them
            eng.blend[1].copy_(masked[1])
        # source trajectory resident in HBM (in-memory hand-off from invert(), or read once from the reference's files)
        in_memory = isinstance(ddim_inv_latents_path, LatentTrajectory)
        traj = ddim_inv_latents_path if in_memory else LatentTrajectory.load(ddim_inv_latents_path, device=device, timesteps=ts)
        # Exact work elimination (SURVEY A.5 probe "branches 1,2 of a B=3 forward equal a B=2 forward"): on a step outside every
        # injection schedule nothing reads the source branch, so it runs on the [negative, editing] slots only -- the engine's twin
        skip_src = lp.cfg_on and nb == 3 and os.environ.get("ANYV2V_SRC_SKIP", "1") == "1"
        twin = None   # (``bind_nosrc``: once per call, at the first step that needs it)
        # multi-edit job: record / replay what the injected sites read from the source branch (SourceFeatureCache).  The sampler options
        # leave it valid: that branch is fed from the inversion trajectory and never sees the edit latent, its noise or its prediction
        cache = self.source_cache if (skip_src and not pnp_utils.has_foreign_hooks(self.unet)
                                      and getattr(self.unet, "frame_parallel", None) is None) else None
        if cache is not None:
            traj_id = ("object", traj.serial) if in_memory else ("files", os.path.abspath(str(ddim_inv_latents_path)))
            cache.begin_run(self, eng, traj_id, ts, load_ddim_latents_at_t(ts[0], traj), lp.source_cond, target_fps, lp.latents.shape)
        for i, t in enumerate(ts):
            if self.pace_record is not None:
                self.pace_record(i, len(ts))
            pnp_utils.register_time(self, t)  # host-side only: python int, no device sync (:1143)
            state = pnp_utils.injection_state(self)
            noise = self._variance_noise(lp.stochastic, sample[nb - 1:nb], generator)   # one draw per step, whichever engine runs it
            # masked edit: after this step the edit latent sits at level ts[i + 1] -- its partner is the source at that level, the clean
            # latent after the last step.  Copied into the static buffer outside the graph, whichever engine runs the step
            extra = {} if masked is None else dict(partner=(
                load_ddim_latents_at_t(ts[i + 1], traj).to(device=device, dtype=torch.float16) if i + 1 < len(ts) else masked[2]))
            kind, key = pnp_step_plan(nb, skip_src, state, None if cache is None else cache.has(t, state))
            if kind in ("nosrc", "replay"):   # [negative, editing] only
                twin = twin or eng.bind_nosrc()
                step_eng, t_row = twin, lp.t_table[i, 1:]
            else:
                sample[0].copy_(load_ddim_latents_at_t(t, traj).to(device=device, dtype=torch.float16)[0], non_blocking=True)
                step_eng, t_row = eng, lp.t_table[i]
            with (cache.step_io(eng, kind, t, state) if kind in ("record", "replay") else nullcontext()):
                step_eng.step(t_row, lp.coef_table[i], key=key, noise=noise, **extra)
            if latents_trace is not None:
                latents_trace[t] = sample[nb - 1:nb].clone()
        return self._finish(sample[nb - 1:nb].clone(), output_type, decode_chunk_size, return_dict)

    def _finish(self, latents, output_type, decode_chunk_size, return_dict):
        if output_type == "latent":
            return I2VGenXLPipelineOutput(frames=latents)
        if output_type not in ("pil", "np", "pt"):
            raise ValueError(f"{output_type} does not exist. Please choose one of ['np', 'pt', 'pil]")     # (``tensor2vid``, :94-95)
        video = self.decode_latents(latents, decode_chunk_size=decode_chunk_size)          # [1, 3, F, H, W] in [-1, 1]
        frames = tensor2vid(video, self._need("vae"), output_type)      # (the runners index ``.frames[0]``, ``run_group_ddim_inversion.py:77``)
        if not return_dict:
            return (frames,)
        return I2VGenXLPipelineOutput(frames=frames)


def tensor2vid(video: torch.Tensor, processor=None, output_type: str = "np"):
    """``pipeline_i2vgen_xl.py:79-97`` over ``VaeImageProcessor.postprocess``: [b, 3, f, H, W] in [-1, 1] -> "pil": one list of PIL frames
    per video ((x / 2 + 0.5) * 255 rounded); "pt": [b, f, 3, H, W] in [0, 1]; "np": the same as float32 numpy [b, f, H, W, 3].
    ``processor``: anything with ``to_pil(video[1, 3, f, H, W])`` (the VAE adapters quantise where the tensor lives) or None."""
    if output_type == "pil":
        def one(v):
            if processor is not None and hasattr(processor, "to_pil"):
                return processor.to_pil(v)
            x = ((v[0].permute(1, 2, 3, 0).float() + 1.0) * 127.5).round().clamp(0, 255).to(torch.uint8).cpu().numpy()
            from PIL import Image
            return [Image.fromarray(fr) for fr in x]
        return [one(video[b:b + 1]) for b in range(video.shape[0])]
    if output_type not in ("np", "pt"):
        raise ValueError(f"{output_type} does not exist. Please choose one of ['np', 'pt', 'pil]")
    frames = (video.float() / 2 + 0.5).clamp(0, 1).permute(0, 2, 1, 3, 4)
    return frames.permute(0, 1, 3, 4, 2).cpu().numpy() if output_type == "np" else frames


# ---------------------------------------------------------------------------------------------------------------
def init_random_weights_(unet: I2VGenXLUNet, seed: int):
    """Random weights of the exact architecture, generated on the device (no pretrained weights offline).
    N(0, 1/fan_in) matrices, N(0, 0.02) biases, N(1, 0.05) norm gains -- same law as oracle.random_state_dict."""
    g = torch.Generator(device=unet.device).manual_seed(seed)
    for name, p in unet.named_parameters():
        shp = p.shape
        if name.endswith(".bias"):
            t = torch.randn(shp, generator=g, device=p.device) * 0.02
        elif p.dim() == 1:
            t = 1.0 + torch.randn(shp, generator=g, device=p.device) * 0.05
        else:
            fan_in = 1
            for d in shp[1:]:
                fan_in *= d
            t = torch.randn(shp, generator=g, device=p.device) / (fan_in ** 0.5)
        p.data.copy_(t.to(torch.float16))
    unet._packed = False


def _clip_text(text_encoder, tokenizer, prompt, device, clip_skip):
    """``encode_prompt`` (:224-409) through the component interface of ``anyv2v_amd.encoders``."""
    if isinstance(prompt, str):
        prompt = [prompt]
    return text_encoder.encode(prompt, device, clip_skip)


def _clip_image(image_encoder, feature_extractor, image, width, device):
    """``_encode_image`` (:411-441) on the centre-cropped, 224x224 bilinear-resized frame (:1051-1055)."""
    return image_encoder.encode(image, width, device)
