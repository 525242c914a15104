"""MI355X-native I2VGen-XL 3-D UNet: the module tree / state-dict keys of diffusers-0.26.3 ``I2VGenXLUNet``
(what the reference imports at ``i2vgen-xl/pipelines/pipeline_i2vgen_xl.py:29`` and calls at ``:845,1146,1395``),
with every layer executed by the hand-written HIP kernels of ``libanyv2v_hip.so``.

Design (not a port of the diffusers forward):
  * one activation layout everywhere: channels-last token matrices ``X[(b f)(h w), C]`` fp16.  Conv2d 3x3,
    the temporal (3,1,1) conv and every Linear are the same gather-GEMM kernel; spatial, cross and temporal
    attention are the same strided flash kernel -> none of the reference's permute/reshape round trips exist;
  * skip concatenations are never materialised (two-source K loop / two-source GroupNorm);
  * everything that does not depend on the timestep is computed once per clip and cached: fps embedding,
    the 145-token context and all 16 cross-attention K/V projections, the image-latents branch
    (exact hoisting);
  * all 22 ``time_emb_proj`` Linears run as ONE GEMM per step;
  * PnP feature injection (``i2vgen-xl/pnp_utils.py``) is aliasing / dead-compute elimination, not copies:
    Q/K of the two target branches alias the source branch inside the attention kernel, and on conv-injection
    steps the main path of ``up_blocks[1].resnets[1]`` runs for the source branch only.
The attribute paths the reference hooks rely on (``pnp_utils.py:20-27,130,239,344``) are preserved:
``unet.up_blocks[i].resnets[j]``, ``.attentions[j].transformer_blocks[0].attn1.processor``, ``.temp_attentions[j]...``.
"""
from __future__ import annotations

import copy
import math
import os

from dataclasses import dataclass
from typing import List, Optional, Tuple

import torch
import torch.nn as nn

from . import ops
from .ops import ACT_GEGLU, ACT_GELU, ACT_NONE, ACT_SILU, MODE_CONV2D, MODE_TEMPORAL


@dataclass
class I2VGenXLUNetConfig:
    in_channels: int = 4
    out_channels: int = 4
    block_out_channels: Tuple[int, ...] = (320, 640, 1280, 1280)
    layers_per_block: int = 2
    norm_num_groups: int = 32
    cross_attention_dim: int = 1024
    attention_head_dim: int = 64
    transformer_in_heads: int = 8
    sample_size: int = 32
    down_block_types: Tuple[str, ...] = ("CrossAttnDownBlock3D",) * 3 + ("DownBlock3D",)
    up_block_types: Tuple[str, ...] = ("UpBlock3D",) + ("CrossAttnUpBlock3D",) * 3

    @property
    def time_embed_dim(self) -> int:
        return self.block_out_channels[0] * 4

    @staticmethod
    def from_json(path: str) -> "I2VGenXLUNetConfig":
        """``<checkpoint>/unet/config.json`` as diffusers writes it (``I2VGenXLUNet.register_to_config``); unknown keys
        (``_class_name``, ``num_attention_heads`` -- which diffusers itself overrides with attention_head_dim) are ignored."""
        import json
        with open(path) as f:
            d = json.load(f)
        kw = {}
        for k in ("in_channels", "out_channels", "layers_per_block", "norm_num_groups", "cross_attention_dim", "sample_size"):
            if d.get(k) is not None:
                kw[k] = int(d[k])
        for k in ("block_out_channels", "down_block_types", "up_block_types"):
            if d.get(k) is not None:
                kw[k] = tuple(d[k])
        if d.get("attention_head_dim") is not None:
            ahd = d["attention_head_dim"]
            kw["attention_head_dim"] = int(ahd[0] if isinstance(ahd, (list, tuple)) else ahd)
        if d.get("transformer_in_heads") is not None:  # (not a diffusers key: diffusers hard-codes 8; mini checkpoints set it)
            kw["transformer_in_heads"] = int(d["transformer_in_heads"])
        return I2VGenXLUNetConfig(**kw)

    @staticmethod
    def mini() -> "I2VGenXLUNetConfig":
        return I2VGenXLUNetConfig(block_out_channels=(64, 128, 256, 256), cross_attention_dim=128,
                                  transformer_in_heads=2, sample_size=8)


def _param(*shape):
    return nn.Parameter(torch.empty(*shape, dtype=torch.float16), requires_grad=False)


def pnp_on(t, schedule) -> bool:
    """``self.injection_schedule is not None and (self.t in self.injection_schedule or self.t == 1000)``
    (``i2vgen-xl/pnp_utils.py:109,189,295``) without a device sync: schedules are python int sets here."""
    if schedule is None or t is None:
        return False
    t = int(t)
    if t == 1000:
        return True
    if isinstance(schedule, (set, frozenset)):
        return t in schedule
    return t in {int(s) for s in schedule}


# ------------------------------------------------------------------------------------------- leaf layers
class Linear(nn.Module):
    def __init__(self, cin, cout, bias=True):
        super().__init__()
        self.in_features, self.out_features = cin, cout
        self.weight = _param(cout, cin)
        self.bias = _param(cout) if bias else None

    def forward(self, x, *unused):  # torch-style call (compat seam B1: ``attn.to_q(hidden_states)``)
        shp = x.shape
        y = ops.gemm(x.reshape(-1, shp[-1]).contiguous(), self.weight, bias=self.bias)
        return y.reshape(*shp[:-1], self.out_features)


class Conv2d(nn.Module):
    def __init__(self, cin, cout, k, stride=1, padding=0, pad_cin_to: Optional[int] = None):
        super().__init__()
        self.cin, self.cout, self.k, self.stride = cin, cout, k, stride
        self.weight = _param(cout, cin, k, k)
        self.bias = _param(cout)
        self.pad_cin_to = pad_cin_to
        self._w = None

    def pack(self):
        w = self.weight.data
        if self.pad_cin_to and self.pad_cin_to > self.cin:
            wp = torch.zeros(self.cout, self.pad_cin_to, self.k, self.k, dtype=w.dtype, device=w.device)
            wp[:, : self.cin] = w
            w = wp
        self._w = w.permute(0, 2, 3, 1).reshape(self.cout, -1).contiguous()  # [Cout, (ky kx cin)]

    def forward(self, x, *unused):
        """torch-style call on an NCHW tensor (compat seam B2: ``self.conv1(hidden_states)`` inside a replaced
        ``ResnetBlock2D.forward``, ``i2vgen-xl/pnp_utils.py:78,107,117-122``) -- same HIP kernel behind a layout round trip."""
        if self._w is None:
            self.pack()
        n, c, H, W = x.shape
        tok = x.to(torch.float16).permute(0, 2, 3, 1).reshape(n * H * W, c).contiguous()
        if self.pad_cin_to and self.pad_cin_to > c:
            tok = torch.nn.functional.pad(tok, (0, self.pad_cin_to - c))
        y = self.tokens(tok, H, W)
        Ho, Wo = (H, W) if self.k == 1 else ((H + 2 - 3) // self.stride + 1, (W + 2 - 3) // self.stride + 1)
        return y.view(n, Ho, Wo, self.cout).permute(0, 3, 1, 2)

    def tokens(self, x, H, W, *, x1=None, up=False, act=ACT_NONE, rowvec=None, rowvec_div=0, residual=None, out=None,
               asym=False, gn=None, _launch=None):
        """x: [N*H*W, Cin] tokens -> [N*Ho*Wo, Cout].  ``asym``: zero padding only after the last row / column
        (``F.pad(x, (0, 1, 0, 1))`` + padding-0 conv of the AutoencoderKL encoder's Downsample2D).  ``gn`` = (records,
        rows_per_group, groups): also write the consumer GroupNorm's records (``ops.gemm``)."""
        if _launch is not None:   # tokens_gn_floats: the same descriptor, handed to the query instead of the launch
            launch, kw = _launch, {}
        else:
            launch, kw = ops.gemm, ({"out": out} if gn is None else {"out": out, "gn": gn})
        if self.k == 1:
            return launch(x, self._w, a1=x1, bias=self.bias, act=act, residual=residual, **kw)
        if up:
            Ho, Wo = 2 * H, 2 * W
        elif asym:
            Ho, Wo = (H + 1 - 3) // self.stride + 1, (W + 1 - 3) // self.stride + 1
        else:
            Ho, Wo = (H + 2 - 3) // self.stride + 1, (W + 2 - 3) // self.stride + 1
        n_img = x.shape[0] // (H * W)
        return launch(x, self._w, a1=x1, bias=self.bias, act=act, rowvec=rowvec, rowvec_div=rowvec_div,
                      residual=residual, mode=MODE_CONV2D, conv=(H, W, Ho, Wo, self.stride, int(up), int(asym)),
                      M=n_img * Ho * Wo, **kw)

    def tokens_gn_floats(self, x, H, W, rows_per_group, groups, **kw):
        """Floats of GroupNorm records ``tokens(x, H, W, gn=(records, rows_per_group, groups), **kw)`` would write, 0 when that
        launch's plan cannot emit them (``ops.gemm_gn_stats_floats``); launches nothing."""
        return self.tokens(x, H, W, _launch=lambda *a, **k: ops.gemm_gn_stats_floats(*a, rows_per_group=rows_per_group, groups=groups, **k),
                           **kw)


def _gn_records(ctx, M, rows_per_group, groups):
    """Record buffer for GroupNorm statistics from a GEMM epilogue (``ANYV2V_GN_EPILOGUE=1``), or None: switch off, a
    frame-parallel clip (its norms are sharded), or a statistics group that is not a whole number of 16-row records.  One buffer
    per step engine (``ctx``), sized in ``_prepare_clip``; a context without one gets it on its first, eager forward -- never
    inside a graph capture."""
    if not ops.GN_EPILOGUE or getattr(ctx, "fp", None) is not None:
        return None
    need = ops.gn_stats_floats(M, rows_per_group, groups)
    if need == 0:
        return None
    rec = getattr(ctx, "gn_rec", None)
    if rec is None or rec.numel() < need:
        assert not torch.cuda.is_current_stream_capturing(), "GroupNorm record buffer must exist before a graph capture"
        rec = ctx.gn_rec = torch.empty(need, dtype=torch.float32, device="cuda")
    return rec


class Conv3dTemporal(nn.Module):
    """Conv3d(C, C, (3,1,1), padding=(1,0,0))."""

    def __init__(self, cin, cout):
        super().__init__()
        self.weight = _param(cout, cin, 3, 1, 1)
        self.bias = _param(cout)
        self._w = None

    def pack(self):
        w = self.weight.data[:, :, :, 0, 0]  # [Cout, Cin, 3]
        self._w = w.permute(0, 2, 1).reshape(w.shape[0], -1).contiguous()  # [Cout, (dt cin)]


class GroupNorm(nn.Module):
    def __init__(self, groups, channels, eps=1e-5):
        super().__init__()
        self.num_groups, self.eps = groups, eps
        self.weight = _param(channels)
        self.bias = _param(channels)

    def forward(self, x):
        """torch-style call on an NCHW tensor (compat seam B2: ``self.norm1(hidden_states)``, ``pnp_utils.py:48,104``)."""
        n, c = x.shape[:2]
        hw = x[0, 0].numel()
        tok = x.to(torch.float16).reshape(n, c, hw).permute(0, 2, 1).reshape(n * hw, c).contiguous()
        stats = torch.empty(ops.gn_scratch_floats(n, 1, self.num_groups), dtype=torch.float32, device=x.device)
        y = ops.groupnorm(tok, self.weight, self.bias, stats, hw, groups=self.num_groups, eps=self.eps)
        return y.view(n, hw, c).permute(0, 2, 1).reshape(x.shape)


class LayerNorm(nn.Module):
    def __init__(self, channels, eps=1e-5):
        super().__init__()
        self.eps = eps
        self.weight = _param(channels)
        self.bias = _param(channels)


class SiLU(nn.Module):
    def forward(self, x):
        return ops.silu(x.contiguous())


class Identity(nn.Module):
    def forward(self, x, *a, **k):
        return x


def expand_shared(x, full_ctx):
    """Shared-stem batch -> full batch: the last batch element is repeated ([source, shared] -> [source, negative,
    editing] for the PnP edit; [shared] -> [negative, positive] for plain CFG sampling)."""
    Bs = full_ctx.B - 1
    n = x.shape[0] // Bs
    out = torch.empty(((Bs + 1) * n, x.shape[1]), dtype=x.dtype, device=x.device)
    out[:Bs * n].copy_(x)
    out[Bs * n:].copy_(x[(Bs - 1) * n:])
    return out


# ------------------------------------------------------------------------------------------- attention
class Geom:
    """How a token matrix [(b f)(h w), C] decomposes into attention sequences."""

    def __init__(self, kind: str, B: int, F: int, HW: int):
        self.kind, self.B, self.F, self.HW = kind, B, F, HW
        if kind == "spatial":
            self.batch, self.S, self.inner = B * F, HW, 1
            self.strides = (HW, 0, 1)
        else:  # temporal: one sequence of F frames per (b, pixel)
            self.batch, self.S, self.inner = B * HW, F, HW
            self.strides = (F * HW, 1, HW)


class HipAttnProcessor:
    """Native ``AttnProcessor2_0`` (``i2vgen-xl/pnp_utils.py:151-228``): fused QKV GEMM -> strided flash
    attention -> out-projection GEMM with bias + residual epilogue.  With ``injection_schedule`` set it is the
    native ``ModifiedSpaAttnProcessor`` / ``ModifiedTmpAttnProcessor`` (``pnp_utils.py:141-228,247-334``): on
    injection steps Q and K of the uncond / cond branches alias the source branch (qk_mod), no copies."""

    def __init__(self, injection_schedule=None):
        self.injection_schedule = injection_schedule
        self.t = None
        # source-feature cache of a multi-edit job (step_engine.SourceFeatureCache): None, ("record", buf) -- copy the source branch's
        # Q | K columns of this step into ``buf`` [Ts, 2 C] -- or ("replay", buf): the batch is [negative, editing] only and the
        # source branch's Q, K are read from ``buf`` (recorded by an earlier edit of the same clip)
        self.src_io = None

    def run(self, attn: "Attention", ctx, h, geom: Geom, residual, kv=None, ln_in=None):
        """``ln_in`` = (x, (W', b', c1), eps): the block's LayerNorm is folded into this attention's first projection
        (``ops.gemm(..., ln=...)``); ``h`` is then None and ``x`` the un-normalised residual stream."""
        Cq = attn.inner_dim
        if ln_in is not None:
            h, (w_in, b_in, c1_in), ln_eps = ln_in

            def proj(rows, lo=0, out=None):   # rows of x -> columns [lo, ...) of the folded projection
                return ops.gemm(rows, w_in[lo:], bias=b_in[lo:], ln=(c1_in[lo:], ln_eps), out=out)
        else:
            def proj(rows, lo=0, out=None):
                return ops.gemm(rows, (attn._w_qkv if kv is None else attn.to_q.weight)[lo:], out=out)
        T = h.shape[0]
        o = torch.empty((T, Cq), dtype=torch.float16, device=h.device)
        if kv is None:  # self-attention
            inject = pnp_on(self.t, self.injection_schedule)
            if (ln_in is not None and geom.kind == "temporal" and not inject and self.src_io is None
                    and ops.temporal_qkv_attn_supported(T // geom.B, Cq, attn.heads, geom.F, geom.HW, h)):
                # plain temporal self-attention at the 64x64 level: projection and attention in one kernel, bit-equal to the two
                # launches below (tattn_fused.hip) -- QKV never reaches HBM; one branch's rows decide, as in ``_fold``
                ops.temporal_qkv_attn(h, w_in, b_in, c1_in, ln_eps, B=geom.B, F=geom.F, HW=geom.HW, heads=attn.heads, scale=attn.scale,
                                      out=o)
                return ops.gemm(o, attn.to_out[0].weight, bias=attn.to_out[0].bias, residual=residual)
            io = self.src_io if inject else None
            if io is not None and io[0] == "replay":
                # [negative, editing] with the source branch's Q, K from the cache: only V is projected here; the kernel aliases
                # Q, K of batch element i to element i % (batch / 2) of the cached source rows (same arithmetic per output as the
                # three-branch shared-softmax launch: bit-equal, tests/gpu_checks.py)
                src_qk = io[1]
                assert src_qk.shape[0] * 2 == T and src_qk.shape[1] == 2 * Cq
                qkv = torch.empty((T, 3 * Cq), dtype=torch.float16, device=h.device)
                proj(h, 2 * Cq, qkv[:, 2 * Cq:])
                ops.attention(src_qk[:, :Cq], src_qk[:, Cq:], qkv[:, 2 * Cq:], o, batch=geom.batch, heads=attn.heads, Sq=geom.S,
                              Sk=geom.S, inner=geom.inner, q_strides=geom.strides, kv_strides=geom.strides,
                              qk_mod=geom.batch // 2, scale=attn.scale)
                return ops.gemm(o, attn.to_out[0].weight, bias=attn.to_out[0].bias, residual=residual)
            if inject and T % 3 == 0 and _V_ONLY:
                # Q and K of the negative / editing branches are never read on an injection step (they alias the source
                # branch's): project Q,K,V for the source third and only V for the other two thirds (exact, 44 % fewer
                # FLOPs and stores in this projection)
                Ts = T // 3
                qkv = torch.empty((T, 3 * Cq), dtype=torch.float16, device=h.device)
                proj(h[:Ts], 0, qkv[:Ts])
                proj(h[Ts:], 2 * Cq, qkv[Ts:, 2 * Cq:])
            else:
                qkv = proj(h)
            if io is not None and io[0] == "record":
                io[1].copy_(qkv[:T // 3, :2 * Cq])
            qk_mod = geom.batch // 3 if inject else 0
            ops.attention(qkv[:, :Cq], qkv[:, Cq:2 * Cq], qkv[:, 2 * Cq:], o, batch=geom.batch, heads=attn.heads,
                          Sq=geom.S, Sk=geom.S, inner=geom.inner, q_strides=geom.strides, kv_strides=geom.strides,
                          qk_mod=qk_mod, scale=attn.scale)
        else:  # cross-attention against the per-clip cached K/V  ([B*Sk, 2C] column window of ctx.kv_all)
            q = proj(h)
            k_, v_, Sk = kv
            ops.attention(q, k_, v_, o, batch=geom.batch, heads=attn.heads, Sq=geom.S, Sk=Sk, inner=1,
                          q_strides=geom.strides, kv_strides=(Sk, 0, 1), kv_div=geom.F, scale=attn.scale)
        return ops.gemm(o, attn.to_out[0].weight, bias=attn.to_out[0].bias, residual=residual)


class Attention(nn.Module):
    def __init__(self, query_dim, cross_attention_dim=None, heads=8, dim_head=64):
        super().__init__()
        self.inner_dim = heads * dim_head
        self.heads, self.dim_head = heads, dim_head
        self.scale = dim_head ** -0.5
        self.is_cross = cross_attention_dim is not None
        ctx_dim = cross_attention_dim if cross_attention_dim is not None else query_dim
        self.to_q = Linear(query_dim, self.inner_dim, bias=False)
        self.to_k = Linear(ctx_dim, self.inner_dim, bias=False)
        self.to_v = Linear(ctx_dim, self.inner_dim, bias=False)
        self.to_out = nn.ModuleList([Linear(self.inner_dim, query_dim, bias=True), Identity()])
        # attribute surface read by the reference processors
        self.spatial_norm = None
        self.group_norm = None
        self.norm_cross = None
        self.residual_connection = False
        self.rescale_output_factor = 1.0
        self.processor = HipAttnProcessor()
        self._w_qkv = None
        self._w_kv = None

    def pack(self):
        if self.is_cross:
            self._w_kv = torch.cat([self.to_k.weight.data, self.to_v.weight.data], 0).contiguous()
        else:
            self._w_qkv = torch.cat([self.to_q.weight.data, self.to_k.weight.data, self.to_v.weight.data], 0).contiguous()

    def prepare_attention_mask(self, attention_mask, target_length, batch_size, out_dim=3):
        return attention_mask

    def run(self, ctx, h, geom: Geom, residual, kv=None, ln_in=None):
        proc = self.processor
        if isinstance(proc, HipAttnProcessor):
            return proc.run(self, ctx, h, geom, residual, kv, ln_in)
        assert ln_in is None, "a foreign processor takes the normalised hidden states"
        return self._run_foreign(proc, ctx, h, geom, residual, kv)

    def _run_foreign(self, proc, ctx, h, geom: Geom, residual, kv):
        """Compatibility seam B1: a torch-style processor object (e.g. the reference's own
        ``ModifiedSpaAttnProcessor``) was plugged in.  Give it the [batch, S, C] tensor it expects (the temporal
        view needs a real permute here), run it, and fold the result back into the token layout."""
        C = h.shape[1]
        if geom.kind == "spatial":
            hs = h.view(geom.batch, geom.S, C)
        else:
            hs = h.view(geom.B, geom.F, geom.HW, C).permute(0, 2, 1, 3).reshape(geom.batch, geom.S, C)
        ehs = None
        if kv is not None:
            ehs = ctx.context.view(ctx.B, ctx.Sk, -1).repeat_interleave(geom.F, dim=0)
        out = proc(self, hs, encoder_hidden_states=ehs)
        if geom.kind != "spatial":
            out = out.view(geom.B, geom.HW, geom.F, C).permute(0, 2, 1, 3)
        out = out.reshape(-1, C).contiguous()
        return ops.add(out, residual)


class GEGLU(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = Linear(dim_in, dim_out * 2)
        self.dim_out = dim_out
        self._w = self._b = None

    def pack(self):
        """Interleave [16 rows of h | 16 rows of gate] so that a lane holds matching (h, gate) pairs (the GEGLU epilogues of gemm_mfma.hip / gemm_big.hip)."""
        w, b = self.proj.weight.data, self.proj.bias.data
        n = self.dim_out
        assert n % 16 == 0
        wh, wg = w[:n].view(n // 16, 16, -1), w[n:].view(n // 16, 16, -1)
        self._w = torch.stack([wh, wg], 1).reshape(2 * n, -1).contiguous()
        bh, bg = b[:n].view(n // 16, 16), b[n:].view(n // 16, 16)
        self._b = torch.stack([bh, bg], 1).reshape(2 * n).contiguous()


class GELUProj(nn.Module):
    def __init__(self, dim_in, dim_out):
        super().__init__()
        self.proj = Linear(dim_in, dim_out)


class FeedForward(nn.Module):
    def __init__(self, dim, inner_dim=None, activation_fn="geglu"):
        super().__init__()
        inner_dim = inner_dim or dim * 4
        self.geglu = activation_fn == "geglu"
        act = GEGLU(dim, inner_dim) if self.geglu else GELUProj(dim, inner_dim)
        self.net = nn.ModuleList([act, Identity(), Linear(inner_dim, dim)])

    def pack(self):
        """The fused feed-forward kernel's layout of the down-projection (``ops.ff_pack_w2``), for the width it covers."""
        lin = self.net[2]
        self._w2s = ops.ff_pack_w2(lin.weight.data) if (self.geglu and tuple(lin.weight.shape) == (320, 1280)) else None

    def run(self, h, residual, ln_in=None):
        w2s = getattr(self, "_w2s", None)
        if ln_in is None and w2s is not None and ops.ff_fused_supported(h.shape[0], h.shape[1], w2s.shape[0] * 32):
            # GEGLU up-projection + down-projection + residual in ONE kernel: the [tokens, 1280] hidden never reaches HBM
            return ops.ff_geglu(h, self.net[0]._w, self.net[0]._b, w2s, self.net[2].bias, residual=residual)
        if ln_in is not None:   # LayerNorm folded into the GEGLU up-projection (BasicTransformerBlock.pack)
            x, (w_in, b_in, c1_in), ln_eps = ln_in
            g = ops.gemm(x, w_in, bias=b_in, act=ACT_GEGLU, ln=(c1_in, ln_eps))
        elif self.geglu:
            g = ops.gemm(h, self.net[0]._w, bias=self.net[0]._b, act=ACT_GEGLU)
        else:
            g = ops.gemm(h, self.net[0].proj.weight, bias=self.net[0].proj.bias, act=ACT_GELU)
        return ops.gemm(g, self.net[2].weight, bias=self.net[2].bias, residual=residual)


class BasicTransformerBlock(nn.Module):
    def __init__(self, dim, heads, dim_head, cross_attention_dim=None, double_self_attention=False):
        super().__init__()
        self.norm1 = LayerNorm(dim)
        self.attn1 = Attention(dim, None, heads, dim_head)
        self.norm2 = LayerNorm(dim)
        self.attn2 = Attention(dim, None if double_self_attention else cross_attention_dim, heads, dim_head)
        self.norm3 = LayerNorm(dim)
        self.ff = FeedForward(dim)

    def pack(self):
        """LayerNorm folds for the widths the weight-stationary GEMM covers (``ops.ln_gemm_supported``: the 64x64 level's 320
        channels; transformer_in's 512 for the GEGLU): norm1 -> attn1's fused QKV, norm2 -> attn2's to_q (cross) or QKV (the
        temporal blocks' second self-attention), norm3 -> the GEGLU up-projection (interleaved as ``GEGLU.pack`` lays it out)."""
        self._ln = {}
        dim = self.norm1.weight.shape[0]
        if dim not in (320, 512) or _NO_LN_FOLD:
            return
        cat = lambda a: torch.cat([a.to_q.weight.data, a.to_k.weight.data, a.to_v.weight.data], 0)
        if dim == 320:
            self._ln["attn1"] = ops.ln_fold(cat(self.attn1), None, self.norm1.weight.data, self.norm1.bias.data)
            w2 = self.attn2.to_q.weight.data if self.attn2.is_cross else cat(self.attn2)
            self._ln["attn2"] = ops.ln_fold(w2, None, self.norm2.weight.data, self.norm2.bias.data)
        # norm3 -> GEGLU: the fold is supported (and tested) but does not pay -- the up-projection is bound by its erf-GELU
        # epilogue, to which the fold adds two fma per output (423 vs 435 us at 196608 rows, profiles/r03_gemm_ws_ab.txt)
        if self.ff.geglu and _LN_FOLD_FF:
            g = self.ff.net[0]
            w, b, c1 = ops.ln_fold(g.proj.weight.data, g.proj.bias.data, self.norm3.weight.data, self.norm3.bias.data)
            n = g.dim_out
            il = lambda t: torch.stack([t[:n].reshape(n // 16, 16, *t.shape[1:]), t[n:].reshape(n // 16, 16, *t.shape[1:])], 1) \
                .reshape(2 * n, *t.shape[1:]).contiguous()
            self._ln["ff"] = (il(w), il(b), il(c1))

    def _fold(self, name, proc_ok, M, N, act=ACT_NONE, per_branch=False):
        """``per_branch``: ``M`` is the row count of ONE batch element -- the canonical quantity for the attention projections, whose
        launches see one, two or three branches' rows depending on the engine (V-only thirds at injected sites, [negative, editing]
        steps under the batch hint, the shared stem): every engine must take the same decision for the same branch, or the
        bit-equality of the two-branch steps with the three-branch step breaks at mid sizes."""
        f = getattr(self, "_ln", {}).get(name)
        return f if (f is not None and proc_ok and ops.ln_gemm_supported(M, self.norm1.weight.shape[0], N, act, hinted=not per_branch)) else None

    def run(self, ctx, x, geom: Geom, expand=None, shrink=None):
        """``expand`` = (full ctx, full geometry): the block was entered with the shared-stem batch (see
        ``I2VGenXLUNet._forward_core``); after self-attention the tokens are expanded to the full batch, where the
        branches start to differ (cross-attention context).
        ``shrink`` = geometry without the first batch element: this block's self-attention is the LAST hook site of a PnP step
        whose source-branch output nobody reads (``_forward_core(drop_source_tail=True)``); from here on only [negative, editing] are computed,
        under the batch hint (3, 2) so that every launch makes the three-branch launch's choices (bit-equal rows).

        Each LayerNorm is folded into the projection that consumes it where the weight-stationary GEMM covers the shape
        (``pack``); otherwise -- other widths, small clips, a foreign processor on the seam -- it is the LayerNorm kernel."""
        dim = x.shape[1]
        rows_b = lambda t, g: t.shape[0] // g.B   # rows of one branch: the same number in every engine that computes that branch
        f = self._fold("attn1", isinstance(self.attn1.processor, HipAttnProcessor), rows_b(x, geom), 3 * dim, per_branch=True)
        if f is not None:
            x = self.attn1.run(ctx, None, geom, residual=x, ln_in=(x, f, self.norm1.eps))
        else:
            h = ops.layernorm(x, self.norm1.weight, self.norm1.bias, self.norm1.eps)
            x = self.attn1.run(ctx, h, geom, residual=x)
        if expand is not None:
            after = getattr(ctx, "batch_hint_after", None)
            ctx, geom = expand
            x = expand_shared(x, ctx)
            if after is not None:   # the stem ends here: from now on the full batch's hint
                ops.set_batch_hint(*after)
        if shrink is not None:
            x = x[x.shape[0] // 3:]
            geom = shrink
            ops.set_batch_hint(3, 2)
        kv = ctx.kv_for(self.attn2) if self.attn2.is_cross else None
        f = self._fold("attn2", isinstance(self.attn2.processor, HipAttnProcessor), rows_b(x, geom), dim if self.attn2.is_cross else 3 * dim,
                       per_branch=True)
        if f is not None:
            x = self.attn2.run(ctx, None, geom, residual=x, kv=kv, ln_in=(x, f, self.norm2.eps))
        else:
            h = ops.layernorm(x, self.norm2.weight, self.norm2.bias, self.norm2.eps)
            x = self.attn2.run(ctx, h, geom, residual=x, kv=kv)
        f = self._fold("ff", True, x.shape[0], 8 * dim, ACT_GEGLU)
        if f is not None:
            return self.ff.run(None, residual=x, ln_in=(x, f, self.norm3.eps))
        h = ops.layernorm(x, self.norm3.weight, self.norm3.bias, self.norm3.eps)
        return self.ff.run(h, residual=x)


class Transformer2DModel(nn.Module):
    def __init__(self, heads, dim_head, in_channels, cross_attention_dim, groups):
        super().__init__()
        inner = heads * dim_head
        self.norm = GroupNorm(groups, in_channels, eps=1e-6)
        self.proj_in = Linear(in_channels, inner)
        self.transformer_blocks = nn.ModuleList([BasicTransformerBlock(inner, heads, dim_head, cross_attention_dim)])
        self.proj_out = Linear(inner, in_channels)

    def run(self, ctx, x, H, W, full_ctx=None):
        """``full_ctx``: ``x`` holds the shared-stem batch of ``ctx``; the output has the full batch of ``full_ctx``."""
        HW = H * W
        h = ops.groupnorm(x, self.norm.weight, self.norm.bias, ctx.stats, HW, groups=self.norm.num_groups,
                          eps=self.norm.eps)
        h = ops.gemm(h, self.proj_in.weight, bias=self.proj_in.bias)
        geom = Geom("spatial", ctx.B, ctx.F, HW)
        for i, blk in enumerate(self.transformer_blocks):
            if full_ctx is not None and i == 0:
                h = blk.run(ctx, h, geom, expand=(full_ctx, Geom("spatial", full_ctx.B, full_ctx.F, HW)))
                ctx, geom = full_ctx, Geom("spatial", full_ctx.B, full_ctx.F, HW)
                x = expand_shared(x, full_ctx)
            else:
                h = blk.run(ctx, h, geom)
        return ops.gemm(h, self.proj_out.weight, bias=self.proj_out.bias, residual=x)


class TransformerTemporalModel(nn.Module):
    def __init__(self, heads, dim_head, in_channels, groups):
        super().__init__()
        inner = heads * dim_head
        self.norm = GroupNorm(groups, in_channels, eps=1e-6)
        self.proj_in = Linear(in_channels, inner)
        self.transformer_blocks = nn.ModuleList(
            [BasicTransformerBlock(inner, heads, dim_head, None, double_self_attention=True)])
        self.proj_out = Linear(inner, in_channels)

    def run(self, ctx, x, H, W):
        fp = getattr(ctx, "fp", None)   # frame-parallel clip: re-shard frames -> pixels around the layer (parallel.py)
        return self._run(ctx, x, H * W, None) if fp is None else fp.temporal(ctx, x, H * W, self._run)

    def _run(self, ctx, x, HW, shard):
        # 5-D GroupNorm: statistics over all frames of a clip
        h = ops.groupnorm(x, self.norm.weight, self.norm.bias, ctx.stats, ctx.F * HW, groups=self.norm.num_groups,
                          eps=self.norm.eps, shard=shard)
        h = ops.gemm(h, self.proj_in.weight, bias=self.proj_in.bias)
        geom = Geom("temporal", ctx.B, ctx.F, HW)
        drop = shard is None and getattr(ctx, "drop_tail_at", None) is self and not self.transformer_blocks[0].attn2.is_cross
        for i, blk in enumerate(self.transformer_blocks):
            if drop and i == 0:
                h = blk.run(ctx, h, geom, shrink=Geom("temporal", ctx.B - 1, ctx.F, HW))
                geom = Geom("temporal", ctx.B - 1, ctx.F, HW)
                x = x[x.shape[0] // 3:]
            else:
                h = blk.run(ctx, h, geom)
        return ops.gemm(h, self.proj_out.weight, bias=self.proj_out.bias, residual=x)


# ------------------------------------------------------------------------------------------- conv blocks
class Upsample2D(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.conv = Conv2d(channels, channels, 3, padding=1)


class Downsample2D(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.conv = Conv2d(channels, channels, 3, stride=2, padding=1)


class ResnetBlock2D(nn.Module):
    """Native ``ResnetBlock2D`` == the body at ``i2vgen-xl/pnp_utils.py:46-126`` including the conv-feature
    injection of ``:109-115`` when ``injection_schedule`` is set (``register_conv_injection``)."""

    def __init__(self, in_channels, out_channels, temb_channels, groups, eps=1e-5):
        super().__init__()
        self.in_channels, self.out_channels = in_channels, out_channels
        self.norm1 = GroupNorm(groups, in_channels, eps)
        self.conv1 = Conv2d(in_channels, out_channels, 3, padding=1)
        self.time_emb_proj = Linear(temb_channels, out_channels)
        self.norm2 = GroupNorm(groups, out_channels, eps)
        self.dropout = Identity()
        self.conv2 = Conv2d(out_channels, out_channels, 3, padding=1)
        self.nonlinearity = SiLU()
        self.upsample = self.downsample = None
        self.conv_shortcut = Conv2d(in_channels, out_channels, 1) if in_channels != out_channels else None
        self.skip_time_act = False
        self.time_embedding_norm = "default"
        self.output_scale_factor = 1.0
        self.t = None
        self.injection_schedule = None
        self.src_io = None  # source-feature cache, see HipAttnProcessor: ("record" | "replay", buf [Ts, Cout]) of the conv features
        self._temb_col = 0  # column of this block's time_emb_proj inside ctx.temb_all
        # GroupNorm statistics over (channels of the group, h, w) of every frame -- the 4-D GroupNorm of diffusers' ResnetBlock2D --
        # or over all frames of a batch element as well (SEINE's ResnetBlock3D normalises [b, c, f, h, w], seine/models/resnet.py:143,177)
        self.norm_over_frames = False

    def forward(self, input_tensor, temb, scale: float = 1.0):
        """torch-style ``ResnetBlock2D.forward(input_tensor[N,Cin,H,W], temb[N,1280])`` (seam B2; the body the reference
        restates at ``i2vgen-xl/pnp_utils.py:46-126``) on the HIP kernels, without injection.  The network itself never
        calls this (it runs ``run`` on token matrices); it exists so that the module behaves like the diffusers one."""
        n, c, H, W = input_tensor.shape
        h = self.nonlinearity(self.norm1(input_tensor))
        h = self.conv1(h) + self.time_emb_proj(self.nonlinearity(temb.to(torch.float16)))[:, :, None, None]
        h = self.conv2(self.nonlinearity(self.norm2(h)))
        if self.conv_shortcut is not None:
            input_tensor = self.conv_shortcut(input_tensor)
        return (input_tensor.to(torch.float16) + h) / self.output_scale_factor

    def _run_foreign(self, ctx, x0, x1, H, W):
        """Compatibility seam B2: ``module.forward`` was replaced on the instance (the reference's
        ``register_conv_injection`` does ``conv_module.forward = conv_forward(conv_module)``, ``pnp_utils.py:130-131``).
        Hand it the NCHW tensors it expects -- its sub-module calls (``self.norm1`` / ``self.conv1`` / ...) still land on
        the HIP kernels through their torch-style ``forward`` -- and fold the result back into the token layout."""
        N = x0.shape[0] // (H * W)
        x = x0 if x1 is None else torch.cat([x0, x1], 1)
        x = x.view(N, H, W, -1).permute(0, 3, 1, 2)
        per = N // ctx.emb.shape[0]   # frames per batch element (temb is per clip-branch; the reference repeats it per frame)
        temb = ctx.emb.repeat_interleave(per, dim=0)
        out = self.__dict__["forward"](x, temb)
        return out.to(torch.float16).permute(0, 2, 3, 1).reshape(N * H * W, -1).contiguous()

    def run(self, ctx, x0, x1, H, W):
        if "forward" in self.__dict__:
            return self._run_foreign(ctx, x0, x1, H, W)
        HW = H * W
        T = x0.shape[0]
        inject = pnp_on(self.t, self.injection_schedule)
        io = self.src_io if inject else None
        if io is not None and io[0] == "replay":
            # [negative, editing] only: both take the source branch's conv features recorded by an earlier edit of this clip --
            # the main path (two GroupNorms, two 3x3 convolutions) is not run at all
            res = self.conv_shortcut.tokens(x0, H, W, x1=x1) if self.conv_shortcut is not None else x0
            hs, Th = io[1], T // 2
            assert hs.shape[0] == Th
            out = torch.empty((T, self.out_channels), dtype=torch.float16, device=x0.device)
            for b in range(2):
                ops.add(res[b * Th:(b + 1) * Th], hs, out=out[b * Th:(b + 1) * Th])
            return out
        Ts = T // 3 if inject else T  # injection step: main path only for the source branch (exact)
        a0 = x0[:Ts]
        a1 = x1[:Ts] if x1 is not None else None
        g = self.norm1.num_groups
        rpg = ctx.F * HW if self.norm_over_frames else HW
        h = ops.groupnorm(a0, self.norm1.weight, self.norm1.bias, ctx.stats, rpg, x1=a1, groups=g, eps=self.norm1.eps,
                          silu=True)
        tv = ctx.temb_all[:, self._temb_col:self._temb_col + self.out_channels]
        rec = _gn_records(ctx, Ts, rpg, g)
        if rec is not None and self.conv1.tokens_gn_floats(h, H, W, rpg, g, rowvec=tv, rowvec_div=ctx.F * HW) > 0:
            # conv1's epilogue writes norm2's statistics: no partial pass over its output
            h = self.conv1.tokens(h, H, W, rowvec=tv, rowvec_div=ctx.F * HW, gn=(rec, rpg, g))
            h = ops.groupnorm_from_stats(h, self.norm2.weight, self.norm2.bias, rec, rpg, groups=g, eps=self.norm2.eps, silu=True)
        else:
            h = self.conv1.tokens(h, H, W, rowvec=tv, rowvec_div=ctx.F * HW)
            h = ops.groupnorm(h, self.norm2.weight, self.norm2.bias, ctx.stats, rpg, groups=g, eps=self.norm2.eps, silu=True)
        if self.conv_shortcut is not None:
            res = self.conv_shortcut.tokens(x0, H, W, x1=x1)
        else:
            res = x0
        if not inject:
            return self.conv2.tokens(h, H, W, residual=res)
        hs = self.conv2.tokens(h, H, W)  # source-branch features, shared by all three branches
        if io is not None and io[0] == "record":
            io[1].copy_(hs)
        out = torch.empty((T, self.out_channels), dtype=torch.float16, device=x0.device)
        for b in range(3):
            ops.add(res[b * Ts:(b + 1) * Ts], hs, out=out[b * Ts:(b + 1) * Ts])
        return out


class TemporalConvLayer(nn.Module):
    def __init__(self, dim, groups):
        super().__init__()
        self.conv1 = nn.Sequential(GroupNorm(groups, dim), SiLU(), Conv3dTemporal(dim, dim))
        self.conv2 = nn.Sequential(GroupNorm(groups, dim), SiLU(), Identity(), Conv3dTemporal(dim, dim))
        self.conv3 = nn.Sequential(GroupNorm(groups, dim), SiLU(), Identity(), Conv3dTemporal(dim, dim))
        self.conv4 = nn.Sequential(GroupNorm(groups, dim), SiLU(), Identity(), Conv3dTemporal(dim, dim))

    def run(self, ctx, x, H, W):
        fp = getattr(ctx, "fp", None)
        return self._run(ctx, x, H * W, None) if fp is None else fp.temporal(ctx, x, H * W, self._run)

    def _run(self, ctx, x, HW, shard):
        h = x
        seqs = (self.conv1, self.conv2, self.conv3, self.conv4)
        rpg = ctx.F * HW
        rec = None   # records of h, written by the conv that produced it (ANYV2V_GN_EPILOGUE=1: conv i -> norm i + 1)
        for i, seq in enumerate(seqs):
            gn, conv = seq[0], seq[-1]
            if rec is not None:
                h = ops.groupnorm_from_stats(h, gn.weight, gn.bias, rec, rpg, groups=gn.num_groups, eps=gn.eps, silu=True)
            else:
                h = ops.groupnorm(h, gn.weight, gn.bias, ctx.stats, rpg, groups=gn.num_groups, eps=gn.eps, silu=True,
                                  shard=shard)
            rec = None
            if i < 3 and shard is None:
                g_next = seqs[i + 1][0].num_groups
                rec = _gn_records(ctx, h.shape[0], rpg, g_next)
                if rec is not None and ops.gemm_gn_stats_floats(h, conv._w, bias=conv.bias, mode=MODE_TEMPORAL, temporal=(ctx.F, HW),
                                                                rows_per_group=rpg, groups=g_next) == 0:
                    rec = None
            if rec is not None:
                h = ops.gemm(h, conv._w, bias=conv.bias, mode=MODE_TEMPORAL, temporal=(ctx.F, HW), gn=(rec, rpg, g_next))
            else:
                h = ops.gemm(h, conv._w, bias=conv.bias, mode=MODE_TEMPORAL, temporal=(ctx.F, HW),
                             residual=x if i == 3 else None)
        return h


class DownBlock3D(nn.Module):
    def __init__(self, cfg, cin, cout, cross_attn, add_downsample):
        super().__init__()
        g, temb = cfg.norm_num_groups, cfg.time_embed_dim
        self.has_cross_attention = cross_attn
        self.resnets, self.temp_convs = nn.ModuleList(), nn.ModuleList()
        if cross_attn:
            self.attentions, self.temp_attentions = nn.ModuleList(), nn.ModuleList()
        for i in range(cfg.layers_per_block):
            self.resnets.append(ResnetBlock2D(cin if i == 0 else cout, cout, temb, g))
            self.temp_convs.append(TemporalConvLayer(cout, g))
            if cross_attn:
                heads = cout // cfg.attention_head_dim
                self.attentions.append(Transformer2DModel(heads, cfg.attention_head_dim, cout, cfg.cross_attention_dim, g))
                self.temp_attentions.append(TransformerTemporalModel(heads, cfg.attention_head_dim, cout, g))
        self.downsamplers = nn.ModuleList([Downsample2D(cout)]) if add_downsample else None

    def run(self, ctx, x, H, W, stem_ctx=None):
        """``stem_ctx``: ``x`` arrives with the shared-stem batch; layer 0 runs on it up to its first cross-attention."""
        outs = []
        for i in range(len(self.resnets)):
            c = stem_ctx if (stem_ctx is not None and i == 0) else ctx
            x = self.resnets[i].run(c, x, None, H, W)
            x = self.temp_convs[i].run(c, x, H, W)
            if self.has_cross_attention:
                x = self.attentions[i].run(c, x, H, W, full_ctx=ctx if c is not ctx else None)
                x = self.temp_attentions[i].run(ctx, x, H, W)
            outs.append(x)
        if self.downsamplers is not None:
            x = self.downsamplers[0].conv.tokens(x, H, W)
            H, W = (H - 1) // 2 + 1, (W - 1) // 2 + 1     # stride 2, padding 1: odd sizes round up
            outs.append(x)
        return x, outs, H, W


class MidBlock3D(nn.Module):
    def __init__(self, cfg, c):
        super().__init__()
        g, temb = cfg.norm_num_groups, cfg.time_embed_dim
        heads = c // cfg.attention_head_dim
        self.resnets = nn.ModuleList([ResnetBlock2D(c, c, temb, g), ResnetBlock2D(c, c, temb, g)])
        self.temp_convs = nn.ModuleList([TemporalConvLayer(c, g), TemporalConvLayer(c, g)])
        self.attentions = nn.ModuleList([Transformer2DModel(heads, cfg.attention_head_dim, c, cfg.cross_attention_dim, g)])
        self.temp_attentions = nn.ModuleList([TransformerTemporalModel(heads, cfg.attention_head_dim, c, g)])

    def run(self, ctx, x, H, W):
        x = self.resnets[0].run(ctx, x, None, H, W)
        x = self.temp_convs[0].run(ctx, x, H, W)
        x = self.attentions[0].run(ctx, x, H, W)
        x = self.temp_attentions[0].run(ctx, x, H, W)
        x = self.resnets[1].run(ctx, x, None, H, W)
        x = self.temp_convs[1].run(ctx, x, H, W)
        return x


class UpBlock3D(nn.Module):
    def __init__(self, cfg, cin, cout, prev_out, cross_attn, add_upsample):
        super().__init__()
        g, temb = cfg.norm_num_groups, cfg.time_embed_dim
        n = cfg.layers_per_block + 1
        self.has_cross_attention = cross_attn
        self.resnets, self.temp_convs = nn.ModuleList(), nn.ModuleList()
        if cross_attn:
            self.attentions, self.temp_attentions = nn.ModuleList(), nn.ModuleList()
        for i in range(n):
            res_skip = cin if i == n - 1 else cout
            res_in = prev_out if i == 0 else cout
            self.resnets.append(ResnetBlock2D(res_in + res_skip, cout, temb, g))
            self.temp_convs.append(TemporalConvLayer(cout, g))
            if cross_attn:
                heads = cout // cfg.attention_head_dim
                self.attentions.append(Transformer2DModel(heads, cfg.attention_head_dim, cout, cfg.cross_attention_dim, g))
                self.temp_attentions.append(TransformerTemporalModel(heads, cfg.attention_head_dim, cout, g))
        self.upsamplers = nn.ModuleList([Upsample2D(cout)]) if add_upsample else None
        self.freeu = None   # (b, s) of I2VGenXLUNet.enable_freeu on up_blocks[0] / [1]; None: off, nothing below runs

    def run(self, ctx, x, skips: List[torch.Tensor], H, W, out_hw=None):
        """``out_hw``: the size the upsampler has to deliver -- that of the skip connections the next block pops ([3P] diffusers
        ``forward_upsample_size``: a latent size that is not a multiple of 8 does not come back from three ceil-halvings by doubling)."""
        for i in range(len(self.resnets)):
            skip = skips.pop()
            if self.freeu is not None:   # FreeU: backbone half times b, skip through the Fourier filter -- in front of the (folded) concat
                x, skip = ops.freeu(x, skip, x.shape[0] // (H * W), H, W, *self.freeu)
            x = self.resnets[i].run(ctx, x, skip, H, W)  # torch.cat([x, skip], 1) folded into the kernels
            x = self.temp_convs[i].run(ctx, x, H, W)
            if self.has_cross_attention:
                x = self.attentions[i].run(ctx, x, H, W)
                x = self.temp_attentions[i].run(ctx, x, H, W)
        if self.upsamplers is not None:
            x, H, W = upsample_tokens(self.upsamplers[0].conv, x, H, W, out_hw)
        return x, H, W


def upsample_tokens(conv, x, H, W, out_hw=None):
    """``Upsample2D``: nearest x 2 (``out_hw`` None or exactly the double: folded into the conv's gather) or nearest to exactly ``out_hw``,
    then the 3 x 3 convolution -> (tokens, Ho, Wo).  For Ho in (2 H - 1, 2 H) the source index floor(o H / Ho) is o >> 1 either way, but
    the conv's zero padding starts at Ho, not at 2 H: the resized image is materialised (one gather) and convolved plainly."""
    if out_hw is None or tuple(out_hw) == (2 * H, 2 * W):
        return conv.tokens(x, H, W, up=True), 2 * H, 2 * W
    Ho, Wo = out_hw
    if Ho not in (2 * H - 1, 2 * H) or Wo not in (2 * W - 1, 2 * W):
        raise ValueError(f"upsample {H} x {W} -> {Ho} x {Wo}: not the size of a skip connection of this UNet")
    n_img = x.shape[0] // (H * W)
    up = torch.empty((n_img * Ho * Wo, x.shape[1]), dtype=x.dtype, device=x.device)
    ops.gather_rows(x, 0, _nearest_rows(n_img, H, W, Ho, Wo, x.device), up, 0, x.shape[1])
    return conv.tokens(up, Ho, Wo), Ho, Wo


_NEAREST_ROWS = {}


def _nearest_rows(n_img, H, W, Ho, Wo, device):
    """int32 [n_img Ho Wo]: the token of the [n_img, H, W] grid that nearest-neighbour resizing to (Ho, Wo) reads (``F.interpolate``
    with ``size=``: floor(o * H / Ho))."""
    key = (n_img, H, W, Ho, Wo, str(device))
    idx = _NEAREST_ROWS.get(key)
    if idx is None:   # (never evicted: a captured step graph reads the table it was captured with; one entry per geometry, <= 0.5 MB)
        yi = (torch.arange(Ho) * H) // Ho
        xi = (torch.arange(Wo) * W) // Wo
        one = (yi[:, None] * W + xi[None, :]).reshape(-1)
        idx = (torch.arange(n_img)[:, None] * (H * W) + one[None, :]).reshape(-1).to(device=device, dtype=torch.int32).contiguous()
        if idx.is_cuda:   # the table is shared by every stream of the process (clip pipeline: two loops, two streams): its H2D copy from
            torch.cuda.current_stream(idx.device).synchronize()   # pageable memory is complete before another stream may read it
        _NEAREST_ROWS[key] = idx
    return idx


class I2VGenXLTransformerTemporalEncoder(nn.Module):
    def __init__(self, dim, heads, dim_head, ff_inner):
        super().__init__()
        self.norm1 = LayerNorm(dim)
        self.attn1 = Attention(dim, None, heads, dim_head)
        self.ff = FeedForward(dim, ff_inner, activation_fn="gelu")


# ------------------------------------------------------------------------------------------- context
class _Ctx:
    """Per-clip state: geometry, scratch, and everything that does not depend on the timestep."""

    def __init__(self):
        self.key = None
        self.kv_slices = {}

    def kv_for(self, attn):
        c0, C = self.kv_slices[id(attn)]
        return self.kv_all[:, c0:c0 + C], self.kv_all[:, c0 + C:c0 + 2 * C], self.Sk


class _ConfigView:
    def __init__(self, cfg):
        self.in_channels = cfg.in_channels
        self.sample_size = cfg.sample_size
        self.cross_attention_dim = cfg.cross_attention_dim


_V_ONLY = os.environ.get("ANYV2V_VONLY", "1") == "1"
_NO_LN_FOLD = os.environ.get("ANYV2V_LN_FOLD", "1") != "1"   # A/B switch: LayerNorm kernel + GEMM instead of the folded form
_LN_FOLD_FF = os.environ.get("ANYV2V_LN_FOLD_FF", "0") == "1"  # also fold norm3 into the GEGLU up-projection (measured: no gain)
PAD_CIN = 64  # conv_in input channels (8) are zero-padded to one MFMA K-tile


class I2VGenXLUNet(nn.Module):
    def __init__(self, cfg: Optional[I2VGenXLUNetConfig] = None):
        super().__init__()
        cfg = cfg or I2VGenXLUNetConfig()
        self.cfg = cfg
        self.config = _ConfigView(cfg)
        boc, g, ic, ted = cfg.block_out_channels, cfg.norm_num_groups, cfg.in_channels, cfg.time_embed_dim
        hd = cfg.attention_head_dim
        self.conv_in = Conv2d(2 * ic, boc[0], 3, padding=1, pad_cin_to=PAD_CIN)
        self.transformer_in = TransformerTemporalModel(cfg.transformer_in_heads, hd, boc[0], g)
        self.image_latents_proj_in = nn.Sequential(Conv2d(4, ic * 4, 3, padding=1), SiLU(),
                                                   Conv2d(ic * 4, ic * 4, 3, padding=1), SiLU(),
                                                   Conv2d(ic * 4, ic, 3, padding=1))
        self.image_latents_temporal_encoder = I2VGenXLTransformerTemporalEncoder(ic, 2, ic, ic * 4)
        self.image_latents_context_embedding = nn.Sequential(
            Conv2d(4, ic * 8, 3, padding=1), SiLU(), Identity(),
            Conv2d(ic * 8, ic * 16, 3, stride=2, padding=1), SiLU(),
            Conv2d(ic * 16, cfg.cross_attention_dim, 3, stride=2, padding=1))
        self.time_embedding = nn.ModuleDict(dict(linear_1=Linear(boc[0], ted), linear_2=Linear(ted, ted)))
        self.context_embedding = nn.Sequential(Linear(cfg.cross_attention_dim, ted), SiLU(),
                                               Linear(ted, cfg.cross_attention_dim * ic))
        self.fps_embedding = nn.Sequential(Linear(boc[0], ted), SiLU(), Linear(ted, ted))
        self.down_blocks = nn.ModuleList()
        out = boc[0]
        for i, typ in enumerate(cfg.down_block_types):
            cin, out = out, boc[i]
            self.down_blocks.append(DownBlock3D(cfg, cin, out, typ.startswith("CrossAttn"), i != len(boc) - 1))
        self.mid_block = MidBlock3D(cfg, boc[-1])
        self.up_blocks = nn.ModuleList()
        rev = list(reversed(boc))
        out = rev[0]
        for i, typ in enumerate(cfg.up_block_types):
            prev_out, out = out, rev[i]
            cin = rev[min(i + 1, len(boc) - 1)]
            self.up_blocks.append(UpBlock3D(cfg, cin, out, prev_out, typ.startswith("CrossAttn"), i != len(boc) - 1))
        self.conv_norm_out = GroupNorm(g, boc[0], eps=1e-5)
        self.conv_act = SiLU()
        self.conv_out = Conv2d(boc[0], cfg.out_channels, 3, padding=1)
        self._packed = False
        self._pack_gen = 0  # bumped by every pack(): captured graphs point at the packed tensors of one generation
        self._ctx = _Ctx()
        self.frame_parallel = None

    def set_frame_parallel(self, fp):
        """Shard ONE clip's frames over the ranks of ``fp`` (``anyv2v_amd.parallel.FrameParallel``; None = off).  Inputs
        and outputs of ``forward`` stay full-size and replicated; only the activations are sharded."""
        if fp is not None and self.freeu is not None:
            raise NotImplementedError("FreeU is enabled: frame-parallel clips do not support it (disable_freeu() first)")
        self.frame_parallel = fp
        self._ctx = _Ctx()

    # ----------------------------------------------------------------------------------- FreeU
    def enable_freeu(self, s1, s2, b1, b2):
        """diffusers ``enable_freeu`` (arXiv 2309.11497), as the reference pipeline forwards it (``pipeline_i2vgen_xl.py:623-648``): in
        front of every skip concat of ``up_blocks[0]`` (b1, s1) and ``up_blocks[1]`` (b2, s2) the first half of the backbone's
        channels is scaled by b and the skip connection's lowest frequencies by s (``ops.freeu``); the other up blocks are untouched.
        A step engine captured before the call does not see it: ``I2VGenXLPipeline.enable_freeu`` keys its engines on ``freeu``."""
        vals = tuple(float(v) for v in (s1, s2, b1, b2))
        if not all(math.isfinite(v) for v in vals):
            raise ValueError(f"enable_freeu: s1, s2, b1, b2 = {vals} must be finite")
        if self.frame_parallel is not None:
            raise NotImplementedError("enable_freeu: not supported on a frame-parallel clip (set_frame_parallel(None) first)")
        self.up_blocks[0].freeu = (vals[2], vals[0])
        self.up_blocks[1].freeu = (vals[3], vals[1])

    def disable_freeu(self):
        for blk in self.up_blocks:
            blk.freeu = None

    @property
    def freeu(self):
        """(s1, s2, b1, b2) while FreeU is enabled, else None."""
        f0, f1 = self.up_blocks[0].freeu, self.up_blocks[1].freeu
        return None if f0 is None or f1 is None else (f0[1], f1[1], f0[0], f1[0])

    # ----------------------------------------------------------------------------------- weights
    @property
    def dtype(self):
        return self.conv_in.weight.dtype

    @property
    def device(self):
        return self.conv_in.weight.device

    def load_state_dict(self, sd, strict=True, **kw):
        r = super().load_state_dict({k: v.to(torch.float16) for k, v in sd.items()}, strict=strict, **kw)
        self._packed = False
        return r

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._packed = False
        return r

    def pack(self):
        """Re-lay weights for the kernels: conv filters -> [Cout, taps*Cin]; fused QKV / KV; GEGLU interleave;
        all time_emb_proj and all cross-attention K/V projections concatenated into one GEMM each."""
        for m in self.modules():
            if m is not self and hasattr(m, "pack"):
                m.pack()
        resnets = [m for m in self.modules() if isinstance(m, ResnetBlock2D)]
        col = 0
        ws, bs = [], []
        for r in resnets:
            r._temb_col = col
            col += r.out_channels
            ws.append(r.time_emb_proj.weight.data)
            bs.append(r.time_emb_proj.bias.data)
        self._w_temb_all = torch.cat(ws, 0).contiguous()
        self._b_temb_all = torch.cat(bs, 0).contiguous()
        cross = [m for m in self.modules() if isinstance(m, Attention) and m.is_cross]
        self._cross = cross
        self._w_kv_all = torch.cat([m._w_kv for m in cross], 0).contiguous()
        self._ctx = _Ctx()
        self._packed = True
        self._pack_gen += 1

    # ----------------------------------------------------------------------------------- conditioning
    def _prepare_clip(self, B, F, H, W, ehs, fps, image_latents, image_embeddings):
        """Everything step-invariant: computed once per clip / per set of conditioning tensors."""
        cfg = self.cfg
        dev = ehs.device
        key = (B, F, H, W, ehs.data_ptr(), ehs._version, image_latents.data_ptr(), image_latents._version,
               image_embeddings.data_ptr(), image_embeddings._version, fps.data_ptr(), fps._version)
        ctx = self._ctx
        if ctx.key == key:
            return ctx
        ctx = _Ctx()
        ctx.B, ctx.F, ctx.H, ctx.W = B, F, H, W
        ctx.fp = fp = self.frame_parallel
        if fp is not None:
            fp.check(F, H, W, len(cfg.block_out_channels))
        HW = H * W
        T = B * F * HW
        ctx.stats = torch.empty(ops.gn_scratch_floats(B * F, 1, cfg.norm_num_groups), dtype=torch.float32, device=dev)
        if ops.GN_EPILOGUE and fp is None:   # GroupNorm records of the largest launch of this engine (every level, 4-D and 5-D norms)
            g = cfg.norm_num_groups
            need = max(ops.gn_stats_floats(T, HW, g), ops.gn_stats_floats(T, F * HW, g))
            ctx.gn_rec = torch.empty(need, dtype=torch.float32, device=dev) if need > 0 else None
        ctx.t_buf = torch.zeros(B, dtype=torch.float32, device=dev)
        boc0, cd = cfg.block_out_channels[0], cfg.cross_attention_dim
        # fps embedding
        fe = ops.timestep_embedding(fps.reshape(-1).to(torch.float32).expand(B).contiguous(), boc0)
        fe = ops.gemm(fe, self.fps_embedding[0].weight, bias=self.fps_embedding[0].bias, act=ACT_SILU)
        ctx.fps_emb = ops.gemm(fe, self.fps_embedding[2].weight, bias=self.fps_embedding[2].bias)
        # context tokens: [text | first-frame latent tokens | CLIP image tokens]
        il0 = torch.empty((B * HW, 4), dtype=torch.float16, device=dev)
        ops.ncfhw_to_tokens(image_latents[:, :, :1].to(torch.float16).contiguous(), il0)
        ce = self.image_latents_context_embedding
        c = ce[0].tokens(il0, H, W, act=ACT_SILU)
        c = ops.adaptive_avgpool(c, B, H, W, 32, 32)
        c = ce[3].tokens(c, 32, 32, act=ACT_SILU)
        c = ce[5].tokens(c, 16, 16)  # [B*64, cd]
        ie = image_embeddings.reshape(B, cd).to(torch.float16).contiguous()
        e = ops.gemm(ie, self.context_embedding[0].weight, bias=self.context_embedding[0].bias, act=ACT_SILU)
        e = ops.gemm(e, self.context_embedding[2].weight, bias=self.context_embedding[2].bias)  # [B, ic*cd]
        n_txt = ehs.shape[1]
        n_il = c.shape[0] // B
        Sk = n_txt + n_il + cfg.in_channels
        ctx.Sk = Sk
        context = torch.empty((B * Sk, cd), dtype=torch.float16, device=dev)
        ehs16 = ehs.to(torch.float16).contiguous()
        for b in range(B):
            r0 = b * Sk
            ops.copy_cols(ehs16[b], 0, context[r0:r0 + n_txt], 0, cd)
            ops.copy_cols(c[b * n_il:(b + 1) * n_il], 0, context[r0 + n_txt:r0 + n_txt + n_il], 0, cd)
            ops.copy_cols(e[b].view(cfg.in_channels, cd), 0, context[r0 + n_txt + n_il:r0 + Sk], 0, cd)
        ctx.context = context
        ctx.kv_all = ops.gemm(context, self._w_kv_all)  # all 16 cross-attention K/V projections, once per clip
        col = 0
        for m in self._cross:
            ctx.kv_slices[id(m)] = (col, m.inner_dim)
            col += 2 * m.inner_dim
        # image-latents branch -> channels 4..7 of the conv_in input
        il = torch.empty((T, 4), dtype=torch.float16, device=dev)
        ops.ncfhw_to_tokens(image_latents.to(torch.float16).contiguous(), il)
        pi = self.image_latents_proj_in
        h = pi[0].tokens(il, H, W, act=ACT_SILU)
        h = pi[2].tokens(h, H, W, act=ACT_SILU)
        h = pi[4].tokens(h, H, W)
        enc = self.image_latents_temporal_encoder
        a = enc.attn1
        n = ops.layernorm(h, enc.norm1.weight, enc.norm1.bias, enc.norm1.eps)
        qkv = ops.gemm(n, a._w_qkv)
        Cq = a.inner_dim
        o = torch.empty((T, Cq), dtype=torch.float16, device=dev)
        geom = Geom("temporal", B, F, HW)
        ops.attention(qkv[:, :Cq], qkv[:, Cq:2 * Cq], qkv[:, 2 * Cq:], o, batch=geom.batch, heads=a.heads, Sq=F, Sk=F,
                      inner=geom.inner, q_strides=geom.strides, kv_strides=geom.strides, scale=a.scale,
                      head_dim=a.dim_head)
        h = ops.gemm(o, a.to_out[0].weight, bias=a.to_out[0].bias, residual=h)
        h = enc.ff.run(h, residual=h)
        if fp is not None:
            # frame-parallel clip: the (cheap, <= 16-channel) image-latents branch above ran replicated on all frames
            # because its temporal encoder attends over them; from here on this rank owns frames [f0, f1)
            f0, f1 = fp.frames(F)
            h = h.view(B, F, HW, -1)[:, f0:f1].reshape(B * (f1 - f0) * HW, -1).contiguous()
            ctx.F, T = f1 - f0, B * (f1 - f0) * HW
        ctx.xin = torch.zeros((T, PAD_CIN), dtype=torch.float16, device=dev)
        ops.copy_cols(h, 0, ctx.xin, cfg.in_channels, cfg.in_channels)
        ctx.key = key
        ctx._keepalive = (ehs, image_latents, image_embeddings, fps)  # pin the tensors the key points at
        ctx.shared_stem = False   # set by the pipeline for the PnP edit batch (see _forward_core)
        ctx.stem_ctx = copy.copy(ctx)  # same buffers, one batch element fewer: geometry of the shared stem
        ctx.stem_ctx.B = max(B - 1, 1)
        self._ctx = ctx
        return ctx

    # ----------------------------------------------------------------------------------- forward
    def forward_tokens(self, sample, timestep, fps, image_latents, image_embeddings, encoder_hidden_states):
        """Returns the channels-last v-prediction [(B F) H W, 8] (columns 0..3 valid)."""
        if not self._packed:
            self.pack()
        B, C, F, H, W = sample.shape
        ctx = self._prepare_clip(B, F, H, W, encoder_hidden_states, fps, image_latents, image_embeddings)
        if torch.is_tensor(timestep):
            ctx.t_buf.copy_(timestep.reshape(-1).to(torch.float32).expand(B), non_blocking=True)
        else:
            ctx.t_buf.fill_(float(timestep))
        return self._forward_core(ctx, sample)

    def _forward_core(self, ctx, sample, drop_source_tail=False):
        """One UNet evaluation given a prepared clip context and ``ctx.t_buf`` (device timestep): pure function of
        (sample, t) -- this is what the pipeline captures into a HIP graph.  ``drop_source_tail`` (PnP step engine only): the
        prediction of batch element 0 is not needed -- the rows of [1:] are returned, see below."""
        cfg = self.cfg
        B, C, F, H, W = sample.shape
        fp = ctx.fp
        if fp is not None:  # frame-parallel clip: this rank's frames of the (replicated, 4-channel) latents
            f0, f1 = fp.frames(F)
            sample, F = sample[:, :, f0:f1].contiguous(), f1 - f0
        # time embedding (+ fps) -> SiLU -> all 22 time_emb_proj at once
        te = ops.timestep_embedding(ctx.t_buf, cfg.block_out_channels[0])
        te = ops.gemm(te, self.time_embedding["linear_1"].weight, bias=self.time_embedding["linear_1"].bias, act=ACT_SILU)
        emb = ops.gemm(te, self.time_embedding["linear_2"].weight, bias=self.time_embedding["linear_2"].bias,
                       residual=ctx.fps_emb)
        ctx.temb_all = ops.gemm(ops.silu(emb), self._w_temb_all, bias=self._b_temb_all)
        ctx.stem_ctx.temb_all = ctx.temb_all
        ctx.emb = emb   # [B, 1280] time + fps embedding (what a replaced ResNet forward receives as temb)
        ctx.stem_ctx.emb = emb[:ctx.stem_ctx.B]
        # stem.  With ``ctx.shared_stem`` (CFG batches [.., negative, positive]: the last two share latent, image latents,
        # fps and timestep and differ only in the cross-attention context) everything up to the first cross-attention
        # -- conv_in, transformer_in, the first ResNet / temporal-conv / self-attention of down_blocks[0] -- runs
        # once for the pair and is expanded where the branches start to differ (exact).
        stem = ctx.stem_ctx if (getattr(ctx, "shared_stem", False) and B >= 2 and self.down_blocks[0].has_cross_attention) else None
        # batch hint (ops.batch_hint; set by a step engine that runs a subset of another engine's branches, e.g. (3, 2)): the
        # shared stem holds one branch less on both sides -- (2, 1) -- until the first transformer block expands it
        hint = getattr(ctx, "batch_hint", None)
        ctx.stem_ctx.batch_hint_after = None
        if hint is not None:
            ctx.stem_ctx.batch_hint_after = hint if stem is not None else None
            ops.set_batch_hint(*((hint[0] - 1, hint[1] - 1) if stem is not None else hint))
        if stem is not None:
            T2 = (B - 1) * F * H * W
            ops.ncfhw_to_tokens(sample[:B - 1], ctx.xin[:T2], col0=0)
            x = self.conv_in.tokens(ctx.xin[:T2], H, W)
            x = self.transformer_in.run(stem, x, H, W)
            skips = [expand_shared(x, ctx)]
        else:
            ops.ncfhw_to_tokens(sample, ctx.xin, col0=0)
            x = self.conv_in.tokens(ctx.xin, H, W)
            x = self.transformer_in.run(ctx, x, H, W)
            skips = [x]
        h_, w_ = H, W
        sizes = [(H, W)]      # per resolution level; the up path returns to exactly these (odd sizes round up on the way down)
        for bi, blk in enumerate(self.down_blocks):
            x, outs, h_, w_ = blk.run(ctx, x, h_, w_, stem_ctx=stem if bi == 0 else None)
            skips.extend(outs)
            if blk.downsamplers is not None:
                sizes.append((h_, w_))
        x = self.mid_block.run(ctx, x, h_, w_)
        # PnP step whose source-branch prediction is discarded (pipeline_i2vgen_xl.py:1136,1160-1162): behind the last hook site --
        # the self-attention of up_blocks[3].temp_attentions[2] -- the source rows are dead; the rest of the forward runs on
        # [negative, editing] only and returns their 2 x F x HW rows (exact)
        last = self.up_blocks[-1].temp_attentions[-1] if getattr(self.up_blocks[-1], "has_cross_attention", False) else None
        drop = bool(drop_source_tail and B == 3 and fp is None and hint is None and last is not None)
        ctx.drop_tail_at = last if drop else None
        try:   # (the last hook site switches the process-global batch hint to (3, 2): restore it on EVERY exit)
            for blk in self.up_blocks:
                sizes.pop()
                x, h_, w_ = blk.run(ctx, x, skips, h_, w_, out_hw=sizes[-1] if sizes else None)
            ctx.drop_tail_at = None
            x = ops.groupnorm(x, self.conv_norm_out.weight, self.conv_norm_out.bias, ctx.stats, H * W,
                              groups=self.conv_norm_out.num_groups, eps=self.conv_norm_out.eps, silu=True)
            vtok = torch.empty((x.shape[0], 8), dtype=torch.float16, device=x.device)
            self.conv_out.tokens(x, H, W, out=vtok)
            if fp is not None:
                vtok = fp.gather_frames(vtok, B, F, H * W)  # every rank steps the full latents (identically)
        finally:
            ctx.drop_tail_at = None
            if drop:
                ops.set_batch_hint(1, 1)
        return vtok

    def forward(self, sample, timestep, fps=None, image_latents=None, image_embeddings=None,
                encoder_hidden_states=None, cross_attention_kwargs=None, return_dict=False):
        """Seam B3: ``unet(latent_model_input, t, encoder_hidden_states=, fps=, image_latents=, image_embeddings=,
        cross_attention_kwargs=, return_dict=False)[0]`` (``pipeline_i2vgen_xl.py:1146-1155``)."""
        B, C, F, H, W = sample.shape
        vtok = self.forward_tokens(sample.to(torch.float16).contiguous(), timestep, fps, image_latents, image_embeddings,
                                   encoder_hidden_states)
        out = ops.tokens_to_ncfhw(vtok, B, self.cfg.out_channels, F, H, W)
        return (out,)
