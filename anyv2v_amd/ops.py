"""Thin torch-tensor -> C-ABI wrappers.  Torch is plumbing only (device memory + current stream)."""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional

import torch

from . import _lib
from ._lib import AttnDesc, GemmDesc

MODE_LINEAR, MODE_CONV2D, MODE_TEMPORAL = 0, 1, 2
ACT_NONE, ACT_SILU, ACT_GELU, ACT_GEGLU, ACT_F32OUT = 0, 1, 2, 3, 4

# global knobs (tests flip them to cross-check kernel variants)
FORCE_NAIVE = False   # route GEMM / attention through the reference-grade kernels
ATTN_FLAGS = int(os.environ.get("ANYV2V_ATTN_FLAGS", "0"))  # bit1 (2): no short kernel; bit3 (8): PnP launches as per-branch aliasing (no shared-softmax kernel)
GEMM_FLAGS = int(os.environ.get("ANYV2V_GEMM_FLAGS", "0"))  # an integer of _lib.ANYV2V_GEMM_* bits (include/anyv2v_hip.h), e.g. 4: NO_BIG, 16: NO_SPLITK
USE_GLDS = os.environ.get("ANYV2V_GLDS", "1") == "1"   # LDS-DMA (global_load_lds) staging variant of the GEMM


def _parse_switch(value: Optional[str]) -> bool:
    return (value or "0").strip() == "1"


# A/B switch, off by default: GroupNorm statistics from the producing GEMM's epilogue (gemm(..., gn=...) + groupnorm_from_stats)
# for conv1 -> norm2 of ResnetBlock2D and conv i -> norm i + 1 of TemporalConvLayer, where the library's query says the plan can
GN_EPILOGUE = _parse_switch(os.environ.get("ANYV2V_GN_EPILOGUE"))


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def _p(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _rowmajor(t: torch.Tensor, name: str):
    assert t.dim() == 2 and t.stride(1) == 1, f"{name}: need a 2-D row-major (stride(1)==1) fp16 view, got {tuple(t.shape)} {t.stride()}"
    assert t.dtype == torch.float16, f"{name}: fp16 expected, got {t.dtype}"
    assert t.is_cuda, f"{name}: device tensor expected"


_WS = {}
WS_SLOT = 0   # callers that enqueue on several streams at once (two step engines side by side) give each stream its own scratch


class workspace_slot:
    """``with ops.workspace_slot(k):`` -- the launches enqueued inside use scratch buffer ``k`` (re-entrant, host-side)."""

    def __init__(self, slot: int):
        self.slot, self.prev = int(slot), 0

    def __enter__(self):
        global WS_SLOT
        self.prev, WS_SLOT = WS_SLOT, self.slot
        return self

    def __exit__(self, *exc):
        global WS_SLOT
        WS_SLOT = self.prev
        return False


def _workspace(device) -> torch.Tensor:
    """Persistent fp32 scratch for split-K partial tiles and stream-K slabs (128 MiB per device and slot -- the split-K rules keep
    planning against 64 MiB, the stream-K form needs 126 MB; allocated once, outside any graph capture because the first GEMM of a
    process always runs eagerly during warm-up)."""
    key = f"{device}:{WS_SLOT}"
    if key not in _WS:
        _WS[key] = torch.empty(32 * 1024 * 1024, dtype=torch.float32, device=device)
    return _WS[key]


def gemm(a0: torch.Tensor, w: torch.Tensor, *, a1: Optional[torch.Tensor] = None, bias=None, rowvec=None,
         rowvec_div: int = 0, residual=None, act: int = ACT_NONE, out: Optional[torch.Tensor] = None,
         mode: int = MODE_LINEAR, conv=None, temporal=None, M: Optional[int] = None, naive: bool = False, ln=None, gn=None,
         _query: bool = False):
    """out[M, N'] = epilogue(gather(A) @ W^T).  ``w`` is [N, taps*K] packed (see anyv2v_hip.h).

    ``gn`` = (stats fp32, rows_per_group, groups): the launch also writes the GroupNorm records of its stored output into ``stats``
    for ``groupnorm_from_stats`` (``gn_stats_floats(M, rows_per_group, groups)`` floats).  Only where ``gemm_gn_stats_floats`` --
    same arguments -- answers > 0; anywhere else the launch is an error, not a fallback.

    ``ln`` = (c1 fp32 [N], eps): LayerNorm folded into the projection -- ``a0`` holds the un-normalised rows, ``w`` / ``bias`` the
    gamma- / beta-folded weights (``ln_fold``); only shapes ``ln_gemm_supported`` accepts.

    conv = (Hi, Wi, Ho, Wo, stride, up[, asym]) for MODE_CONV2D; temporal = (F, HW) for MODE_TEMPORAL.
    ``M`` overrides the row count (output rows); A may have a different number of rows for convs.
    """
    lib = _lib.load()
    _rowmajor(a0, "A0")
    _rowmajor(w, "W")
    C0 = a0.shape[1]
    C1 = 0
    if a1 is not None:
        _rowmajor(a1, "A1")
        C1 = a1.shape[1]
    taps = 1 if mode == MODE_LINEAR else (9 if mode == MODE_CONV2D else 3)
    N = w.shape[0]
    assert w.shape[1] == taps * (C0 + C1), f"W is {tuple(w.shape)}, expected [{N}, {taps}*({C0}+{C1})]"
    assert w.stride(0) == w.shape[1], "W must be contiguous"
    if M is None:
        M = a0.shape[0]
    n_out = N // 2 if act == ACT_GEGLU else N
    if _query and out is None:
        pass   # the query plans without an output buffer (fresh allocations are 16-byte aligned)
    elif act == ACT_F32OUT:  # raw fp32 accumulator (+bias) -> float32 matrix
        if out is None:
            out = torch.empty((M, n_out), dtype=torch.float32, device=a0.device)
        assert out.dim() == 2 and out.stride(1) == 1 and out.dtype == torch.float32 and out.is_cuda
        assert rowvec is None and residual is None
    else:
        if out is None:
            out = torch.empty((M, n_out), dtype=torch.float16, device=a0.device)
        _rowmajor(out, "C")
    assert out is None or (out.shape[0] >= M and out.shape[1] >= n_out)
    d = GemmDesc()
    d.A0, d.A1, d.W, d.C = _p(a0), _p(a1), _p(w), _p(out)
    d.bias, d.rowvec, d.R = _p(bias), _p(rowvec), _p(residual)
    d.M, d.N, d.C0, d.C1 = M, N, C0, C1
    d.lda0 = a0.stride(0)
    d.lda1 = a1.stride(0) if a1 is not None else 0
    d.ldc = out.stride(0) if out is not None else n_out
    d.ldr = residual.stride(0) if residual is not None else 0
    d.ldrv = rowvec.stride(0) if rowvec is not None else 0
    d.rowvec_div = rowvec_div
    d.mode = mode
    if mode == MODE_CONV2D:
        d.Hi, d.Wi, d.Ho, d.Wo, d.stride, d.up = conv[:6]
        d.asym = conv[6] if len(conv) > 6 else 0  # 1: pad only right / bottom (AutoencoderKL Downsample2D)
    elif mode == MODE_TEMPORAL:
        d.F, d.HW = temporal
    d.act = act
    d.flags = ((_lib.ANYV2V_GEMM_NAIVE if (naive or FORCE_NAIVE) else 0) | (_lib.ANYV2V_GEMM_LDS_DMA if USE_GLDS else 0)
               | GEMM_FLAGS)
    if ln is not None:
        c1, eps = ln
        assert c1.dtype == torch.float32 and c1.is_cuda and c1.numel() >= N and c1.is_contiguous()
        d.ln_c1, d.ln_eps = _p(c1), float(eps)
    ws = _workspace(a0.device)
    d.workspace, d.workspace_bytes = ws.data_ptr(), ws.numel() * 4
    if gn is not None:
        stats, rows_per_group, groups = gn
        d.gn_rows_per_group, d.gn_groups = int(rows_per_group), int(groups)
        if stats is not None:
            assert stats.dtype == torch.float32 and stats.is_cuda and stats.is_contiguous()
            d.gn_stats, d.gn_stats_floats = stats.data_ptr(), stats.numel()
    if _query:
        return int(lib.anyv2v_gemm_gn_stats_floats(C.byref(d)))
    _lib.check(lib.anyv2v_gemm_f16(C.byref(d), _stream()), "anyv2v_gemm_f16")
    return out


def gemm_gn_stats_floats(a0: torch.Tensor, w: torch.Tensor, *, rows_per_group: int, groups: int = 32, **kw) -> int:
    """Floats of records ``gemm(a0, w, gn=(stats, rows_per_group, groups), **kw)`` would write, or 0 when the plan that launch gets
    cannot emit them (``anyv2v_gemm_gn_stats_floats``: split-K, naive, GEGLU, ...).  Same arguments as the launch, the batch hint
    in force included; launches nothing, so a host can choose before a graph capture."""
    return gemm(a0, w, gn=(None, rows_per_group, groups), _query=True, **kw)


def gn_launches(reset: bool = True) -> int:
    """GEMM launches that emitted GroupNorm records since the last reset (counted at enqueue time; for tests)."""
    return int(_lib.load().anyv2v_gemm_gn_launches(int(reset)))


def gn_stats_floats(M: int, rows_per_group: int, groups: int = 32) -> int:
    """Size of the record buffer shared by ``gemm(gn=...)`` and ``groupnorm_from_stats`` (== anyv2v_groupnorm_stats_floats): one
    3-float record per (16 rows, channel group), plus room to pre-fold statistics groups of more than 256 records."""
    return int(_lib.load().anyv2v_groupnorm_stats_floats(int(M), int(rows_per_group), int(groups)))


def groupnorm_from_stats(x: torch.Tensor, gamma, beta, stats: torch.Tensor, rows_per_group: int, *, groups: int = 32,
                         eps: float = 1e-5, silu: bool = False, out=None):
    """GroupNorm (+ SiLU) of ``x`` from the records the GEMM that produced ``x`` wrote into ``stats``: no statistics pass over
    ``x``.  Single source."""
    lib = _lib.load()
    _rowmajor(x, "X")
    assert x.is_contiguous()
    M, Cc = x.shape
    if out is None:
        out = torch.empty((M, Cc), dtype=torch.float16, device=x.device)
    assert out.is_contiguous()
    assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() >= gn_stats_floats(M, rows_per_group, groups) > 0
    sizes = (C.c_int32 * 5)(M, Cc, rows_per_group, groups, min(stats.numel(), 2 ** 31 - 1))
    _lib.check(lib.anyv2v_groupnorm_apply_stats_f16(_p(x), _p(out), _p(gamma), _p(beta), _p(stats), sizes, eps, int(silu),
                                                    _stream()), "anyv2v_groupnorm_apply_stats_f16")
    return out


FF_FUSED = os.environ.get("ANYV2V_FF_FUSED", "1") == "1"   # A/B switch: fused feed-forward kernel (ff_fused.hip) vs GEGLU GEMM + Linear


def ff_fused_supported(M: int, C: int, H: int) -> bool:
    """Shapes the fused feed-forward kernel covers AND pays on: the 320-channel transformer blocks at the 64x64 level's row counts
    (same threshold, on hinted rows, as the weight-stationary GEMMs it replaces)."""
    return FF_FUSED and not FORCE_NAIVE and USE_GLDS and C == 320 and H == 1280 and M * _HINT[0] // _HINT[1] >= 32768


def ff_pack_w2(w2: torch.Tensor) -> torch.Tensor:
    """``Linear(H, C).weight`` [C, H] -> the fused kernel's layout [H / 32][C][32]: slab-major, and inside a slab of 32 hidden units
    column 8 q + e holds hidden unit 4 q + e (e < 4) or 16 + 4 q + (e - 4) (e >= 4) -- the MFMA K-slot order in which the kernel's
    GEGLU registers already hold the hidden values (include/anyv2v_hip.h, AnyV2VFFDesc)."""
    C, H = w2.shape
    assert H % 32 == 0
    q, e = torch.arange(4).view(4, 1), torch.arange(8).view(1, 8)
    perm = torch.where(e < 4, 4 * q + e, 16 + 4 * q + (e - 4)).reshape(32).to(w2.device)   # slot -> hidden unit of the slab
    return w2.view(C, H // 32, 32)[:, :, perm].permute(1, 0, 2).contiguous()


def ff_geglu(x: torch.Tensor, w1p: torch.Tensor, b1p: torch.Tensor, w2s: torch.Tensor, b2: torch.Tensor, residual=None, out=None):
    """y = GEGLU(x W1^T + b1) W2^T + b2 (+ residual) in one kernel (``anyv2v_ff_geglu_f16``); ``w1p`` / ``b1p`` as ``GEGLU.pack``
    interleaves them, ``w2s`` from ``ff_pack_w2``."""
    lib = _lib.load()
    M, Cc = x.shape
    H = w2s.shape[0] * 32
    assert x.dtype == torch.float16 and x.stride(1) == 1 and w1p.is_contiguous() and w2s.is_contiguous()
    assert tuple(w1p.shape) == (2 * H, Cc) and tuple(w2s.shape) == (H // 32, Cc, 32) and b1p.numel() == 2 * H and b2.numel() == Cc
    if out is None:
        out = torch.empty((M, Cc), dtype=torch.float16, device=x.device)
    for name, t in (("residual", residual), ("out", out)):   # the kernel reads / writes them as 8-byte vectors at row * ld + column
        assert t is None or (tuple(t.shape) == (M, Cc) and t.dtype == torch.float16 and t.stride(1) == 1 and t.device == x.device), \
            f"ff_geglu: {name} must be an fp16 [{M}, {Cc}] matrix with unit column stride on {x.device}"
    d = _lib.FFDesc()
    d.X, d.W1, d.b1, d.W2, d.b2, d.Y = _p(x), _p(w1p), _p(b1p), _p(w2s), _p(b2), _p(out)
    d.R = _p(residual) if residual is not None else None
    d.M, d.C, d.H = M, Cc, H
    d.ldx, d.ldy, d.ldr = x.stride(0), out.stride(0), (residual.stride(0) if residual is not None else 0)
    d.flags = d.reserved0 = 0
    _lib.check(lib.anyv2v_ff_geglu_f16(C.byref(d), _stream()), "anyv2v_ff_geglu_f16")
    return out


def ln_gemm_supported(M: int, K: int, N: int, act: int = ACT_NONE, hinted: bool = True) -> bool:
    """Shapes for which ``gemm(..., ln=...)`` runs (the weight-stationary kernel, gemm_ws.hip) AND pays: the 64x64 level's row
    counts.  Mirrors the library's own check; everything else runs ``layernorm`` + ``gemm``.  ``hinted=False``: ``M`` is already a
    canonical row count (one branch's rows) and is compared as it is, whatever batch hint is in force."""
    if FORCE_NAIVE or not USE_GLDS or (GEMM_FLAGS & (_lib.ANYV2V_GEMM_NO_WS | _lib.ANYV2V_GEMM_NO_BIG)) or (M * _HINT[0] // _HINT[1] if hinted else M) < 32768:
        return False
    if K == 320:
        return N % 160 == 0 and N // 160 <= 32
    return K == 512 and act == ACT_GEGLU and N % 128 == 0 and N // 128 <= 32


def ln_fold(w: torch.Tensor, bias: Optional[torch.Tensor], gamma: torch.Tensor, beta: torch.Tensor):
    """(W', b', c1) of LN(x) W^T + b = rstd (x W'^T - mean c1) + b':  W' = W diag(gamma) rounded to fp16, c1 = row sums of that
    ROUNDED W' in fp32 (so that x W'^T - mean c1 is exactly the product of the centred row with the weights the kernel multiplies
    by: no cancellation error from the rounding), b' = b + W beta."""
    wf = w.float() * gamma.float()[None, :]
    w16 = wf.to(torch.float16).contiguous()
    c1 = w16.float().sum(1).contiguous()
    b = w.float() @ beta.float()
    if bias is not None:
        b = b + bias.float()
    return w16, b.to(torch.float16).contiguous(), c1


def gn_scratch_floats(M: int, rows_per_group: int, groups: int = 32) -> int:
    """Size of the ``stats`` scratch of ``groupnorm`` (== anyv2v_groupnorm_scratch_floats): any plan's partial sums, and the pivots of
    the sharded form behind them."""
    return int(_lib.load().anyv2v_groupnorm_scratch_floats(int(M), int(rows_per_group), int(groups)))


def _gn_operands(x0, x1, out):
    """(M, C0, C1, out) of a GroupNorm call over [x0 | x1]: the operand checks, and the output where none was handed over."""
    _rowmajor(x0, "X0")
    assert x0.is_contiguous()
    M, C0 = x0.shape
    C1 = 0
    if x1 is not None:
        _rowmajor(x1, "X1")
        assert x1.is_contiguous() and x1.shape[0] == M
        C1 = x1.shape[1]
    if out is None:
        out = torch.empty((M, C0 + C1), dtype=torch.float16, device=x0.device)
    assert out.is_contiguous()
    return M, C0, C1, out


def groupnorm(x0: torch.Tensor, gamma, beta, stats: torch.Tensor, rows_per_group: int, *, x1=None, groups: int = 32,
              eps: float = 1e-5, silu: bool = False, out=None, shard=None):
    """``shard`` = (shards, all_reduce_sum): this rank holds 1/shards of every statistics group (frame- / pixel-parallel
    clip, ``anyv2v_amd.parallel.FrameParallel``).  ``all_reduce_sum`` is called twice, in the same order on every rank: on the
    ranks' pivots / shards (the agreed pivot of the shifted sums), then on the partial sums about that pivot."""
    if shard is not None:
        return _groupnorm_sharded(x0, gamma, beta, stats, rows_per_group, x1, groups, eps, silu, out, shard)
    lib = _lib.load()
    M, C0, C1, out = _gn_operands(x0, x1, out)
    need = gn_scratch_floats(M, rows_per_group, groups)
    assert stats.dtype == torch.float32 and stats.numel() >= need, "GroupNorm scratch too small"
    _lib.check(lib.anyv2v_groupnorm_f16(_p(x0), _p(x1), C0, C1, _p(out), _p(gamma), _p(beta), _p(stats), M,
                                        rows_per_group, groups, eps, int(silu), _stream()), "anyv2v_groupnorm_f16")
    return out


def _groupnorm_sharded(x0, gamma, beta, stats, rows_per_group, x1, groups, eps, silu, out, shard):
    lib = _lib.load()
    shards, all_reduce_sum = shard
    M, C0, C1, out = _gn_operands(x0, x1, out)
    n = int(lib.anyv2v_groupnorm_partial_floats(M, rows_per_group, groups, C0 + C1))
    npiv = (M // rows_per_group) * groups
    assert n > 0 and stats.dtype == torch.float32 and stats.numel() >= n + npiv, "GroupNorm scratch too small"
    piv = stats[n:n + npiv]   # behind the partial sums (a gn_scratch_floats() buffer has room for both: tests/test_norm_plan_host.py)
    _lib.check(lib.anyv2v_groupnorm_pivot_f16(_p(x0), _p(x1), C0, C1, _p(piv), M, rows_per_group, groups, int(shards), _stream()),
               "anyv2v_groupnorm_pivot_f16")
    all_reduce_sum(piv)
    _lib.check(lib.anyv2v_groupnorm_partial_pivot_f16(_p(x0), _p(x1), C0, C1, _p(piv), _p(stats), M, rows_per_group, groups,
                                                      _stream()), "anyv2v_groupnorm_partial_pivot_f16")
    all_reduce_sum(stats[:n])
    _lib.check(lib.anyv2v_groupnorm_apply_pivot_f16(_p(x0), _p(x1), C0, C1, _p(out), _p(gamma), _p(beta), _p(piv), _p(stats), M,
                                                    rows_per_group, groups, eps, int(silu), int(shards), _stream()),
               "anyv2v_groupnorm_apply_pivot_f16")
    return out


def layernorm(x: torch.Tensor, gamma, beta, eps: float = 1e-5, out=None):
    lib = _lib.load()
    _rowmajor(x, "X")
    assert x.is_contiguous()
    M, Cc = x.shape
    if out is None:
        out = torch.empty_like(x)
    _lib.check(lib.anyv2v_layernorm_f16(_p(x), _p(out), _p(gamma), _p(beta), M, Cc, eps, _stream()), "anyv2v_layernorm_f16")
    return out


def softmax_rows(s: torch.Tensor, scale: float, out: Optional[torch.Tensor] = None):
    """fp32 logits [rows, cols] -> fp16 softmax(scale * s) (row-wise)."""
    lib = _lib.load()
    assert s.dim() == 2 and s.stride(1) == 1 and s.dtype == torch.float32 and s.is_cuda
    rows, cols = s.shape
    if out is None:
        out = torch.empty((rows, cols), dtype=torch.float16, device=s.device)
    _rowmajor(out, "P")
    _lib.check(lib.anyv2v_softmax_rows_f32_f16(_p(s), s.stride(0), _p(out), out.stride(0), rows, cols, float(scale), _stream()),
               "anyv2v_softmax_rows_f32_f16")
    return out


def attention_entry(head_dim, causal, has_bias):
    """The entry point ``attention`` calls: 2 = ``anyv2v_attention_bias_f16`` (a bias), 0 = ``anyv2v_attention_f16`` (head_dim 64 without the
    causal mask), 1 = ``anyv2v_attention_small_f16`` (anything else).  The numbers are the planner's (csrc/attention_plan.h: AttnEntry)."""
    if has_bias:
        return 2
    return 0 if head_dim == 64 and not causal else 1


def attention(q, k, v, out, *, batch, heads, Sq, Sk, inner=1, q_strides, kv_strides, kv_div=1, qk_mod=0,
              scale=0.125, head_dim=64, naive=False, causal=False, bias=None):
    """Strided multi-head attention over token matrices; see anyv2v_hip.h for the addressing.  ``causal`` (CLIP text tower)
    and head_dim != 64 run on the small generic kernel; ``bias`` (fp32 [heads, Sq, Sk], added to the scaled scores) on the
    generic one."""
    lib = _lib.load()
    for t, n in ((q, "Q"), (k, "K"), (v, "V"), (out, "O")):
        _rowmajor(t, n)
    d = AttnDesc()
    d.Q, d.K, d.V, d.O = _p(q), _p(k), _p(v), _p(out)
    d.ldq, d.ldk, d.ldv, d.ldo = q.stride(0), k.stride(0), v.stride(0), out.stride(0)
    d.batch, d.heads, d.Sq, d.Sk, d.inner = batch, heads, Sq, Sk, inner
    d.q_outer, d.q_inner, d.q_seq = q_strides
    d.kv_outer, d.kv_inner, d.kv_seq = kv_strides
    d.kv_div, d.qk_mod, d.scale = kv_div, qk_mod, scale
    d.flags = (1 if (naive or FORCE_NAIVE) else 0) | ATTN_FLAGS | (16 if causal else 0)
    entry = attention_entry(head_dim, causal, bias is not None)
    if entry == 2:
        assert bias.dtype == torch.float32 and bias.is_contiguous() and tuple(bias.shape) == (heads, Sq, Sk) and bias.device == q.device
        _lib.check(lib.anyv2v_attention_bias_f16(C.byref(d), head_dim, _p(bias), _stream()), "anyv2v_attention_bias_f16")
    elif entry == 0:
        _lib.check(lib.anyv2v_attention_f16(C.byref(d), _stream()), "anyv2v_attention_f16")
    else:
        _lib.check(lib.anyv2v_attention_small_f16(C.byref(d), head_dim, _stream()), "anyv2v_attention_small_f16")
    return out


# A/B switch: temporal self-attention with its QKV projection inside (tattn_fused.hip) vs the LayerNorm-folded QKV GEMM + attention
TATTN_FUSED_DEFAULT = "1"


def tattn_fused_enabled() -> bool:
    """ANYV2V_TATTN_FUSED, read when asked (a test or an A/B run flips it without re-importing the package)."""
    return os.environ.get("ANYV2V_TATTN_FUSED", TATTN_FUSED_DEFAULT).strip() == "1"


TATTN_MIN_ROWS = 32768   # rows of one branch from which the LayerNorm-folded weight-stationary GEMM is taken (csrc/tattn_plan.h)


def temporal_qkv_attn_supported(rows_per_branch: int, C: int, heads: int, F: int, HW: int, x: Optional[torch.Tensor] = None) -> bool:
    """Where ``temporal_qkv_attn`` stands for ``gemm(x, W', bias=b', ln=...)`` + ``attention`` (bit-equal) AND pays: the plan of
    csrc/tattn_plan.cpp (16 frames, 320 channels = 5 heads of 64, even HW) from the row count at which the two launches take the
    weight-stationary path.  ``rows_per_branch``: the rows of ONE batch element (F * HW), as ``_fold(..., per_branch=True)`` sees
    them -- every engine decides alike whatever batch it runs.  ``x``: the operand; a tensor off the GPU says no."""
    if not tattn_fused_enabled() or FORCE_NAIVE or not USE_GLDS or (x is not None and not x.is_cuda):
        return False
    if GEMM_FLAGS & (_lib.ANYV2V_GEMM_NO_WS | _lib.ANYV2V_GEMM_NO_BIG) or ATTN_FLAGS & 3:   # the two launches would not be the ones it equals
        return False
    return (F == 16 and C == 320 and heads == 5 and HW > 0 and HW % 2 == 0 and rows_per_branch == F * HW
            and rows_per_branch >= TATTN_MIN_ROWS)


def temporal_qkv_attn(x: torch.Tensor, w: torch.Tensor, bias: torch.Tensor, c1: torch.Tensor, eps: float, *, B: int, F: int, HW: int,
                      heads: int, scale: float = 0.125, out: Optional[torch.Tensor] = None):
    """out[(b f) hw, C] = temporal attention of QKV = LN-folded ``x`` W'^T + b' (``ln_fold`` operands, W' = [Wq; Wk; Wv] diag(gamma))
    in one kernel (``anyv2v_temporal_qkv_attn_f16``): the QKV tensor is never written.  Shapes outside the kernel's coverage are an
    error, not a fallback -- ask ``temporal_qkv_attn_supported`` first."""
    lib = _lib.load()
    _rowmajor(x, "X")
    _rowmajor(w, "W")
    Cc = x.shape[1]
    assert x.shape[0] == B * F * HW and tuple(w.shape) == (3 * Cc, Cc) and w.is_contiguous()
    assert bias is not None and bias.dtype == torch.float16 and bias.is_cuda and bias.numel() == 3 * Cc and bias.is_contiguous()
    assert c1.dtype == torch.float32 and c1.is_cuda and c1.numel() == 3 * Cc and c1.is_contiguous()
    if out is None:
        out = torch.empty((x.shape[0], Cc), dtype=torch.float16, device=x.device)
    _rowmajor(out, "O")
    assert out.shape[0] == x.shape[0] and out.shape[1] == Cc
    d = _lib.TattnDesc()
    d.X, d.W, d.bias, d.ln_c1, d.O = _p(x), _p(w), _p(bias), _p(c1), _p(out)
    d.B, d.F, d.HW, d.C, d.heads = B, F, HW, Cc, heads
    d.ldx, d.ldo = x.stride(0), out.stride(0)
    d.ln_eps, d.scale, d.flags = float(eps), float(scale), 0
    _lib.check(lib.anyv2v_temporal_qkv_attn_f16(C.byref(d), _stream()), "anyv2v_temporal_qkv_attn_f16")
    return out


def silu(x: torch.Tensor, out=None):
    lib = _lib.load()
    assert x.is_contiguous() and x.dtype == torch.float16
    if out is None:
        out = torch.empty_like(x)
    _lib.check(lib.anyv2v_silu_f16(_p(x), _p(out), x.numel(), _stream()), "anyv2v_silu_f16")
    return out


def add(a: torch.Tensor, b: torch.Tensor, out=None):
    lib = _lib.load()
    assert a.is_contiguous() and b.is_contiguous() and a.numel() == b.numel()
    if out is None:
        out = torch.empty_like(a)
    _lib.check(lib.anyv2v_add_f16(_p(a), _p(b), _p(out), a.numel(), _stream()), "anyv2v_add_f16")
    return out


def timestep_embedding(t_f32: torch.Tensor, dim: int, out=None):
    lib = _lib.load()
    assert t_f32.dtype == torch.float32 and t_f32.is_contiguous()
    B = t_f32.numel()
    if out is None:
        out = torch.empty((B, dim), dtype=torch.float16, device=t_f32.device)
    _lib.check(lib.anyv2v_timestep_embedding_f16(_p(t_f32), _p(out), B, dim, _stream()), "anyv2v_timestep_embedding_f16")
    return out


def ncfhw_to_tokens(x: torch.Tensor, out: torch.Tensor, col0: int = 0):
    lib = _lib.load()
    B, Cc, F, H, W = x.shape
    assert x.is_contiguous() and x.dtype == torch.float16
    _rowmajor(out, "Y")
    _lib.check(lib.anyv2v_ncfhw_to_tokens_f16(_p(x), _p(out), B, Cc, F, H * W, out.stride(0), col0, _stream()),
               "anyv2v_ncfhw_to_tokens_f16")
    return out


def tokens_to_ncfhw(x: torch.Tensor, B: int, Cc: int, F: int, H: int, W: int, col0: int = 0, out=None):
    lib = _lib.load()
    _rowmajor(x, "X")
    if out is None:
        out = torch.empty((B, Cc, F, H, W), dtype=torch.float16, device=x.device)
    _lib.check(lib.anyv2v_tokens_to_ncfhw_f16(_p(x), _p(out), B, Cc, F, H * W, x.stride(0), col0, _stream()),
               "anyv2v_tokens_to_ncfhw_f16")
    return out


def adaptive_avgpool(x: torch.Tensor, N: int, Hi: int, Wi: int, Ho: int, Wo: int, out=None):
    lib = _lib.load()
    _rowmajor(x, "X")
    assert x.is_contiguous()
    Cc = x.shape[1]
    if out is None:
        out = torch.empty((N * Ho * Wo, Cc), dtype=torch.float16, device=x.device)
    assert out.is_contiguous() and out.dtype == torch.float16 and tuple(out.shape) == (N * Ho * Wo, Cc)
    _lib.check(lib.anyv2v_adaptive_avgpool_f16(_p(x), _p(out), N, Hi, Wi, Ho, Wo, Cc, _stream()), "anyv2v_adaptive_avgpool_f16")
    return out


def copy_cols(x: torch.Tensor, xcol0: int, y: torch.Tensor, ycol0: int, ncols: int):
    lib = _lib.load()
    _rowmajor(x, "X")
    _rowmajor(y, "Y")
    assert x.shape[0] == y.shape[0]
    _lib.check(lib.anyv2v_copy_cols_f16(_p(x), x.stride(0), xcol0, _p(y), y.stride(0), ycol0, x.shape[0], ncols, _stream()),
               "anyv2v_copy_cols_f16")
    return y


def gather_rows(x: torch.Tensor, xcol0: int, idx: torch.Tensor, y: torch.Tensor, ycol0: int, ncols: int):
    """y[m, ycol0:ycol0+ncols] = x[idx[m], xcol0:xcol0+ncols]; ``idx`` int32 on the device, one entry per row of ``y``."""
    lib = _lib.load()
    _rowmajor(x, "X")
    _rowmajor(y, "Y")
    assert idx.dtype == torch.int32 and idx.is_contiguous() and idx.numel() == y.shape[0] and idx.device == x.device
    _lib.check(lib.anyv2v_gather_rows_f16(_p(x), x.stride(0), xcol0, _p(idx), _p(y), y.stride(0), ycol0, y.shape[0], ncols,
                                          _stream()), "anyv2v_gather_rows_f16")
    return y


def freeu(hidden: torch.Tensor, skip: torch.Tensor, n_img: int, H: int, W: int, b: float, s: float, out=None):
    """FreeU on the pair an up block concatenates (``anyv2v_freeu_f16``, include/anyv2v_hip.h), token matrices [n_img H W, C]:
    the first half of ``hidden``'s channels times ``b``; ``skip`` through the 2 x 2-box Fourier filter with scale ``s``, per
    (image, channel) plane.  Out of place -> (hidden', skip'); ``out`` = (hidden', skip') to write into given matrices."""
    lib = _lib.load()
    _rowmajor(hidden, "hidden")
    _rowmajor(skip, "skip")
    rows = n_img * H * W
    assert hidden.shape[0] == rows and skip.shape[0] == rows, f"freeu: {tuple(hidden.shape)} / {tuple(skip.shape)} rows, expected {rows}"
    if out is None:
        out = (torch.empty((rows, hidden.shape[1]), dtype=torch.float16, device=hidden.device),
               torch.empty((rows, skip.shape[1]), dtype=torch.float16, device=skip.device))
    ho, so = out
    _rowmajor(ho, "hidden'")
    _rowmajor(so, "skip'")
    assert tuple(ho.shape) == tuple(hidden.shape) and tuple(so.shape) == tuple(skip.shape)
    _lib.check(lib.anyv2v_freeu_f16(_p(hidden), hidden.stride(0), _p(ho), ho.stride(0), hidden.shape[1], float(b),
                                    _p(skip), skip.stride(0), _p(so), so.stride(0), skip.shape[1], float(s), n_img, H, W, _stream()),
               "anyv2v_freeu_f16")
    return ho, so


def tile_blend(tiles: torch.Tensor, C: int, plan, bases, n_img: int, out=None):
    """Stitch of the tiled VAE (``anyv2v_tile_blend_f16``, include/anyv2v_hip.h): ``tiles`` is the token matrix [rows, ld] that holds
    the raw tiles -- tile (ty, tx) of image n at row ``bases[ty][tx] + n * th * tw`` -- ``plan`` a ``vae_tiling.StitchPlan``.
    -> fp16 [n_img, C, plan.H, plan.W]."""
    lib = _lib.load()
    _rowmajor(tiles, "tiles")
    ph, wh, pd, wd = plan.tables(bases, tiles.device)
    if out is None:
        out = torch.empty((n_img, C, plan.H, plan.W), dtype=torch.float16, device=tiles.device)
    assert out.is_contiguous() and out.dtype == torch.float16 and tuple(out.shape) == (n_img, C, plan.H, plan.W)
    _lib.check(lib.anyv2v_tile_blend_f16(_p(tiles), tiles.shape[0], tiles.stride(0), C, ph.data_ptr(), wh.data_ptr(), _p(pd), _p(wd),
                                         plan.ay.n_tiles, plan.ax.n_tiles, _p(out), n_img, plan.H, plan.W, _stream()),
               "anyv2v_tile_blend_f16")
    return out


def rotary(x: torch.Tensor, col0: int, rot_dim: int, rows_per_pos: int, n_pos: int, theta: float = 10000.0, windows: int = 1,
           window_stride: int = 0):
    """In-place rotary position embedding of columns [col0 + w * window_stride, ... + rot_dim), w < windows (interleaved pairs);
    the position of row r is (r // rows_per_pos) % n_pos -- see include/anyv2v_hip.h."""
    lib = _lib.load()
    _rowmajor(x, "X")
    _lib.check(lib.anyv2v_rotary_f16(_p(x), x.stride(0), x.shape[0], col0, rot_dim, windows, window_stride, rows_per_pos, n_pos,
                                     float(theta), _stream()), "anyv2v_rotary_f16")
    return x


def cfg_ddim_step(vtok: torch.Tensor, b_unc: int, b_cond: int, guidance: float, coef: torch.Tensor,
                  lat: torch.Tensor, out: torch.Tensor):
    """lat/out: [1, C, F, H, W] fp16; vtok: [(nb F) HW, ld] channels-last v-prediction; coef: 4 device floats."""
    lib = _lib.load()
    _rowmajor(vtok, "V")
    assert lat.is_contiguous() and out.is_contiguous() and lat.dtype == torch.float16 and lat.shape[0] == 1
    assert coef.dtype == torch.float32 and coef.numel() >= 4
    _, Cc, F, H, W = lat.shape
    _lib.check(lib.anyv2v_cfg_ddim_step_f16(_p(vtok), vtok.stride(0), b_unc, b_cond, float(guidance), _p(coef), _p(lat),
                                            _p(out), Cc, F, H * W, _stream()), "anyv2v_cfg_ddim_step_f16")
    return out


GUIDANCE_STATS_FLOATS = _lib.GUIDANCE_STATS_BLOCKS * _lib.GUIDANCE_STATS_RECORD


def _branches_inside(vtok: torch.Tensor, branches, F: int, HW: int):
    assert all(0 <= b and (b + 1) * F * HW <= vtok.shape[0] for b in branches), \
        f"branch {tuple(branches)} of {F} x {HW} pixels lies outside the {vtok.shape[0]} token rows"


def guidance_stats(vtok: torch.Tensor, b_unc: int, b_cond: int, guidance: float, lat_shape, out: Optional[torch.Tensor] = None):
    """Records of the guidance rescale (``anyv2v_guidance_stats_f16``): sums about a pivot of the text branch ``vtok[b_cond]`` and of
    the guided prediction, over one clip ``lat_shape`` = [1, C, F, H, W].  -> fp32 [GUIDANCE_STATS_FLOATS], for ``cfg_ddim_step_ex``."""
    lib = _lib.load()
    _rowmajor(vtok, "V")
    _, Cc, F, H, W = lat_shape
    _branches_inside(vtok, (b_unc, b_cond), F, H * W)
    if out is None:
        out = torch.empty(GUIDANCE_STATS_FLOATS, dtype=torch.float32, device=vtok.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and out.numel() >= GUIDANCE_STATS_FLOATS and out.device == vtok.device
    _lib.check(lib.anyv2v_guidance_stats_f16(_p(vtok), vtok.stride(0), b_unc, b_cond, float(guidance), _p(out), Cc, F, H * W, _stream()),
               "anyv2v_guidance_stats_f16")
    return out


def cfg_ddim_step_ex(vtok: torch.Tensor, b_unc: int, b_cond: int, guidance: float, row: torch.Tensor, lat: torch.Tensor,
                     out: torch.Tensor, *, prediction: int = 0, stats: Optional[torch.Tensor] = None, phi: float = 0.0,
                     noise: Optional[torch.Tensor] = None):
    """``cfg_ddim_step`` with guidance rescale and stochastic DDIM (``anyv2v_cfg_ddim_step_ex_f16``).  row: 8 device floats {sa_t, sb_t,
    c_x0, c_eps, sigma, phi, n, 0} (``DDIMScheduler.coefficient_table(..., eta=, phi=, n=)``); ``stats`` from ``guidance_stats`` when
    ``phi`` > 0 (the host's copy of row[5]); ``noise``: fp16, planar like ``lat``, or None when sigma is 0 for the whole run."""
    lib = _lib.load()
    _rowmajor(vtok, "V")
    assert lat.is_contiguous() and out.is_contiguous() and lat.dtype == out.dtype == torch.float16 and lat.shape[0] == 1 and out.shape == lat.shape
    assert row.dtype == torch.float32 and row.is_contiguous() and row.numel() >= 8 and row.device == vtok.device
    _, Cc, F, H, W = lat.shape
    _branches_inside(vtok, (b_cond,) if b_unc < 0 else (b_unc, b_cond), F, H * W)
    if stats is not None:
        assert stats.dtype == torch.float32 and stats.is_contiguous() and stats.numel() >= GUIDANCE_STATS_FLOATS and stats.device == vtok.device
    if noise is not None:
        assert noise.dtype == torch.float16 and noise.is_contiguous() and noise.numel() == lat.numel() and noise.device == vtok.device
    _lib.check(lib.anyv2v_cfg_ddim_step_ex_f16(_p(vtok), vtok.stride(0), b_unc, b_cond, float(guidance), int(prediction), _p(row), _p(stats),
                                               float(phi), _p(noise), _p(lat), _p(out), Cc, F, H * W, _stream()),
               "anyv2v_cfg_ddim_step_ex_f16")
    return out


def gaussian_taps(sigma: float, max_radius: Optional[int] = None, name: str = "feather", unit: str = "latent pixels"):
    """The feather's taps for ``latent_mask``: ``exp(-k^2 / (2 sigma^2)) / sum`` for k = -R .. R, R = ceil(3 sigma), computed in fp64 and
    rounded to fp32 -> list of 2 R + 1 Python floats that are exactly fp32 values ([] for sigma = 0: no feather).  ``max_radius``: the
    largest R of the kernel that takes them (``pixel_alpha`` passes its own, and how to name the argument it refuses)."""
    import math
    sigma = float(sigma)
    max_radius = _lib.MASK_MAX_RADIUS if max_radius is None else max_radius
    if not 0.0 <= sigma <= max_radius / 3.0:   # (also refuses NaN)
        raise ValueError(f"{name}={sigma}: 0 <= {name} <= {max_radius // 3} {unit}")
    R = int(math.ceil(3.0 * sigma))
    if R == 0:
        return []
    raw = [math.exp(-(k * k) / (2.0 * sigma * sigma)) for k in range(-R, R + 1)]
    total = math.fsum(raw)
    return [C.c_float(v / total).value for v in raw]


def latent_mask(mask: torch.Tensor, grow: int = 0, sigma: float = 0.0, out: Optional[torch.Tensor] = None):
    """Pixel mask [Fm, H, W] fp16 in [0, 1] -> latent mask [Fm, H / 8, W / 8] fp16 (``anyv2v_latent_mask_f16``): 8 x 8 mean, grown by
    ``grow`` latent pixels (window maximum), feathered by a Gaussian of ``sigma`` latent pixels.  Once per clip, outside any graph."""
    lib = _lib.load()
    assert mask.dim() == 3 and mask.dtype == torch.float16 and mask.is_contiguous(), f"latent_mask: contiguous fp16 [Fm, H, W] expected, got {tuple(mask.shape)} {mask.dtype}"
    Fm, H, W = mask.shape
    taps = gaussian_taps(sigma)
    R = len(taps) // 2
    if out is None:
        out = torch.empty((Fm, H // 8, W // 8), dtype=torch.float16, device=mask.device)
    assert out.dtype == torch.float16 and out.is_contiguous() and tuple(out.shape) == (Fm, H // 8, W // 8) and out.device == mask.device
    ws = torch.empty(2 * out.numel(), dtype=torch.float32, device=mask.device)
    arr = (C.c_float * len(taps))(*taps) if taps else None
    _lib.check(lib.anyv2v_latent_mask_f16(_p(mask), Fm, H, W, int(grow), arr, R, _p(ws), _p(out), _stream()), "anyv2v_latent_mask_f16")
    return out


def masked_blend(x: torch.Tensor, src: torch.Tensor, mask: torch.Tensor, out: Optional[torch.Tensor] = None):
    """``out = mask == 0 ? src : mask == 1 ? x : fp16(fmaf(mask, x - src, src))`` (``anyv2v_masked_blend_f16``): x / src / out
    [1, C, F, h, w] fp16, mask [Fm, h, w] fp16 with Fm 1 or F, broadcast over the channels.  ``out`` may be ``x`` (in place)."""
    lib = _lib.load()
    if out is None:
        out = torch.empty_like(x)
    for t in (x, src, out):
        assert t.dtype == torch.float16 and t.is_contiguous() and t.dim() == 5 and t.shape[0] == 1 and t.shape == x.shape and t.device == x.device
    _, Cc, F, H, W = x.shape
    assert mask.dtype == torch.float16 and mask.is_contiguous() and mask.dim() == 3 and tuple(mask.shape[1:]) == (H, W) and mask.device == x.device, \
        f"masked_blend: mask {tuple(mask.shape)} {mask.dtype} against latents {tuple(x.shape)}"
    _lib.check(lib.anyv2v_masked_blend_f16(_p(x), _p(src), _p(mask), mask.shape[0], _p(out), Cc, F, H * W, _stream()), "anyv2v_masked_blend_f16")
    return out


def diff_map_accum(vtok: torch.Tensor, C_: int, F: int, HW: int, acc: torch.Tensor, first):
    """``acc[p] = first ? s[p] : acc[p] + s[p]``, ``s[p] = sum_c |vtok[F HW + p, c] - vtok[p, c]|`` (``anyv2v_diff_map_accum_f16``): vtok is
    the UNet's token-layout output of the batch [source, edit], acc fp32 with F * HW elements.  ``first``: a bool, or a one-element int32
    DEVICE tensor read by the kernel -- the form a captured graph needs to serve the first map and the following ones."""
    lib = _lib.load()
    _rowmajor(vtok, "V")
    assert vtok.shape[0] >= 2 * F * HW and vtok.shape[1] >= C_, f"diff_map_accum: {tuple(vtok.shape)} tokens for 2 x {F} x {HW} pixels of {C_} channels"
    assert acc.dtype == torch.float32 and acc.is_contiguous() and acc.numel() == F * HW and acc.device == vtok.device
    flag = None
    if torch.is_tensor(first):
        assert first.dtype == torch.int32 and first.numel() == 1 and first.device == vtok.device
        flag, first = first, 0
    _lib.check(lib.anyv2v_diff_map_accum_f16(_p(vtok), vtok.stride(0), int(C_), int(F), int(HW), _p(acc), int(bool(first)), _p(flag), _stream()),
               "anyv2v_diff_map_accum_f16")
    return acc


def diff_map_finish(acc: torch.Tensor, F: int, h: int, w: int, ratio: float, threshold: float, out=None):
    """fp32 accumulator [F h w] -> (map fp16 [F, h, w], pixel mask bool [F, 8 h, 8 w]) (``anyv2v_diff_map_finish_f16``):
    ``map = fp16(clamp(ratio acc / mean(acc), 0, 1))`` with one mean over the clip (0 when the mean is 0), ``mask = map > fp16(threshold)``
    with every latent pixel replicated over its 8 x 8 block.  ``out`` = (map, uint8 or bool mask) to write into given tensors."""
    lib = _lib.load()
    assert acc.dtype == torch.float32 and acc.is_contiguous() and acc.numel() == F * h * w and acc.is_cuda
    if out is None:
        out = (torch.empty((F, h, w), dtype=torch.float16, device=acc.device), torch.empty((F, 8 * h, 8 * w), dtype=torch.bool, device=acc.device))
    m, pm = out
    assert m.dtype == torch.float16 and m.is_contiguous() and tuple(m.shape) == (F, h, w) and m.device == acc.device
    assert pm.dtype in (torch.bool, torch.uint8) and pm.is_contiguous() and tuple(pm.shape) == (F, 8 * h, 8 * w) and pm.device == acc.device
    rec = torch.empty(_lib.DIFF_MAP_BLOCKS, dtype=torch.float32, device=acc.device)
    _lib.check(lib.anyv2v_diff_map_finish_f16(_p(acc), int(F), int(h), int(w), float(ratio), float(threshold), _p(rec), _p(m), _p(pm), _stream()),
               "anyv2v_diff_map_finish_f16")
    return m, pm


def pixel_alpha(latent_mask: torch.Tensor, grow_px: int = 0, feather_px: float = 0.0, out: Optional[torch.Tensor] = None):
    """Latent mask [Fm, h, w] fp16 (``latent_mask``'s result) -> pixel-space alpha [Fm, 8 h, 8 w] fp32 (``anyv2v_pixel_alpha_f16``): 1 on the
    cells with mask > 0 grown by ``grow_px`` pixels, a Gaussian of ``feather_px`` pixels (sigma <= 16; R = ceil(3 sigma)) falling to exactly
    0 beyond ``grow_px + 2 R``.  Separable passes; once per clip, outside any graph."""
    lib = _lib.load()
    assert latent_mask.dim() == 3 and latent_mask.dtype == torch.float16 and latent_mask.is_contiguous(), \
        f"pixel_alpha: contiguous fp16 [Fm, h, w] expected, got {tuple(latent_mask.shape)} {latent_mask.dtype}"
    if isinstance(grow_px, bool) or not 0 <= grow_px <= _lib.COMPOSITE_MAX_GROW or int(grow_px) != grow_px:   # (the range check also refuses NaN)
        raise ValueError(f"grow_px={grow_px}: an integer, 0 <= grow_px <= {_lib.COMPOSITE_MAX_GROW} pixels")
    taps = gaussian_taps(feather_px, _lib.COMPOSITE_MAX_RADIUS, "feather_px", "pixels")
    Fm, h, w = latent_mask.shape
    if out is None:
        out = torch.empty((Fm, 8 * h, 8 * w), dtype=torch.float32, device=latent_mask.device)
    assert out.dtype == torch.float32 and out.is_contiguous() and tuple(out.shape) == (Fm, 8 * h, 8 * w) and out.device == latent_mask.device
    ws = torch.empty(2 * out.numel(), dtype=torch.float32, device=latent_mask.device)
    arr = (C.c_float * len(taps))(*taps) if taps else None
    _lib.check(lib.anyv2v_pixel_alpha_f16(_p(latent_mask), Fm, h, w, int(grow_px), arr, len(taps) // 2, _p(ws), _p(out), _stream()),
               "anyv2v_pixel_alpha_f16")
    return out


def _composite_operands(video, source_u8, alpha):
    assert video.dtype == torch.float16 and video.is_contiguous() and video.dim() == 5 and video.shape[0] == 1 and video.shape[1] == 3, \
        f"composite: contiguous fp16 video [1, 3, F, H, W] expected, got {tuple(video.shape)} {video.dtype}"
    _, _, F, H, W = video.shape
    assert source_u8.dtype == torch.uint8 and source_u8.is_contiguous() and tuple(source_u8.shape) == (F, H, W, 3) and source_u8.device == video.device, \
        f"composite: source {tuple(source_u8.shape)} {source_u8.dtype} against video {tuple(video.shape)}: uint8 [F, H, W, 3] expected"
    assert alpha.dtype == torch.float32 and alpha.is_contiguous() and alpha.dim() == 3 and alpha.shape[0] in (1, F) \
        and tuple(alpha.shape[1:]) == (H, W) and alpha.device == video.device, \
        f"composite: alpha {tuple(alpha.shape)} {alpha.dtype} against video {tuple(video.shape)}: fp32 [1 or F, H, W] expected"
    return F, H, W


def composite_stats(video: torch.Tensor, source_u8: torch.Tensor, alpha: torch.Tensor, out: Optional[torch.Tensor] = None):
    """The colour match's statistics (``anyv2v_composite_stats_u8``) -> int64 [COMPOSITE_STATS_BLOCKS, COMPOSITE_STATS_RECORD]: per block
    and channel c, at [5 c .. 5 c + 4], count / sum e / sum e^2 / sum s / sum s^2 over the kept pixels (alpha == 0) of the whole clip, e the
    byte ``vae.to_pil`` forms from the video, s the source byte.  Exact integer sums."""
    lib = _lib.load()
    F, H, W = _composite_operands(video, source_u8, alpha)
    shape = (_lib.COMPOSITE_STATS_BLOCKS, _lib.COMPOSITE_STATS_RECORD)
    if out is None:
        out = torch.empty(shape, dtype=torch.int64, device=video.device)
    assert out.dtype == torch.int64 and out.is_contiguous() and tuple(out.shape) == shape and out.device == video.device
    _lib.check(lib.anyv2v_composite_stats_u8(_p(video), _p(source_u8), _p(alpha), alpha.shape[0], F, H, W, _p(out), _stream()),
               "anyv2v_composite_stats_u8")
    return out


def composite(video: torch.Tensor, source_u8: torch.Tensor, alpha: torch.Tensor, match_color: bool = False, out: Optional[torch.Tensor] = None):
    """``out = alpha == 0 ? source : alpha == 1 ? e : rint(fmaf(alpha, e - source, source))`` in bytes (``anyv2v_composite_u8``): video
    [1, 3, F, H, W] fp16 in [-1, 1] (``decode_latents``), source uint8 [F, H, W, 3], alpha fp32 [Fm, H, W] with Fm 1 or F -> uint8
    [F, H, W, 3]; e is the byte ``vae.to_pil`` forms.  ``match_color``: e is first mapped by the gain and bias that carry the edit's
    per-channel mean and deviation over the kept region to the source's (``composite_stats``, one more launch)."""
    lib = _lib.load()
    F, H, W = _composite_operands(video, source_u8, alpha)
    rec = composite_stats(video, source_u8, alpha) if match_color else None
    if out is None:
        out = torch.empty_like(source_u8)
    assert out.dtype == torch.uint8 and out.is_contiguous() and out.shape == source_u8.shape and out.device == video.device
    _lib.check(lib.anyv2v_composite_u8(_p(video), _p(source_u8), _p(alpha), alpha.shape[0], _p(rec), _p(out), F, H, W, _stream()),
               "anyv2v_composite_u8")
    return out


def _track_frames(what, t, last=None):
    shape = ("F", "H", "W") + (() if last is None else (str(last),))
    assert t.dtype == torch.uint8 and t.is_contiguous() and t.dim() == len(shape) and (last is None or t.shape[-1] == last) \
        and t.shape[0] >= 1 and t.shape[1] >= 8 and t.shape[2] >= 8 and t.shape[1] % 8 == 0 and t.shape[2] % 8 == 0, \
        f"{what}: contiguous uint8 [{', '.join(shape)}] with H, W positive multiples of 8 expected, got {tuple(t.shape)} {t.dtype}"
    return int(t.shape[0]), int(t.shape[1]), int(t.shape[2])


def luma_u8(frames: torch.Tensor):
    """uint8 [F, H, W, 3] -> uint8 [F, H, W], ``Y = (77 R + 150 G + 29 B + 128) >> 8`` (``anyv2v_luma_u8``)."""
    lib = _lib.load()
    F, H, W = _track_frames("luma_u8", frames, 3)
    out = torch.empty((F, H, W), dtype=torch.uint8, device=frames.device)
    _lib.check(lib.anyv2v_luma_u8(_p(frames), _p(out), F, H, W, _stream()), "anyv2v_luma_u8")
    return out


def block_match(luma: torch.Tensor, radius: int = 16):
    """Luma uint8 [F, H, W] -> int16 [F, H / 8, W / 8, 2], per frame k >= 1 and 8 x 8 cell the displacement (dy, dx) in [-radius, radius]^2
    that minimises (SAD of the cell's 16 x 16 window of frame k against frame k - 1, dy^2 + dx^2, dy, dx); frame 0: zeros
    (``anyv2v_block_match_u8``; the definition is in ``include/anyv2v_hip.h``).  ``radius``: an integer 0 .. 32."""
    lib = _lib.load()
    F, H, W = _track_frames("block_match", luma)
    if isinstance(radius, bool) or not 0 <= radius <= _lib.TRACK_MAX_RADIUS or int(radius) != radius:   # (the range check also refuses NaN)
        raise ValueError(f"radius={radius}: an integer, 0 <= radius <= {_lib.TRACK_MAX_RADIUS} pixels")
    out = torch.empty((F, H // 8, W // 8, 2), dtype=torch.int16, device=luma.device)
    _lib.check(lib.anyv2v_block_match_u8(_p(luma), _p(out), F, H, W, int(radius), _stream()), "anyv2v_block_match_u8")
    return out


def _track_flow(what, flow):
    assert flow.dtype == torch.int16 and flow.is_contiguous() and flow.dim() == 4 and flow.shape[3] == 2 and min(flow.shape[:3]) >= 1, \
        f"{what}: contiguous int16 [F, h, w, 2] expected, got {tuple(flow.shape)} {flow.dtype}"
    return (int(v) for v in flow.shape[:3])


def flow_median(flow: torch.Tensor):
    """int16 [F, h, w, 2] -> the same with every component replaced by the median of its 3 x 3 cell neighbourhood, replicate border
    (``anyv2v_flow_median_i16``)."""
    lib = _lib.load()
    F, h, w = _track_flow("flow_median", flow)
    out = torch.empty_like(flow)
    _lib.check(lib.anyv2v_flow_median_i16(_p(flow), _p(out), F, h, w, _stream()), "anyv2v_flow_median_i16")
    return out


def mask_propagate(mask0: torch.Tensor, flow: torch.Tensor):
    """Frame-0 mask [H, W] (bool, or uint8 with non-zero = set) carried along ``flow`` int16 [F, H / 8, W / 8, 2] -> bool [F, H, W] with
    ``mask_k[p] = mask_{k-1}[clamp(p + D_k[cell(p)])]`` (``anyv2v_mask_propagate_u8``: one launch, the chain walked per pixel)."""
    lib = _lib.load()
    F, h, w = _track_flow("mask_propagate", flow)
    assert mask0.dtype in (torch.bool, torch.uint8) and mask0.is_contiguous() and tuple(mask0.shape) == (8 * h, 8 * w) \
        and mask0.device == flow.device, \
        f"mask_propagate: contiguous bool / uint8 mask [{8 * h}, {8 * w}] expected for a flow of {tuple(flow.shape)}, got {tuple(mask0.shape)} {mask0.dtype}"
    out = torch.empty((F, 8 * h, 8 * w), dtype=torch.uint8, device=flow.device)
    _lib.check(lib.anyv2v_mask_propagate_u8(_p(mask0), _p(flow), _p(out), F, 8 * h, 8 * w, _stream()), "anyv2v_mask_propagate_u8")
    return out.view(torch.bool)


def first_frame_mask(source: torch.Tensor, edited: torch.Tensor, threshold: int = 24, min_count: int = 8):
    """Source and edited first frame, uint8 [H, W, 3] -> bool [1, H, W], constant on 8 x 8 cells: a cell is set when at least
    ``min_count`` (1 .. 64) of its pixels have ``max_c |edited - source| > threshold`` (strict, 0 .. 255) (``anyv2v_first_frame_mask_u8``)."""
    lib = _lib.load()
    _, H, W = _track_frames("first_frame_mask", source[None] if source.dim() == 3 else source, 3)
    assert source.dim() == 3 and edited.dtype == torch.uint8 and edited.is_contiguous() and edited.shape == source.shape \
        and edited.device == source.device, \
        f"first_frame_mask: edited {tuple(edited.shape)} {edited.dtype} against source {tuple(source.shape)}: the same uint8 [H, W, 3] expected"
    if isinstance(threshold, bool) or not 0 <= threshold <= 255 or int(threshold) != threshold:
        raise ValueError(f"threshold={threshold}: an integer, 0 <= threshold <= 255")
    if isinstance(min_count, bool) or not 1 <= min_count <= 64 or int(min_count) != min_count:
        raise ValueError(f"min_count={min_count}: an integer, 1 <= min_count <= 64")
    out = torch.empty((1, H, W), dtype=torch.uint8, device=source.device)
    _lib.check(lib.anyv2v_first_frame_mask_u8(_p(source), _p(edited), _p(out), H, W, int(threshold), int(min_count), _stream()),
               "anyv2v_first_frame_mask_u8")
    return out.view(torch.bool)


_RESAMPLE_TABLES = {}   # (in_size, in0, in1, out_size, filter) -> (ksize, bounds, coeffs) on the host
_RESAMPLE_DEVICE = {}   # (pass geometry, device) -> the pass with its tables on the device


def resample_table(in_size: int, in0: float, in1: float, out_size: int, resample: str = "lanczos"):
    """The table of one side as ``anyv2v_resample_table`` builds it (host code, no GPU) -> ``(ksize, bounds int32 [out_size, 2],
    coeffs int32 [out_size, ksize])`` on the CPU, cached per geometry.  ``ValueError`` for what the planner refuses."""
    if resample not in _lib.RESAMPLE_FILTERS:
        raise ValueError(f"resample={resample!r}: one of {sorted(_lib.RESAMPLE_FILTERS)} ('nearest' is not a resampling filter of this kind)")
    key = (int(in_size), float(in0), float(in1), int(out_size), resample)
    if key not in _RESAMPLE_TABLES:
        lib = _lib.load()
        args = key[:4] + (_lib.RESAMPLE_FILTERS[resample],)
        ksize = lib.anyv2v_resample_table(*args, None, None)
        if ksize > 0:
            bounds = torch.empty((key[3], 2), dtype=torch.int32)
            coeffs = torch.empty((key[3], ksize), dtype=torch.int32)
            ptr = C.POINTER(C.c_int)
            ksize = lib.anyv2v_resample_table(*args, C.cast(bounds.data_ptr(), ptr), C.cast(coeffs.data_ptr(), ptr))
        if ksize <= 0:
            msg = lib.anyv2v_last_error()
            raise ValueError(f"resample_u8: {msg.decode() if msg else 'the table was refused'}")
        if len(_RESAMPLE_TABLES) >= 64:
            _RESAMPLE_TABLES.clear()
        _RESAMPLE_TABLES[key] = (ksize, bounds, coeffs)
    return _RESAMPLE_TABLES[key]


def resample_passes(H: int, W: int, size, resample: str = "lanczos", box=None, window=None):
    """What ``resample_u8`` launches for frames of H x W: ``(window, row0, rows, h, v)``.  ``h`` / ``v``: ``None`` where Pillow skips the
    pass (that side's size unchanged and its box the whole side), else ``(ksize, bounds, coeffs)`` cut to the window's outputs, on the
    CPU.  The horizontal pass (or the copy in its place) covers the input rows [row0, row0 + rows) that the vertical pass reads -- its
    bounds count from row0 --, as in Pillow."""
    try:
        out_w, out_h = (int(v) for v in size)
        ok = (out_w, out_h) == tuple(size)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"size={size!r}: (out_w, out_h), two integers")
    try:
        x0, y0, x1, y1 = (float(v) for v in ((0, 0, W, H) if box is None else box))
    except (TypeError, ValueError):
        raise ValueError(f"box={box!r}: (x0, y0, x1, y1) in source pixels") from None
    try:
        wx, wy, ww, wh = (int(v) for v in ((0, 0, out_w, out_h) if window is None else window))
        ok = window is None or (wx, wy, ww, wh) == tuple(window)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"window={window!r}: (wx, wy, ww, wh), four integers")
    need_h = out_w != W or x0 != 0.0 or x1 != float(W)
    need_v = out_h != H or y0 != 0.0 or y1 != float(H)
    # the tables first: a bad size or box is the planner's to refuse
    th = resample_table(W, x0, x1, out_w, resample) if need_h else None
    tv = resample_table(H, y0, y1, out_h, resample) if need_v else None
    if not (0 <= wx and 0 <= wy and ww >= 1 and wh >= 1 and wx + ww <= out_w and wy + wh <= out_h):
        raise ValueError(f"window={window!r} does not lie inside size={tuple(size)!r}")
    h = v = None
    row0, rows = wy, wh
    if need_v:
        bounds = tv[1][wy:wy + wh].clone()
        row0 = int(bounds[0, 0])
        rows = int(bounds[-1, 0] + bounds[-1, 1]) - row0
        bounds[:, 0] -= row0
        v = (tv[0], bounds, tv[2][wy:wy + wh].contiguous())
    if need_h:
        h = (th[0], th[1][wx:wx + ww].contiguous(), th[2][wx:wx + ww].contiguous())
    return (wx, wy, ww, wh), row0, rows, h, v


def resample_u8(frames: torch.Tensor, size, resample: str = "lanczos", box=None, window=None):
    """Pillow's ``Image.resize(size, resample, box)`` of every frame, byte for byte, and optionally only the rectangle ``window`` of it
    (equal to ``.crop`` of the whole): contiguous uint8 [F, H, W, C] on the GPU, C = 1 or 3 -> uint8 [F, wh, ww, C].  ``size = (out_w,
    out_h)``; ``resample``: lanczos, bicubic, bilinear or box; ``box = (x0, y0, x1, y1)`` floats in source pixels (default: the frame);
    ``window = (wx, wy, ww, wh)`` integers in output pixels (default: all of it).  Two launches (``anyv2v_resample_h_u8``,
    ``anyv2v_resample_v_u8``; the definition is in ``include/anyv2v_hip.h``), one where Pillow skips a pass, a copy where it skips both."""
    if not (isinstance(frames, torch.Tensor) and frames.dtype == torch.uint8 and frames.dim() == 4 and frames.is_contiguous() and frames.is_cuda
            and frames.shape[0] >= 1 and frames.shape[3] in (1, 3)):
        got = f"{tuple(frames.shape)} {frames.dtype} on {frames.device}" if isinstance(frames, torch.Tensor) else type(frames).__name__
        raise ValueError(f"resample_u8: a contiguous uint8 [F, H, W, C] tensor on the GPU with C = 1 or 3 expected, got {got}")
    F, H, W, Cc = (int(v) for v in frames.shape)
    key = (H, W, tuple(size) if isinstance(size, (tuple, list)) else size, resample, None if box is None else tuple(box),
           None if window is None else tuple(window), str(frames.device))
    if key not in _RESAMPLE_DEVICE:
        win, row0, rows, h, v = resample_passes(H, W, size, resample, box, window)
        if len(_RESAMPLE_DEVICE) >= 64:
            _RESAMPLE_DEVICE.clear()
        _RESAMPLE_DEVICE[key] = (win, row0, rows) + tuple(None if p is None else (p[0], p[1].to(frames.device), p[2].to(frames.device))
                                                          for p in (h, v))
    (wx, wy, ww, wh), row0, rows, h, v = _RESAMPLE_DEVICE[key]
    lib = _lib.load()
    if h is None:
        x = frames[:, row0:row0 + rows, wx:wx + ww].contiguous()
        if v is None and x.data_ptr() == frames.data_ptr():
            x = x.clone()
    else:
        x = torch.empty((F, rows, ww, Cc), dtype=torch.uint8, device=frames.device)
        _lib.check(lib.anyv2v_resample_h_u8(_p(frames), _p(x), F, H, W, Cc, row0, rows, ww, _p(h[1]), _p(h[2]), h[0], _stream()),
                   "anyv2v_resample_h_u8")
    if v is None:
        return x
    out = torch.empty((F, wh, ww, Cc), dtype=torch.uint8, device=frames.device)
    _lib.check(lib.anyv2v_resample_v_u8(_p(x), _p(out), F, rows, ww, Cc, wh, _p(v[1]), _p(v[2]), v[0], _stream()), "anyv2v_resample_v_u8")
    return out


_RESTORE_DEVICE = {}    # (geometry, device) -> the passes of ``restore_passes`` with their tables on the device


def _dest(dest, sh, sw, what):
    try:
        dx0, dy0, dx1, dy1 = (int(v) for v in dest)
        ok = (dx0, dy0, dx1, dy1) == tuple(dest)
    except (TypeError, ValueError):
        ok = False
    if not ok or not (0 <= dx0 < dx1 <= sw and 0 <= dy0 < dy1 <= sh):
        raise ValueError(f"{what}: dest={dest!r}: (dx0, dy0, dx1, dy1), a non-empty integer rectangle inside the {sw} x {sh} frame")
    return dx0, dy0, dx1, dy1


def restore_passes(h: int, w: int, dest, box, resample: str = "lanczos"):
    """What ``restore_u8`` launches for an edit of h x w resized from ``box`` to the size of ``dest``: ``(edit, alpha)``, each
    ``(row0, rows, hpass, vtable)`` on the CPU -- the input rows [row0, row0 + rows) the horizontal pass covers, its table (``None`` where
    Pillow skips it) and the vertical table re-based to row0, an identity table (``ksize`` 1, coefficient ``1 << 22``) where Pillow skips
    the vertical pass.  The edit's tables are of ``resample``, alpha's of bilinear.  ``box`` is taken the way Pillow takes it: its four
    numbers as C floats and the width ``x1 - x0`` formed in float (``ImagingResample`` reads ``float box[4]``), so that the tables are the
    ones Pillow builds for the same argument."""
    f32 = lambda v: C.c_float(v).value
    try:
        x0, y0, x1, y1 = (f32(float(v)) for v in box)
    except (TypeError, ValueError):
        raise ValueError(f"box={box!r}: (x0, y0, x1, y1) in the edit's pixels") from None
    x1, y1 = x0 + f32(x1 - x0), y0 + f32(y1 - y0)
    dw, dh = int(dest[2]) - int(dest[0]), int(dest[3]) - int(dest[1])
    passes = []
    for name in (resample, "bilinear"):
        _, row0, rows, hp, vp = resample_passes(h, w, (dw, dh), name, (x0, y0, x1, y1))
        if vp is None:   # (dh == h and the box is the whole side)
            vp = (1, torch.stack([torch.arange(dh, dtype=torch.int32), torch.ones(dh, dtype=torch.int32)], dim=1).contiguous(),
                  torch.full((dh, 1), 1 << 22, dtype=torch.int32))
        passes.append((row0, rows, hp, vp))
    return tuple(passes)


def restore_paste_u8(source: torch.Tensor, edit_h: torch.Tensor, alpha_h: Optional[torch.Tensor], dest, e_table, a_table=None,
                     out: Optional[torch.Tensor] = None):
    """``anyv2v_restore_paste_u8`` (the definition is in ``include/anyv2v_hip.h``): ``source`` uint8 [F, sh, sw, 3], ``edit_h`` uint8
    [F, e_rows, dw, 3] and ``alpha_h`` uint8 [1 or F, a_rows, dw] or None, the horizontal intermediates; ``e_table`` / ``a_table``
    ``(ksize, bounds, coeffs)`` on the device -> uint8 [F, sh, sw, 3]."""
    ok = lambda t, nd: isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.dim() == nd and t.is_contiguous() and t.is_cuda
    if not (ok(source, 4) and source.shape[3] == 3 and source.shape[0] >= 1):
        raise ValueError("restore_paste_u8: source: a contiguous uint8 [F, sh, sw, 3] tensor on the GPU expected")
    F, sh, sw, _ = (int(v) for v in source.shape)
    dx0, dy0, dx1, dy1 = _dest(dest, sh, sw, "restore_paste_u8")
    dw, dh = dx1 - dx0, dy1 - dy0
    if not (ok(edit_h, 4) and edit_h.shape[0] == F and edit_h.shape[1] >= 1 and tuple(edit_h.shape[2:]) == (dw, 3) and edit_h.device == source.device):
        raise ValueError(f"restore_paste_u8: edit_h: a contiguous uint8 [{F}, rows, {dw}, 3] tensor on {source.device} expected")
    if alpha_h is not None and not (ok(alpha_h, 3) and alpha_h.shape[0] in (1, F) and alpha_h.shape[1] >= 1 and alpha_h.shape[2] == dw
                                    and alpha_h.device == source.device and a_table is not None):
        raise ValueError(f"restore_paste_u8: alpha_h: a contiguous uint8 [1 or {F}, rows, {dw}] tensor on {source.device} with its table expected")
    for t in (e_table,) + (() if alpha_h is None else (a_table,)):
        ksize, bounds, coeffs = t
        if not (bounds.dtype == torch.int32 and coeffs.dtype == torch.int32 and tuple(bounds.shape) == (dh, 2) and tuple(coeffs.shape) == (dh, ksize)
                and bounds.is_contiguous() and coeffs.is_contiguous() and bounds.device == source.device and coeffs.device == source.device):
            raise ValueError(f"restore_paste_u8: a table (ksize, int32 [{dh}, 2], int32 [{dh}, ksize]) on {source.device} expected")
    if out is None:
        out = torch.empty_like(source)
    elif not (ok(out, 4) and out.shape == source.shape and out.device == source.device):
        raise ValueError("restore_paste_u8: out: a contiguous uint8 tensor of the source's shape and device expected")
    a = (1, 1, None, None, 1) if alpha_h is None else (int(alpha_h.shape[0]), int(alpha_h.shape[1]), _p(a_table[1]), _p(a_table[2]), a_table[0])
    _lib.check(_lib.load().anyv2v_restore_paste_u8(_p(source), _p(edit_h), _p(alpha_h), _p(out), F, sh, sw, dx0, dy0, dx1, dy1,
                                                   int(edit_h.shape[1]), _p(e_table[1]), _p(e_table[2]), e_table[0], *a, _stream()),
               "anyv2v_restore_paste_u8")
    return out


def restore_u8(edited_u8: torch.Tensor, source_u8: torch.Tensor, dest, box, resample: str = "lanczos", alpha_u8: Optional[torch.Tensor] = None):
    """An edit at the working size back at the source clip's own size, per frame Pillow's
    ``out = S.copy(); out.paste(E.resize(dsize, resample, box), (dx0, dy0), mask=A.resize(dsize, BILINEAR, box))`` byte for byte (a plain
    paste without alpha): ``edited_u8`` contiguous uint8 [F, h, w, 3] and ``source_u8`` [F, sh, sw, 3] on the GPU, ``dest = (dx0, dy0,
    dx1, dy1)`` integers in source pixels, ``box`` floats in the edit's pixels (``prepare.restore_geometry`` makes both), ``alpha_u8``
    uint8 [1 or F, h, w] (255 = the edit) -> uint8 [F, sh, sw, 3].  Outside ``dest`` the result holds the source's bytes.  Up to three
    launches: ``anyv2v_resample_h_u8`` on the edit and on alpha, then ``anyv2v_restore_paste_u8``."""
    ok = lambda t, nd: isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.dim() == nd and t.is_contiguous() and t.is_cuda and t.shape[0] >= 1
    got = lambda t: f"{tuple(t.shape)} {t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
    if not (ok(edited_u8, 4) and edited_u8.shape[3] == 3):
        raise ValueError(f"restore_u8: edited_u8: a contiguous uint8 [F, h, w, 3] tensor on the GPU expected, got {got(edited_u8)}")
    F, h, w, _ = (int(v) for v in edited_u8.shape)
    if not (ok(source_u8, 4) and source_u8.shape[3] == 3 and source_u8.shape[0] == F and source_u8.device == edited_u8.device):
        raise ValueError(f"restore_u8: source_u8: a contiguous uint8 [{F}, sh, sw, 3] tensor on {edited_u8.device} expected, got {got(source_u8)}")
    if alpha_u8 is not None and not (ok(alpha_u8, 3) and alpha_u8.shape[0] in (1, F) and tuple(alpha_u8.shape[1:]) == (h, w)
                                     and alpha_u8.device == edited_u8.device):
        raise ValueError(f"restore_u8: alpha_u8: a contiguous uint8 [1 or {F}, {h}, {w}] tensor on {edited_u8.device} expected, got {got(alpha_u8)}")
    sh, sw = int(source_u8.shape[1]), int(source_u8.shape[2])
    dest = _dest(dest, sh, sw, "restore_u8")
    dw = dest[2] - dest[0]
    pe, pa = _restore_device_passes(h, w, dest, box, resample, edited_u8.device)
    edit_h = _restore_horizontal(edited_u8, pe, dw)
    alpha_h = None if alpha_u8 is None else _restore_horizontal(alpha_u8[..., None], pa, dw)[..., 0]
    return restore_paste_u8(source_u8, edit_h, alpha_h, dest, pe[3], None if alpha_u8 is None else pa[3])


def _restore_device_passes(h, w, dest, box, resample, dev):
    """``restore_passes`` with the tables on ``dev``, cached per geometry and device."""
    key = (h, w, dest, tuple(box) if isinstance(box, (tuple, list)) else box, resample, str(dev))
    if key not in _RESTORE_DEVICE:
        passes = restore_passes(h, w, dest, box, resample)
        if len(_RESTORE_DEVICE) >= 64:
            _RESTORE_DEVICE.clear()
        on = lambda t: None if t is None else (t[0], t[1].to(dev), t[2].to(dev))
        _RESTORE_DEVICE[key] = tuple((row0, rows, on(hp), on(vp)) for row0, rows, hp, vp in passes)
    return _RESTORE_DEVICE[key]


def _restore_horizontal(x, p, dw):
    """The horizontal pass of one operand of the way back: x uint8 [N, h, w, C] -> [N, rows, dw, C] (a copy of the rows where Pillow skips it)."""
    row0, rows, hp, _ = p
    if hp is None:
        return x[:, row0:row0 + rows].contiguous()
    N, h, w, Cc = (int(v) for v in x.shape)
    y = torch.empty((N, rows, dw, Cc), dtype=torch.uint8, device=x.device)
    _lib.check(_lib.load().anyv2v_resample_h_u8(_p(x), _p(y), N, h, w, Cc, row0, rows, dw, _p(hp[1]), _p(hp[2]), hp[0], _stream()),
               "anyv2v_resample_h_u8")
    return y


def detail_gate_u8(edit_u8: torch.Tensor, prepared_u8: torch.Tensor, lo: int = 8, hi: int = 32, radius: int = 2):
    """Where the edit stayed close to the prepared source (``anyv2v_detail_gate_u8``; the definition is in ``include/anyv2v_hip.h``): both
    contiguous uint8 [F, h, w, 3] on the GPU -> uint8 [F, h, w], 255 where the mean over a ``(2 radius + 1)^2`` box of ``max_c |E - P|`` is
    at most ``lo``, 0 where it is at least ``hi``, a linear ramp between.  Integers, ``0 <= lo < hi <= 255``, ``0 <= radius <= 16``.  Two
    launches (row sums into a uint16 scratch, column sums and the ramp)."""
    ok = lambda t: isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.dim() == 4 and t.is_contiguous() and t.is_cuda \
        and t.shape[0] >= 1 and t.shape[3] == 3
    got = lambda t: f"{tuple(t.shape)} {t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
    if not ok(edit_u8):
        raise ValueError(f"detail_gate_u8: edit_u8: a contiguous uint8 [F, h, w, 3] tensor on the GPU expected, got {got(edit_u8)}")
    if not (ok(prepared_u8) and prepared_u8.shape == edit_u8.shape and prepared_u8.device == edit_u8.device):
        raise ValueError(f"detail_gate_u8: prepared_u8: a contiguous uint8 {list(edit_u8.shape)} tensor on {edit_u8.device} expected, "
                         f"got {got(prepared_u8)}")
    lo, hi, radius = detail_parameters(lo, hi, radius, "detail_gate_u8: ")
    F, h, w, _ = (int(v) for v in edit_u8.shape)
    out = torch.empty((F, h, w), dtype=torch.uint8, device=edit_u8.device)
    scratch = torch.empty((F, h, w), dtype=torch.int16, device=edit_u8.device)
    _lib.check(_lib.load().anyv2v_detail_gate_u8(_p(edit_u8), _p(prepared_u8), _p(out), F, h, w, lo, hi, radius, _p(scratch), 2 * scratch.numel(),
                                                 _stream()), "anyv2v_detail_gate_u8")
    return out


def detail_parameters(lo, hi, radius, what=""):
    """The gate's parameters as integers, or a ``ValueError``: ``0 <= lo < hi <= 255``, ``0 <= radius <= 16``."""
    whole = lambda v: not isinstance(v, bool) and isinstance(v, (int, float)) and int(v) == v
    if not (whole(lo) and whole(hi) and 0 <= lo < hi <= 255):
        raise ValueError(f"{what}lo={lo!r}, hi={hi!r}: integers, 0 <= lo < hi <= 255")
    if not (whole(radius) and 0 <= radius <= _lib.DETAIL_MAX_RADIUS):
        raise ValueError(f"{what}radius={radius!r}: an integer, 0 <= radius <= {_lib.DETAIL_MAX_RADIUS}")
    return int(lo), int(hi), int(radius)


def restore_detail_u8(edited_u8: torch.Tensor, prepared_u8: torch.Tensor, gate_u8: torch.Tensor, source_u8: torch.Tensor, dest, box,
                      resample: str = "lanczos", alpha_u8: Optional[torch.Tensor] = None):
    """``restore_u8`` with the source's fine detail carried into the upscaled edit (``anyv2v_restore_detail_u8``; the definition is in
    ``include/anyv2v_hip.h``): ``prepared_u8`` uint8 [F, h, w, 3] is the frame the model saw (``prepare_frames`` of the source), ``gate_u8``
    uint8 [1 or F, h, w] says where the detail ``S - up(P)`` is added (255) and where not (0) -- ``detail_gate_u8`` makes one, any other is
    taken as it is.  A gate of 0 gives ``restore_u8``; ``edited_u8 == prepared_u8`` under a gate of 255 gives the source.  Up to five
    launches: ``anyv2v_resample_h_u8`` on the edit, the prepared source, the gate and alpha, then ``anyv2v_restore_detail_u8``."""
    ok = lambda t, nd: isinstance(t, torch.Tensor) and t.dtype == torch.uint8 and t.dim() == nd and t.is_contiguous() and t.is_cuda and t.shape[0] >= 1
    got = lambda t: f"{tuple(t.shape)} {t.dtype} on {t.device}" if isinstance(t, torch.Tensor) else type(t).__name__
    if not (ok(edited_u8, 4) and edited_u8.shape[3] == 3):
        raise ValueError(f"restore_detail_u8: edited_u8: a contiguous uint8 [F, h, w, 3] tensor on the GPU expected, got {got(edited_u8)}")
    F, h, w, _ = (int(v) for v in edited_u8.shape)
    dev = edited_u8.device
    if not (ok(prepared_u8, 4) and prepared_u8.shape == edited_u8.shape and prepared_u8.device == dev):
        raise ValueError(f"restore_detail_u8: prepared_u8: a contiguous uint8 [{F}, {h}, {w}, 3] tensor on {dev} expected, got {got(prepared_u8)}")
    if not (ok(source_u8, 4) and source_u8.shape[3] == 3 and source_u8.shape[0] == F and source_u8.device == dev):
        raise ValueError(f"restore_detail_u8: source_u8: a contiguous uint8 [{F}, sh, sw, 3] tensor on {dev} expected, got {got(source_u8)}")
    for name, t in (("gate_u8", gate_u8),) + (() if alpha_u8 is None else (("alpha_u8", alpha_u8),)):
        if not (ok(t, 3) and t.shape[0] in (1, F) and tuple(t.shape[1:]) == (h, w) and t.device == dev):
            raise ValueError(f"restore_detail_u8: {name}: a contiguous uint8 [1 or {F}, {h}, {w}] tensor on {dev} expected, got {got(t)}")
    sh, sw = int(source_u8.shape[1]), int(source_u8.shape[2])
    dx0, dy0, dx1, dy1 = dest = _dest(dest, sh, sw, "restore_detail_u8")
    dw = dx1 - dx0
    pe, pa = _restore_device_passes(h, w, dest, box, resample, dev)
    edit_h, prep_h = _restore_horizontal(edited_u8, pe, dw), _restore_horizontal(prepared_u8, pe, dw)
    gate_h = _restore_horizontal(gate_u8[..., None], pa, dw)
    alpha_h = None if alpha_u8 is None else _restore_horizontal(alpha_u8[..., None], pa, dw)
    out = torch.empty_like(source_u8)
    _lib.check(_lib.load().anyv2v_restore_detail_u8(_p(source_u8), _p(edit_h), _p(prep_h), _p(gate_h), _p(alpha_h), _p(out), F, sh, sw, dx0, dy0,
                                                    dx1, dy1, int(edit_h.shape[1]), _p(pe[3][1]), _p(pe[3][2]), pe[3][0], int(gate_u8.shape[0]),
                                                    1 if alpha_u8 is None else int(alpha_u8.shape[0]), int(gate_h.shape[1]), _p(pa[3][1]),
                                                    _p(pa[3][2]), pa[3][0], _stream()), "anyv2v_restore_detail_u8")
    return out


def ddim_step(v: torch.Tensor, x: torch.Tensor, sa_t: float, sb_t: float, sa_p: float, sb_p: float, out=None):
    lib = _lib.load()
    v = v.to(torch.float16).contiguous()
    x = x.to(torch.float16).contiguous()
    if out is None:
        out = torch.empty_like(x)
    _lib.check(lib.anyv2v_ddim_step_f16(_p(v), _p(x), _p(out), sa_t, sb_t, sa_p, sb_p, x.numel(), _stream()),
               "anyv2v_ddim_step_f16")
    return out


PRED_V, PRED_EPSILON, PRED_SAMPLE = 0, 1, 2


def guided_step(e: torch.Tensor, x: torch.Tensor, coef, *, b_txt: int, b_unc: int = -1, b_img: int = -1, g_txt: float = 1.0,
                g_img: float = 1.0, prediction: int = PRED_V, out=None, noise=None, sigma: float = 0.0):
    """e: [nb, ...] the UNet's prediction of every branch; x: one branch's latents; coef = (sa_t, sb_t, c_x0, c_eps):
    y = c_x0 x0 + c_eps eps (+ sigma noise) -- DDIM: (c_x0, c_eps) = (sa_p, sb_p)."""
    lib = _lib.load()
    assert e.is_contiguous() and x.is_contiguous() and e.dtype == x.dtype == torch.float16
    n = x.numel()
    assert e.numel() % n == 0 and max(b_txt, b_unc, b_img) < e.numel() // n
    if out is None:
        out = torch.empty_like(x)
    sa_t, sb_t, sa_p, sb_p = (float(c) for c in coef)
    if noise is not None or sigma != 0.0:
        assert noise is None or (noise.is_contiguous() and noise.dtype == torch.float16 and noise.numel() == n)
        _lib.check(lib.anyv2v_guided_step_noise_f16(_p(e), n, b_unc, b_img, b_txt, float(g_img), float(g_txt), int(prediction), sa_t, sb_t,
                                                    sa_p, sb_p, _p(x), _p(out), _p(noise), float(sigma), _stream()),
                   "anyv2v_guided_step_noise_f16")
        return out
    _lib.check(lib.anyv2v_guided_step_f16(_p(e), n, b_unc, b_img, b_txt, float(g_img), float(g_txt), int(prediction), sa_t, sb_t, sa_p,
                                          sb_p, _p(x), _p(out), _stream()), "anyv2v_guided_step_f16")
    return out


_HINT = [1, 1]   # mirrored for the host-side decisions (ln_gemm_supported)


def set_batch_hint(num: int, den: int):
    """Switch the hint inside a forward (the shared stem of a CFG batch has one branch less than the layers behind it, so its
    ratio differs: ``I2VGenXLUNet._forward_core``)."""
    _lib.check(_lib.load().anyv2v_set_batch_hint(int(num), int(den)), "anyv2v_set_batch_hint")
    _HINT[:] = [int(num), int(den)]


class batch_hint:
    """``with ops.batch_hint(3, 2): ...`` -- the launches inside choose kernels / split-K factors / GroupNorm chunking as if they had
    3/2 of their rows (``anyv2v_set_batch_hint``): a [negative, editing] step then computes, bit for bit, what the three-branch step
    computes for those branches.  Also valid around a HIP-graph capture (the choices are baked at capture time)."""

    def __init__(self, num: int, den: int):
        self.num, self.den = int(num), int(den)

    def __enter__(self):
        _lib.check(_lib.load().anyv2v_set_batch_hint(self.num, self.den), "anyv2v_set_batch_hint")
        _HINT[:] = [self.num, self.den]
        return self

    def __exit__(self, *exc):
        _lib.check(_lib.load().anyv2v_set_batch_hint(1, 1), "anyv2v_set_batch_hint")
        _HINT[:] = [1, 1]
        return False


def selftest(scratch: torch.Tensor):
    lib = _lib.load()
    assert scratch.dtype == torch.uint8 and scratch.is_contiguous()
    _lib.check(lib.anyv2v_selftest(_p(scratch), scratch.numel(), _stream()), "anyv2v_selftest")
