"""GPU parity checks shared by the pytest files (``-m gpu``) and ``tools/gpu_check.py`` (diagnostic report).

Each check returns a dict(name=..., err=..., tol=..., ok=...).  Kernel-level checks compare the HIP kernels with
plain PyTorch fp32 ops on the same fp16-rounded inputs; model-level checks compare with the CPU oracle
(``oracle/``) and with the golden fixtures generated from the reference's own code (``tests/golden``).
"""
from __future__ import annotations

import math
import os
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from anyv2v_amd import ops  # noqa: E402

DEV = "cuda"
_GLDS_DEFAULT = ops.USE_GLDS


def _effective_cpus() -> int:
    n = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    try:
        quota, period = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        if quota != "max":
            n = min(n, max(1, int(int(quota) / int(period))))
    except Exception:
        pass
    return max(1, n)


# the CPU oracle: never more torch threads than the cgroup CPU quota (the GPU box: 256 hw threads, quota 16)
torch.set_num_threads(min(torch.get_num_threads(), _effective_cpus()))


def _rel(a: torch.Tensor, b: torch.Tensor):
    a = a.float()
    b = b.float().to(a.device)
    denom = b.abs().max().clamp_min(1e-6)
    return float((a - b).abs().max() / denom), float((a - b).norm() / b.norm().clamp_min(1e-12))


def _res(name, got, ref, tol):
    if not torch.isfinite(got.float()).all():
        return dict(name=name, err=float("nan"), l2=float("nan"), tol=tol, ok=False)
    mx, l2 = _rel(got, ref)
    # both metrics are gated: max |diff| / max |ref| and relative L2 (which is never larger than sqrt(N) x the former but is the one
    # a systematic small error moves)
    return dict(name=name, err=mx, l2=l2, tol=tol, ok=bool(mx <= tol and l2 <= tol))


# Kernel-level tolerance: max |got - ref| / max |ref| against PyTorch fp32 on identical fp16 inputs.  The measured worst case over
# all kernel checks is 8.5e-4 (fp16 output rounding, 2^-11 of the largest magnitude, plus fp32 accumulation-order effects;
# tools/gpu_check.py, round 2) -- the bound is ~2.3 x that, so a 3 x regression fails.  (Round 1 used 4e-3 / 6e-3.)
KTOL = 2e-3


def rnd(*shape, scale=1.0, seed=None):
    g = torch.Generator(device="cpu")
    g.manual_seed(seed if seed is not None else (hash(shape) % 100000))
    return (torch.randn(*shape, generator=g) * scale).to(torch.float16).to(DEV)


# ------------------------------------------------------------------------------------------------ layouts
def check_selftest():
    out = []
    scratch = torch.zeros(16384, dtype=torch.uint8, device=DEV)
    g = torch.Generator().manual_seed(5)
    A16 = torch.randint(-4, 5, (16, 32), generator=g).to(torch.float16)
    B16 = torch.randint(-4, 5, (32, 16), generator=g).to(torch.float16)
    A32 = torch.randint(-4, 5, (32, 16), generator=g).to(torch.float16)
    B32 = torch.randint(-4, 5, (16, 32), generator=g).to(torch.float16)
    host = scratch.cpu()
    host[0:1024] = A16.view(torch.uint8).reshape(-1)
    host[1024:2048] = B16.view(torch.uint8).reshape(-1)
    host[3072:4096] = A32.view(torch.uint8).reshape(-1)
    host[4096:5120] = B32.view(torch.uint8).reshape(-1)
    scratch.copy_(host)
    ops.selftest(scratch)
    torch.cuda.synchronize()
    h = scratch.cpu()
    D16 = h[2048:3072].view(torch.float32).reshape(16, 16)
    D32 = h[5120:9216].view(torch.float32).reshape(32, 32)
    TR = h[9216:9728].view(torch.float16).reshape(64, 4)
    out.append(_res("mfma_16x16x32_f16 layout", D16, A16.float() @ B16.float(), 0.0))
    out.append(_res("mfma_32x32x16_f16 layout", D32, A32.float() @ B32.float(), 0.0))
    # expected tr16 semantics: within each 16-lane group, out[c][j] = in[4 j + (c >> 2)][c & 3]; in[i][e] = 4 (16 g + i) + e
    exp = torch.empty(64, 4)
    for l in range(64):
        gq, c = l // 16, l % 16
        for j in range(4):
            i = 4 * j + (c >> 2)
            exp[l, j] = 4 * (16 * gq + i) + (c & 3)
    r = _res("ds_read_b64_tr_b16 semantics (probe)", TR.float(), exp, 0.0)
    r["dump"] = TR.float()[:20].tolist()
    r["informational"] = True
    out.append(r)
    return out


# ------------------------------------------------------------------------------------------------ gemm
def _gemm_ref(a, w, bias=None, rowvec=None, rowvec_div=0, residual=None, act=0):
    y = a.float() @ w.float().t()
    if bias is not None:
        y = y + bias.float()
    if rowvec is not None:
        idx = torch.arange(y.shape[0], device=y.device) // rowvec_div
        y = y + rowvec.float()[idx]
    if act == ops.ACT_SILU:
        y = F.silu(y)
    elif act == ops.ACT_GELU:
        y = F.gelu(y)
    if residual is not None:
        y = y + residual.float()
    return y


def check_gemm(variants=("reg", "glds", "naive")):
    out = []
    cases = [  # (M, N, K)
        (300, 320, 320), (1000, 512, 512), (257, 64, 128), (128, 4, 320), (4096, 1280, 1280), (77, 640, 1024),
        # large M with ragged M / N tails, 1 and 2 K-tiles (128-row kernel; N = 320 / 640 may take the persistent one)
        (8300, 320, 320), (20001, 640, 1280), (9000, 512, 64), (8192, 4, 128), (12345, 160, 192),
    ]
    for var in variants:
        ops.USE_GLDS = var == "glds"
        naive = var == "naive"
        for (M, N, K) in cases:
            a, w = rnd(M, K), rnd(N, K, scale=1 / math.sqrt(K))
            bias, res = rnd(N), rnd(M, N)
            rv = rnd((M + 49) // 50, N)
            y = ops.gemm(a, w, bias=bias, rowvec=rv, rowvec_div=50, residual=res, naive=naive,
                         out=torch.zeros(M, (N + 7) // 8 * 8, dtype=torch.float16, device=DEV))[:, :N]
            out.append(_res(f"gemm[{var}] M{M} N{N} K{K} +bias+rowvec+res", y, _gemm_ref(a, w, bias, rv, 50, res), KTOL))
        # two sources + SiLU
        a0, a1 = rnd(500, 128), rnd(500, 64)
        w = rnd(320, 192, scale=0.1)
        y = ops.gemm(a0, w, a1=a1, act=ops.ACT_SILU, naive=naive)
        out.append(_res(f"gemm[{var}] two-source + silu", y, _gemm_ref(torch.cat([a0, a1], 1), w, act=ops.ACT_SILU), KTOL))
        # strided A / C views (column windows of wider buffers)
        big = rnd(400, 960)
        w = rnd(320, 320, scale=0.06)
        dst = torch.zeros(400, 640, dtype=torch.float16, device=DEV)
        ops.gemm(big[:, 320:640], w, out=dst[:, 320:], naive=naive)
        out.append(_res(f"gemm[{var}] strided views", dst[:, 320:], _gemm_ref(big[:, 320:640], w), KTOL))
        # GEGLU at small and large M
        for M in (333, 9001):
            dim, inner = 128, 512
            a = rnd(M, dim)
            wfull, bfull = rnd(2 * inner, dim, scale=1 / math.sqrt(dim)), rnd(2 * inner, scale=0.1)
            wh, wg = wfull[:inner].view(inner // 16, 16, dim), wfull[inner:].view(inner // 16, 16, dim)
            wp = torch.stack([wh, wg], 1).reshape(2 * inner, dim).contiguous()
            bp = torch.stack([bfull[:inner].view(-1, 16), bfull[inner:].view(-1, 16)], 1).reshape(-1).contiguous()
            y = ops.gemm(a, wp, bias=bp, act=ops.ACT_GEGLU, naive=naive)
            proj = a.float() @ wfull.float().t() + bfull.float()
            ref = proj[:, :inner] * F.gelu(proj[:, inner:])
            out.append(_res(f"gemm[{var}] GEGLU M{M}", y, ref, KTOL))
    ops.USE_GLDS = _GLDS_DEFAULT
    return out


def check_gemm_big(extra=0, tag="big", exact=True):
    """Persistent 256x320 kernel (gemm_big_kernel), forced with flag bit3 on shapes small enough for the references:
    single / multiple rounds per block, every mode, two-source K loop, bias / temb / residual / GEGLU epilogues.
    ``exact`` = False: the forced kernel sums K in a different order (stream-K: fp32 partial slabs) -- the bit-equality rows become
    5e-4 rows.  ``extra``: further AnyV2VGemmDesc.flags bits, e.g. bit17 (| bit19 / bit20) = the ping-pong kernel gemm_pp_kernel (192- / 256-row
    tiles) on every non-GEGLU case -- same references, same bit-equality with the 128-row kernel."""
    out = []
    saved = ops.GEMM_FLAGS
    ops.GEMM_FLAGS = (saved & ~4) | 8 | extra
    try:
        for (M, N, K, res, rvd) in [(512, 320, 320, True, 0), (1024, 640, 192, False, 128), (256, 960, 64, True, 256),
                                    (256 * 41, 2560, 128, True, 0), (256 * 300, 320, 64, False, 0)]:
            a, w, bias = rnd(M, K), rnd(N, K, scale=1 / math.sqrt(K)), rnd(N)
            r = rnd(M, N) if res else None
            rv = rnd(M // rvd, N) if rvd else None
            y = ops.gemm(a, w, bias=bias, rowvec=rv, rowvec_div=rvd, residual=r)
            out.append(_res(f"gemm[{tag}] M{M} N{N} K{K} res={res} rowvec={bool(rvd)}", y, _gemm_ref(a, w, bias, rv, rvd, r), KTOL))
            yn = ops.gemm(a, w, bias=bias, rowvec=rv, rowvec_div=rvd, residual=r, naive=True)
            out.append(_res(f"gemm[{tag}] == naive kernel M{M} N{N} K{K}", y, yn.float(), 2e-3))
            # the two tile-kernel families accumulate every output element in the same order: BIT-equal without split-K (what lets a
            # batch-hinted launch keep its own kernel family and only take the reference launch's split factor, gemm_plan.cpp)
            ops.GEMM_FLAGS = (saved & ~8) | 4 | 16
            ys = ops.gemm(a, w, bias=bias, rowvec=rv, rowvec_div=rvd, residual=r)
            ops.GEMM_FLAGS = (saved & ~4) | 8 | extra
            out.append(_res(f"gemm[{tag}] bit-equal to the 128-row kernel M{M} N{N} K{K}", y, ys.float(), 0.0 if exact else 5e-4))
        # two-source K loop (skip concat)
        a0, a1 = rnd(768, 128), rnd(768, 64)
        w = rnd(320, 192, scale=0.1)
        y = ops.gemm(a0, w, a1=a1)
        out.append(_res(f"gemm[{tag}] two-source", y, _gemm_ref(torch.cat([a0, a1], 1), w), KTOL))
        # GEGLU, one and several rounds
        for M in (512, 256 * 70):
            dim, inner = 128, 640
            a = rnd(M, dim)
            wfull, bfull = rnd(2 * inner, dim, scale=1 / math.sqrt(dim)), rnd(2 * inner, scale=0.1)
            wh, wg = wfull[:inner].view(inner // 16, 16, dim), wfull[inner:].view(inner // 16, 16, dim)
            wp = torch.stack([wh, wg], 1).reshape(2 * inner, dim).contiguous()
            bp = torch.stack([bfull[:inner].view(-1, 16), bfull[inner:].view(-1, 16)], 1).reshape(-1).contiguous()
            y = ops.gemm(a, wp, bias=bp, act=ops.ACT_GEGLU)
            proj = a.float() @ wfull.float().t() + bfull.float()
            out.append(_res(f"gemm[{tag}] GEGLU M{M}", y, proj[:, :inner] * F.gelu(proj[:, inner:]), KTOL))
        # rastered tile order of wide-N launches (8 x 4 super-tiles per XCD round; flags bits 13-16): every order computes each
        # output tile with the same K loop -> BIT-equal to the classic order; ragged M (holes in the last super-tile row),
        # plain and GEGLU epilogues, a forced order on a launch the auto rule would leave alone
        for (M, N, K, geglu) in [(192 * 40 + 70, 2560, 128, False), (192 * 16, 5120, 64, True), (192 * 33, 2560, 64, True)]:
            a, w, bias = rnd(M, K), rnd(N, K, scale=1 / math.sqrt(K)), rnd(N)
            act = ops.ACT_GEGLU if geglu else ops.ACT_NONE
            ops.GEMM_FLAGS = ((saved & ~4) | 8 | extra) | (1 << 13)
            y0 = ops.gemm(a, w, bias=bias, act=act)
            yn = ops.gemm(a, w, bias=bias, act=act, naive=True)
            out.append(_res(f"gemm[{tag}] classic order == naive kernel M{M} N{N} K{K} geglu={geglu}", y0, yn.float(), 2e-3))
            for code, nfast in ((0, 0), (2, 0), (3, 0), (3, 1), (4, 0), (5, 1), (6, 0)):
                ops.GEMM_FLAGS = ((saved & ~4) | 8 | extra) | (code << 13) | (nfast << 16)
                y = ops.gemm(a, w, bias=bias, act=act)
                out.append(_res(f"gemm[{tag}] raster code {code} nfast {nfast} bit-equal to the classic order M{M} N{N} geglu={geglu}", y,
                                y0.float(), 0.0 if exact else 5e-4))
            ops.GEMM_FLAGS = (saved & ~4) | 8 | extra
        # conv 3x3 (stride 1, stride 2, folded upsample) with temb row vector / residual
        n, ci, co, H, W = 8, 64, 320, 16, 16
        x, w, b = rnd(n, ci, H, W), rnd(co, ci, 3, 3, scale=1 / math.sqrt(9 * ci)), rnd(co)
        temb, res = rnd(4, co), rnd(n * H * W, co)
        y = ops.gemm(_to_tokens(x), _pack_conv(w), bias=b, rowvec=temb, rowvec_div=2 * H * W, residual=res,
                     mode=ops.MODE_CONV2D, conv=(H, W, H, W, 1, 0))
        ref = F.conv2d(x.float(), w.float(), b.float(), padding=1) + temb.float().repeat_interleave(2, 0)[:, :, None, None]
        out.append(_res(f"conv3x3[{tag}] s1 +bias+temb+res", y, _to_tokens(ref) + res.float(), KTOL))
        ops.GEMM_FLAGS = (saved & ~8) | 4 | 16
        ys = ops.gemm(_to_tokens(x), _pack_conv(w), bias=b, rowvec=temb, rowvec_div=2 * H * W, residual=res, mode=ops.MODE_CONV2D,
                      conv=(H, W, H, W, 1, 0))
        ops.GEMM_FLAGS = (saved & ~4) | 8 | extra
        out.append(_res(f"conv3x3[{tag}] bit-equal to the 128-row kernel", y, ys.float(), 0.0 if exact else 5e-4))
        y = ops.gemm(_to_tokens(x), _pack_conv(w), bias=b, mode=ops.MODE_CONV2D, conv=(H, W, H // 2, W // 2, 2, 0),
                     M=n * (H // 2) * (W // 2))
        out.append(_res(f"conv3x3[{tag}] stride 2", y, _to_tokens(F.conv2d(x.float(), w.float(), b.float(), stride=2, padding=1)), KTOL))
        y = ops.gemm(_to_tokens(x), _pack_conv(w), bias=b, mode=ops.MODE_CONV2D, conv=(H, W, 2 * H, 2 * W, 1, 1),
                     M=n * 4 * H * W)
        ref = F.conv2d(F.interpolate(x.float(), scale_factor=2.0, mode="nearest"), w.float(), b.float(), padding=1)
        out.append(_res(f"conv3x3[{tag}] nearest-x2 folded", y, _to_tokens(ref), KTOL))
        # two-source conv (up-block skip concat)
        x1 = rnd(n, 128, H, W)
        w2 = rnd(co, ci + 128, 3, 3, scale=1 / math.sqrt(9 * (ci + 128)))
        y = ops.gemm(_to_tokens(x), _pack_conv(w2), a1=_to_tokens(x1), bias=b, mode=ops.MODE_CONV2D, conv=(H, W, H, W, 1, 0))
        ref = F.conv2d(torch.cat([x, x1], 1).float(), w2.float(), b.float(), padding=1)
        out.append(_res(f"conv3x3[{tag}] two-source", y, _to_tokens(ref), KTOL))
        # temporal (3,1,1) conv with residual
        B_, Fr, HW, C = 2, 8, 64, 128
        xt = rnd(B_ * Fr * HW, C)
        wt, bt, rt = rnd(320, C, 3, scale=1 / math.sqrt(3 * C)), rnd(320), rnd(B_ * Fr * HW, 320)
        y = ops.gemm(xt, wt.permute(0, 2, 1).reshape(320, 3 * C).contiguous(), bias=bt, residual=rt, mode=ops.MODE_TEMPORAL,
                     temporal=(Fr, HW))
        x5 = xt.float().view(B_, Fr, HW, C).permute(0, 3, 1, 2)  # [B, C, F, HW]
        ref = F.conv1d(x5.permute(0, 3, 1, 2).reshape(B_ * HW, C, Fr), wt.float(), bt.float(), padding=1)
        ref = ref.view(B_, HW, 320, Fr).permute(0, 3, 1, 2).reshape(B_ * Fr * HW, 320) + rt.float()
        out.append(_res(f"temporal conv[{tag}] +res", y, ref, KTOL))
        # more output tiles than CUs AND several K-tiles per tile: the persistent loop's tile switch with a live LDS-DMA pipeline
        # (conv 3x3 + temb + residual over 72 images of 32 x 32: 288 / 384 tiles, 9 K-tiles; temporal conv: 300 / 400 tiles, 6 K-tiles)
        n, ci, co, H, W = 72, 64, 320, 32, 32
        x, w, b = rnd(n, ci, H, W), rnd(co, ci, 3, 3, scale=1 / math.sqrt(9 * ci)), rnd(co)
        temb, res = rnd(n // 8, co), rnd(n * H * W, co)
        for r_ in (res, None):
            y = ops.gemm(_to_tokens(x), _pack_conv(w), bias=b, rowvec=temb, rowvec_div=8 * H * W, residual=r_, mode=ops.MODE_CONV2D,
                         conv=(H, W, H, W, 1, 0))
            ref = F.conv2d(x.float(), w.float(), b.float(), padding=1) + temb.float().repeat_interleave(8, 0)[:, :, None, None]
            out.append(_res(f"conv3x3[{tag}] 288+ tiles x 9 K-tiles res={r_ is not None}", y, _to_tokens(ref) + (r_.float() if r_ is not None else 0.0), KTOL))
            ops.GEMM_FLAGS = (saved & ~8) | 4 | 16
            ys = ops.gemm(_to_tokens(x), _pack_conv(w), bias=b, rowvec=temb, rowvec_div=8 * H * W, residual=r_, mode=ops.MODE_CONV2D,
                          conv=(H, W, H, W, 1, 0))
            ops.GEMM_FLAGS = (saved & ~4) | 8 | extra
            out.append(_res(f"conv3x3[{tag}] 288+ tiles bit-equal to the 128-row kernel res={r_ is not None}", y, ys.float(), 0.0 if exact else 5e-4))
        B_, Fr, HW, C = 3, 16, 1600, 128
        xt = rnd(B_ * Fr * HW, C)
        wt, bt, rt = rnd(320, C, 3, scale=1 / math.sqrt(3 * C)), rnd(320), rnd(B_ * Fr * HW, 320)
        y = ops.gemm(xt, wt.permute(0, 2, 1).reshape(320, 3 * C).contiguous(), bias=bt, residual=rt, mode=ops.MODE_TEMPORAL, temporal=(Fr, HW))
        ref = F.conv1d(xt.float().view(B_, Fr, HW, C).permute(0, 2, 3, 1).reshape(B_ * HW, C, Fr), wt.float(), bt.float(), padding=1)
        ref = ref.view(B_, HW, 320, Fr).permute(0, 3, 1, 2).reshape(B_ * Fr * HW, 320) + rt.float()
        out.append(_res(f"temporal conv[{tag}] 300+ tiles x 6 K-tiles +res", y, ref, KTOL))
        a, w2, bb = rnd(256 * 300 + 40, 1280), rnd(640, 1280, scale=1 / math.sqrt(1280)), rnd(640)
        r2 = rnd(256 * 300 + 40, 640)
        y = ops.gemm(a, w2, bias=bb, residual=r2)
        out.append(_res(f"gemm[{tag}] FF-down shape 76840 x 640 x 1280 +res (ragged M)", y, _gemm_ref(a, w2, bb, None, 0, r2), KTOL))
        ops.GEMM_FLAGS = (saved & ~8) | 4 | 16
        ys = ops.gemm(a, w2, bias=bb, residual=r2)
        ops.GEMM_FLAGS = (saved & ~4) | 8 | extra
        out.append(_res(f"gemm[{tag}] FF-down shape bit-equal to the 128-row kernel", y, ys.float(), 0.0 if exact else 5e-4))
    finally:
        ops.GEMM_FLAGS = saved
    return out


def check_conv_halo():
    """gemm_swh_kernel (round 6: 3x3 stride-1 convolution whose A operand is staged ONCE per (dy, channel slice) as an LDS patch and
    read three times with a one-pixel address shift, K order (dy, slice, dx)), forced with flags bit28 on every image width it
    takes (16 / 32 / 64): one / two sources, bias / temb row vector / residual epilogues, tile counts below and above the CU count,
    row counts that are not a multiple of the 192-row tile (images cut by a tile boundary), against F.conv2d in fp32 (kernel tolerance)
    and against the tap-gather kernels' result (5e-4: the same products in another summation order)."""
    out = []
    saved = ops.GEMM_FLAGS
    try:
        for (n, H, c0, c1, co, res, rvd) in [(3, 64, 64, 0, 320, False, 0), (2, 64, 128, 64, 320, True, 0), (6, 32, 128, 0, 640, False, 2),
                                             (70, 32, 64, 0, 320, True, 0), (5, 16, 192, 0, 320, False, 0), (13, 16, 64, 64, 640, True, 0),
                                             (300, 16, 64, 0, 320, False, 100)]:
            x0 = rnd(n, c0, H, H)
            x1 = rnd(n, c1, H, H) if c1 else None
            ci = c0 + c1
            w, b = rnd(co, ci, 3, 3, scale=1 / math.sqrt(9 * ci)), rnd(co)
            r = rnd(n * H * H, co) if res else None
            temb = rnd(n // rvd, co) if rvd else None
            kw = dict(bias=b, a1=None if x1 is None else _to_tokens(x1), rowvec=temb, rowvec_div=rvd * H * H if rvd else 0, residual=r,
                      mode=ops.MODE_CONV2D, conv=(H, H, H, H, 1, 0))
            ops.GEMM_FLAGS = saved | (1 << 28)
            y = ops.gemm(_to_tokens(x0), _pack_conv(w), **kw)
            ops.GEMM_FLAGS = saved
            yd = ops.gemm(_to_tokens(x0), _pack_conv(w), **kw)
            xx = x0 if x1 is None else torch.cat([x0, x1], 1)
            ref = F.conv2d(xx.float(), w.float(), b.float(), padding=1)
            if rvd:
                ref = ref + temb.float().repeat_interleave(rvd, 0)[:, :, None, None]
            ref = _to_tokens(ref) + (r.float() if res else 0.0)
            tag = f"{n} x {H}x{H}, {c0}+{c1} -> {co}, res={res} temb={bool(rvd)}"
            out.append(_res(f"conv3x3[halo] {tag} vs F.conv2d fp32", y, ref, KTOL))
            out.append(_res(f"conv3x3[halo] {tag} vs the tap-gather kernels", y, yd.float(), 5e-4))
    finally:
        ops.GEMM_FLAGS = saved
    return out


def _geglu_pack(wfull, bfull, inner):
    dim = wfull.shape[1]
    wh, wg = wfull[:inner].view(inner // 16, 16, dim), wfull[inner:].view(inner // 16, 16, dim)
    wp = torch.stack([wh, wg], 1).reshape(2 * inner, dim).contiguous()
    bp = torch.stack([bfull[:inner].view(-1, 16), bfull[inner:].view(-1, 16)], 1).reshape(-1).contiguous()
    return wp, bp


def check_gemm_ws():
    """Weight-stationary K = 320 kernel (gemm_ws.hip), forced with flag bit10 at sizes the references finish quickly, and
    through the dispatch threshold at the bench's own row counts: one / several strips per wave, ragged M (row guards and
    clamped look-ahead), 1 / 2 / 6 / 16 slabs, bias / residual / GEGLU epilogues, strided A / C / R views, and equality
    with the tile kernels it replaces (flag bit9)."""
    out = []
    saved = ops.GEMM_FLAGS
    K = 320
    try:
        for (M, N, res) in [(100, 160, False), (2049, 320, True), (4113, 960, False), (9000, 320, True), (33000, 320, True),
                            (70001, 960, False)]:
            a, w, bias = rnd(M, K), rnd(N, K, scale=1 / math.sqrt(K)), rnd(N)
            r = rnd(M, N) if res else None
            ops.GEMM_FLAGS = saved | 1024
            y = ops.gemm(a, w, bias=bias, residual=r)
            out.append(_res(f"gemm[ws] M{M} N{N} res={res}", y, _gemm_ref(a, w, bias, residual=r), KTOL))
            ops.GEMM_FLAGS = saved | 512
            yt = ops.gemm(a, w, bias=bias, residual=r)
            out.append(_res(f"gemm[ws] == tile kernels M{M} N{N}", y, yt.float(), 1e-3))
        # no bias; column windows of wider buffers for A, C and R (the V-only projection writes qkv[:, 640:960])
        ops.GEMM_FLAGS = saved | 1024
        big, w = rnd(5000, 960), rnd(320, K, scale=1 / math.sqrt(K))
        dst = torch.zeros(5000, 960, dtype=torch.float16, device=DEV)
        rbuf = rnd(5000, 640)
        ops.gemm(big[:, 320:640], w, out=dst[:, 640:], residual=rbuf[:, 320:])
        out.append(_res("gemm[ws] strided A / C / R views", dst[:, 640:], _gemm_ref(big[:, 320:640], w, residual=rbuf[:, 320:]), KTOL))
        out.append(_res("gemm[ws] strided C leaves the other columns alone", dst[:, :640], torch.zeros(5000, 640), 0.0))
        # GEGLU: 2 slabs (inner 160) and 16 slabs (inner 1280, the layer's own width)
        for (M, inner) in [(777, 160), (3000, 1280), (40000, 1280)]:
            a = rnd(M, K)
            wfull, bfull = rnd(2 * inner, K, scale=1 / math.sqrt(K)), rnd(2 * inner, scale=0.1)
            wp, bp = _geglu_pack(wfull, bfull, inner)
            y = ops.gemm(a, wp, bias=bp, act=ops.ACT_GEGLU)
            proj = a.float() @ wfull.float().t() + bfull.float()
            out.append(_res(f"gemm[ws] GEGLU M{M} inner{inner}", y, proj[:, :inner] * F.gelu(proj[:, inner:]), KTOL))
        # transformer_in's width (K = 512): 64-column slabs (128 for GEGLU), 16 K-steps, ring of 8
        ops.GEMM_FLAGS = saved | 1024
        K5 = 512
        for (M, N, res) in [(4100, 512, True), (9001, 512, False), (33000, 512, True)]:
            a, w, bias = rnd(M, K5), rnd(N, K5, scale=1 / math.sqrt(K5)), rnd(N)
            r = rnd(M, N) if res else None
            ops.GEMM_FLAGS = saved | 1024
            y = ops.gemm(a, w, bias=bias, residual=r)
            out.append(_res(f"gemm[ws] K512 M{M} N{N} res={res}", y, _gemm_ref(a, w, bias, residual=r), KTOL))
            ops.GEMM_FLAGS = saved | 512
            out.append(_res(f"gemm[ws] K512 == tile kernels M{M} N{N}", y, ops.gemm(a, w, bias=bias, residual=r).float(), 1e-3))
        ops.GEMM_FLAGS = saved | 1024
        for (M, inner) in [(3000, 2048), (777, 128)]:
            a = rnd(M, K5)
            wfull, bfull = rnd(2 * inner, K5, scale=1 / math.sqrt(K5)), rnd(2 * inner, scale=0.1)
            wp, bp = _geglu_pack(wfull, bfull, inner)
            y = ops.gemm(a, wp, bias=bp, act=ops.ACT_GEGLU)
            proj = a.float() @ wfull.float().t() + bfull.float()
            out.append(_res(f"gemm[ws] K512 GEGLU M{M} inner{inner}", y, proj[:, :inner] * F.gelu(proj[:, inner:]), KTOL))
        # the dispatch threshold itself (no flag): the inversion step's row count, with residual; bit-reproducible
        ops.GEMM_FLAGS = saved
        M = 65536
        a, w, bias, r = rnd(M, K), rnd(320, K, scale=1 / math.sqrt(K)), rnd(320), rnd(M, 320)
        y = ops.gemm(a, w, bias=bias, residual=r)
        out.append(_res("gemm[ws] dispatch M65536 N320 +res", y, _gemm_ref(a, w, bias, residual=r), KTOL))
        out.append(_res("gemm[ws] bit-reproducible", y, ops.gemm(a, w, bias=bias, residual=r).float(), 0.0))
        ops.GEMM_FLAGS = saved | 512
        out.append(_res("gemm[ws] dispatch == tile kernels", y, ops.gemm(a, w, bias=bias, residual=r).float(), 1e-3))
    finally:
        ops.GEMM_FLAGS = saved
    return out


def check_gemm_ws_ln():
    """LayerNorm folded into the weight-stationary kernel (``ops.gemm(..., ln=...)``): un-normalised rows in, gamma / beta folded
    into the weights (``ops.ln_fold``), row statistics taken by the matrix pipe.  Against torch fp32 LayerNorm -> Linear (-> GEGLU)
    on the same fp16 inputs, and against the unfused HIP path (layernorm kernel + GEMM); rows with a large mean (|mean| = 6 sigma:
    the fold subtracts mean x column sums) and ragged row counts included."""
    out = []
    eps = 1e-5
    for (M, K, N, act, shift) in [(40000, 320, 960, 0, 0.0), (33001, 320, 320, 0, 6.0), (36000, 320, 2560, ops.ACT_GEGLU, 0.0),
                                  (34000, 512, 4096, ops.ACT_GEGLU, 3.0), (33001, 320, 320, 0, 12.0), (33001, 320, 960, 0, 24.0)]:
        x = (rnd(M, K).float() * (1.0 + 0.5 * torch.rand(M, 1, device=DEV)) + shift * torch.randn(M, 1, device=DEV)).half()
        gamma, beta = (1.0 + 0.3 * rnd(K).float()).half(), (0.2 * rnd(K, seed=7).float()).half()
        geglu = act == ops.ACT_GEGLU
        wfull = rnd(N, K, scale=1 / math.sqrt(K))
        bfull = rnd(N, scale=0.1) if geglu or N != 960 else None      # attention's to_q / to_k / to_v have no bias
        y_ln = F.layer_norm(x.float(), (K,), gamma.float(), beta.float(), eps)
        proj = y_ln @ wfull.float().t() + (bfull.float() if bfull is not None else 0.0)
        if geglu:
            inner = N // 2
            ref = proj[:, :inner] * F.gelu(proj[:, inner:])
            wp, bp = _geglu_pack(wfull, bfull, inner)
        else:
            ref, wp, bp = proj, wfull, bfull
        wq, bq, c1 = ops.ln_fold(wp, bp, gamma, beta)
        assert ops.ln_gemm_supported(M, K, N, act)
        y = ops.gemm(x, wq, bias=bq, act=act, ln=(c1, eps))
        out.append(_res(f"gemm[ws+LN] M{M} K{K} N{N} act{act} mean-shift {shift}: vs torch fp32 LayerNorm -> Linear", y, ref, KTOL))
        h = ops.layernorm(x, gamma, beta, eps)
        yu = ops.gemm(h, wp, bias=bp, act=act)
        out.append(_res(f"gemm[ws+LN] M{M} K{K} N{N}: vs layernorm kernel + GEMM", y, yu.float(), 3e-3))
    # shapes outside the fold's coverage are refused loudly, not silently computed without the LayerNorm
    try:
        ops.gemm(rnd(64, 640), rnd(640, 640), ln=(torch.zeros(640, device=DEV), eps))
        out.append(dict(name="gemm[ws+LN] unsupported shape is refused", err=1.0, l2=1.0, tol=0.0, ok=False))
    except Exception as e:
        out.append(dict(name=f"gemm[ws+LN] unsupported shape is refused ({type(e).__name__})", err=0.0, l2=0.0, tol=0.0, ok=True))
    return out


def check_ff_fused():
    """anyv2v_ff_geglu_f16 (ff_fused.hip): GEGLU up-projection + down-projection (+ residual) of the 320-channel blocks in one kernel vs
    torch fp32 on the un-packed weights (hidden rounded to fp16 once, as the unfused GEGLU GEMM stores it), and vs the unfused pair of
    GEMMs; one strip, ragged tails, more strips than the 1024 pair slots (several rounds: the weight rings wrap), with / without residual."""
    out = []
    C, H = 320, 1280
    w1, b1 = rnd(2 * H, C, scale=1 / math.sqrt(C)), rnd(2 * H, scale=0.1)
    w2, b2 = rnd(C, H, scale=1 / math.sqrt(H)), rnd(C, scale=0.1)
    w1p, b1p = _geglu_pack(w1, b1, H)
    w2s = ops.ff_pack_w2(w2)
    for M, res in [(32, False), (32 * 5 + 7, True), (128 * 256, True), (128 * 256 * 2 + 32 * 3 + 5, True), (196608, False)]:
        x = rnd(M, C)
        r = rnd(M, C) if res else None
        y = ops.ff_geglu(x, w1p, b1p, w2s, b2, residual=r)
        proj = x.float() @ w1.float().t() + b1.float()
        hid = (proj[:, :H] * F.gelu(proj[:, H:])).half().float()
        ref = (hid @ w2.float().t() + b2.float()).half().float()
        if res:
            ref = ref + r.float()
        out.append(_res(f"ff_fused M{M} res={res} vs torch fp32", y, ref, KTOL))
        g = ops.gemm(x, w1p, bias=b1p, act=ops.ACT_GEGLU)
        yu = ops.gemm(g, w2, bias=b2, residual=r)
        out.append(_res(f"ff_fused M{M} res={res} vs the unfused GEGLU GEMM + Linear", y, yu.float(), KTOL))
    return out


def check_gemm_splitk():
    """Split-K path (launches that cannot fill the chip and have >= 16 K-tiles; fp32 partial tiles + a second pass that
    sums them in split order): against torch, against the unsplit kernel (flag bit4), and bit-reproducibility.
    (A fused last-arriver reduction was tried and dropped: the device-scope fences it needs write back / invalidate the
    per-XCD L2 on gfx950 and cost far more than the second launch -- DESIGN.md.)"""
    out = []
    saved = ops.GEMM_FLAGS
    try:
        # 8x8-level conv: M = 3 clips x 16 frames x 64 px, K = 2304 (36 K-tiles), 24 x 2 = 48 tiles -> 4 splits
        n, ci, co, H, W = 48, 256, 320, 8, 8
        x, w, b = rnd(n, ci, H, W), rnd(co, ci, 3, 3, scale=1 / math.sqrt(9 * ci)), rnd(co)
        temb, res = rnd(3, co), rnd(n * H * W, co)
        kw = dict(bias=b, rowvec=temb, rowvec_div=16 * H * W, residual=res, mode=ops.MODE_CONV2D, conv=(H, W, H, W, 1, 0))
        ref = F.conv2d(x.float(), w.float(), b.float(), padding=1) + temb.float().repeat_interleave(16, 0)[:, :, None, None]
        ref = _to_tokens(ref) + res.float()
        xt, wp = _to_tokens(x), _pack_conv(w)
        ys = [ops.gemm(xt, wp, **kw) for _ in range(3)]
        out.append(_res("conv3x3[split-K] vs torch", ys[0], ref, KTOL))
        out.append(_res("conv3x3[split-K] bit-reproducible", ys[0], ys[2].float(), 0.0))
        ops.GEMM_FLAGS = saved | 16
        y_one = ops.gemm(xt, wp, **kw)
        out.append(_res("conv3x3[split-K] vs unsplit kernel", ys[0], y_one.float(), 2e-3))
        ops.GEMM_FLAGS = saved
        # the same launch with an activation: gemm_splitk_reduce_kernel applies it to the summed partial tiles (+ bias + temb) and
        # rounds to fp16 before the residual add (the reference adds in fp32: inside KTOL).  An activation keeps the launch off the
        # persistent kernel, the 128-row kernel splits it 4 ways (tests/test_gemm_plan_host.py: splitk_conv_silu / _gelu).
        pre = _to_tokens(F.conv2d(x.float(), w.float(), b.float(), padding=1) + temb.float().repeat_interleave(16, 0)[:, :, None, None])
        for act, tag in ((ops.ACT_SILU, "SiLU"), (ops.ACT_GELU, "GELU")):
            ref_act = (F.silu(pre) if act == ops.ACT_SILU else F.gelu(pre)) + res.float()
            ya = [ops.gemm(xt, wp, act=act, **kw) for _ in range(3)]
            out.append(_res(f"conv3x3[split-K] + {tag} vs torch", ya[0], ref_act, KTOL))
            same = bool(torch.equal(ya[0], ya[1]) and torch.equal(ya[0], ya[2]))
            out.append(dict(name=f"conv3x3[split-K] + {tag} bit-reproducible over three runs", err=0.0 if same else 1.0, l2=0.0, tol=0.0, ok=same))
            ops.GEMM_FLAGS = saved | 16
            out.append(_res(f"conv3x3[split-K] + {tag} vs unsplit kernel", ya[0], ops.gemm(xt, wp, act=act, **kw).float(), 2e-3))
            ops.GEMM_FLAGS = saved
        # same level, N = 1280: split-K work items of the persistent 192x320 kernel (16 x 4 tiles x 4 splits = one round);
        # M = 3000 is not a multiple of 192 (row guards), compared with the 128-row kernel's split path (flag bit2) too
        n, ci, co = 48, 640, 1280
        x, w, b = rnd(n, ci, H, W), rnd(co, ci, 3, 3, scale=1 / math.sqrt(9 * ci)), rnd(co)
        temb, res = rnd(3, co), rnd(n * H * W, co)
        kw = dict(bias=b, rowvec=temb, rowvec_div=16 * H * W, residual=res, mode=ops.MODE_CONV2D, conv=(H, W, H, W, 1, 0))
        ref = F.conv2d(x.float(), w.float(), b.float(), padding=1) + temb.float().repeat_interleave(16, 0)[:, :, None, None]
        ref = _to_tokens(ref) + res.float()
        xt, wp = _to_tokens(x), _pack_conv(w)
        ys = [ops.gemm(xt, wp, **kw) for _ in range(3)]
        out.append(_res("conv3x3[persistent split-K] vs torch", ys[0], ref, KTOL))
        out.append(_res("conv3x3[persistent split-K] bit-reproducible", ys[0], ys[2].float(), 0.0))
        ops.GEMM_FLAGS = saved | 4
        out.append(_res("conv3x3[persistent split-K] vs 128-row split-K", ys[0], ops.gemm(xt, wp, **kw).float(), 2e-3))
        ops.GEMM_FLAGS = saved
        a, wl, rl = rnd(3000, 5120), rnd(1280, 5120, scale=1 / math.sqrt(5120)), rnd(3000, 1280)
        y = ops.gemm(a, wl, bias=rnd(1280) * 0, residual=rl)
        out.append(_res("gemm[persistent split-K] M3000 N1280 K5120 +res", y, _gemm_ref(a, wl) + rl.float(), KTOL))
        # linear, long K, small M
        a, wl = rnd(1024, 5120), rnd(1280, 5120, scale=1 / math.sqrt(5120))
        y = ops.gemm(a, wl, bias=rnd(1280) * 0)
        out.append(_res("gemm[split-K] M1024 N1280 K5120", y, _gemm_ref(a, wl), KTOL))
    finally:
        ops.GEMM_FLAGS = saved
    return out


def _to_tokens(x):  # NCHW -> [(n h w), c]
    n, c, h, w = x.shape
    return x.permute(0, 2, 3, 1).reshape(n * h * w, c).contiguous()


def _pack_conv(w):  # [Co, Ci, 3, 3] -> [Co, 9*Ci]
    return w.permute(0, 2, 3, 1).reshape(w.shape[0], -1).contiguous()


def check_conv(variants=("reg", "glds", "naive")):
    out = []
    for var in variants:
        ops.USE_GLDS = var == "glds"
        naive = var == "naive"
        # 3x3 stride 1 with bias + temb rowvec + residual
        n, ci, co, H, W = 6, 64, 128, 12, 10
        x, w, b = rnd(n, ci, H, W), rnd(co, ci, 3, 3, scale=1 / math.sqrt(9 * ci)), rnd(co)
        temb, res = rnd(3, co), rnd(n * H * W, co)
        y = ops.gemm(_to_tokens(x), _pack_conv(w), bias=b, rowvec=temb, rowvec_div=2 * H * W, residual=res,
                     mode=ops.MODE_CONV2D, conv=(H, W, H, W, 1, 0), naive=naive)
        ref = F.conv2d(x.float(), w.float(), b.float(), padding=1)
        ref = ref + temb.float().repeat_interleave(2, 0)[:, :, None, None]
        ref = _to_tokens(ref) + res.float()
        out.append(_res(f"conv3x3[{var}] s1 +bias+temb+res", y, ref, KTOL))
        # stride 2
        Ho, Wo = H // 2, W // 2
        y = ops.gemm(_to_tokens(x), _pack_conv(w), bias=b, mode=ops.MODE_CONV2D, conv=(H, W, Ho, Wo, 2, 0),
                     M=n * Ho * Wo, naive=naive)
        ref = _to_tokens(F.conv2d(x.float(), w.float(), b.float(), stride=2, padding=1))
        out.append(_res(f"conv3x3[{var}] stride 2", y, ref, KTOL))
        # nearest x2 upsample folded
        y = ops.gemm(_to_tokens(x), _pack_conv(w), bias=b, mode=ops.MODE_CONV2D, conv=(H, W, 2 * H, 2 * W, 1, 1),
                     M=n * 4 * H * W, naive=naive)
        ref = _to_tokens(F.conv2d(F.interpolate(x.float(), scale_factor=2.0, mode="nearest"), w.float(), b.float(), padding=1))
        out.append(_res(f"conv3x3[{var}] upsample x2", y, ref, KTOL))
        # two sources (skip concat)
        x1 = rnd(n, 128, H, W)
        w2 = rnd(co, ci + 128, 3, 3, scale=1 / math.sqrt(9 * (ci + 128)))
        y = ops.gemm(_to_tokens(x), _pack_conv(w2), a1=_to_tokens(x1), mode=ops.MODE_CONV2D, conv=(H, W, H, W, 1, 0), naive=naive)
        ref = _to_tokens(F.conv2d(torch.cat([x, x1], 1).float(), w2.float(), padding=1))
        out.append(_res(f"conv3x3[{var}] two-source", y, ref, KTOL))
        # temporal (3,1,1)
        B, Fr, HW, C = 2, 5, 24, 64
        xt = rnd(B * Fr * HW, C)
        w3, b3 = rnd(C, C, 3, 1, 1, scale=1 / math.sqrt(3 * C)), rnd(C)
        wp = w3[:, :, :, 0, 0].permute(0, 2, 1).reshape(C, -1).contiguous()
        y = ops.gemm(xt, wp, bias=b3, mode=ops.MODE_TEMPORAL, temporal=(Fr, HW), residual=xt, naive=naive)
        x5 = xt.view(B, Fr, HW, C).permute(0, 3, 1, 2).unsqueeze(-1).float()  # [B,C,F,HW,1]
        ref = F.conv3d(x5, w3.float(), b3.float(), padding=(1, 0, 0)) + x5
        ref = ref.squeeze(-1).permute(0, 2, 3, 1).reshape(B * Fr * HW, C)
        out.append(_res(f"temporal conv[{var}] +res", y, ref, KTOL))
        # large M (>= 8192 rows): conv s1 two-source + temb + res, upsample, temporal
        n, ci, c1, co, H, W = 6, 64, 128, 160, 40, 36
        x, x1 = rnd(n, ci, H, W), rnd(n, c1, H, W)
        w2, b = rnd(co, ci + c1, 3, 3, scale=1 / math.sqrt(9 * (ci + c1))), rnd(co)
        temb, res = rnd(3, co), rnd(n * H * W, co)
        y = ops.gemm(_to_tokens(x), _pack_conv(w2), a1=_to_tokens(x1), bias=b, rowvec=temb, rowvec_div=2 * H * W,
                     residual=res, mode=ops.MODE_CONV2D, conv=(H, W, H, W, 1, 0), naive=naive)
        ref = F.conv2d(torch.cat([x, x1], 1).float(), w2.float(), b.float(), padding=1)
        ref = _to_tokens(ref + temb.float().repeat_interleave(2, 0)[:, :, None, None]) + res.float()
        out.append(_res(f"conv3x3[{var}] large-M two-source +bias+temb+res", y, ref, KTOL))
        xs = rnd(3, 64, 30, 30)
        ws = rnd(320, 64, 3, 3, scale=1 / math.sqrt(9 * 64))
        y = ops.gemm(_to_tokens(xs), _pack_conv(ws), mode=ops.MODE_CONV2D, conv=(30, 30, 60, 60, 1, 1), M=3 * 3600, naive=naive)
        ref = _to_tokens(F.conv2d(F.interpolate(xs.float(), scale_factor=2.0, mode="nearest"), ws.float(), padding=1))
        out.append(_res(f"conv3x3[{var}] large-M upsample x2", y, ref, KTOL))
        B, Fr, HW, C = 2, 8, 600, 128
        xt = rnd(B * Fr * HW, C)
        w3, b3 = rnd(C, C, 3, 1, 1, scale=1 / math.sqrt(3 * C)), rnd(C)
        wp = w3[:, :, :, 0, 0].permute(0, 2, 1).reshape(C, -1).contiguous()
        y = ops.gemm(xt, wp, bias=b3, mode=ops.MODE_TEMPORAL, temporal=(Fr, HW), residual=xt, naive=naive)
        x5 = xt.view(B, Fr, HW, C).permute(0, 3, 1, 2).unsqueeze(-1).float()
        ref = (F.conv3d(x5, w3.float(), b3.float(), padding=(1, 0, 0)) + x5).squeeze(-1).permute(0, 2, 3, 1).reshape(B * Fr * HW, C)
        out.append(_res(f"temporal conv[{var}] large-M +res", y, ref, KTOL))
    # tiny-channel conv goes through the reference-grade kernel automatically
    x, w, b = rnd(2, 4, 8, 8), rnd(16, 4, 3, 3, scale=0.2), rnd(16)
    y = ops.gemm(_to_tokens(x), _pack_conv(w), bias=b, act=ops.ACT_SILU, mode=ops.MODE_CONV2D, conv=(8, 8, 8, 8, 1, 0))
    out.append(_res("conv3x3 Cin=4 (naive path) + silu", y, _to_tokens(F.silu(F.conv2d(x.float(), w.float(), b.float(), padding=1))), KTOL))
    ops.USE_GLDS = _GLDS_DEFAULT
    return out


# ------------------------------------------------------------------------------------------------ norms
def check_norms():
    out = []
    stats = torch.zeros(ops.gn_scratch_floats(64, 1), dtype=torch.float32, device=DEV)
    for (n, c, hw, silu, eps) in [(6, 320, 100, True, 1e-5), (3, 64, 64, False, 1e-6), (4, 1280, 64, True, 1e-5)]:
        x = rnd(n * hw, c) + 0.5
        ga, be = rnd(c) + 1.0, rnd(c)
        y = ops.groupnorm(x, ga, be, stats, hw, groups=32, eps=eps, silu=silu)
        ref = F.group_norm(x.float().view(n, hw, c).permute(0, 2, 1), 32, ga.float(), be.float(), eps)
        if silu:
            ref = F.silu(ref)
        out.append(_res(f"groupnorm 4-D n{n} c{c} hw{hw} silu={silu}", y, ref.permute(0, 2, 1).reshape(n * hw, c), KTOL))
    # 5-D (per clip over frames) + two sources with a group straddling the boundary (1280 + 640 -> 60 ch/group)
    B, Fr, hw, c0, c1 = 2, 3, 16, 1280, 640
    x0, x1 = rnd(B * Fr * hw, c0), rnd(B * Fr * hw, c1) * 2 + 1
    ga, be = rnd(c0 + c1) + 1.0, rnd(c0 + c1)
    y = ops.groupnorm(x0, ga, be, stats, Fr * hw, x1=x1, groups=32, eps=1e-5, silu=True)
    xc = torch.cat([x0, x1], 1).float().view(B, Fr * hw, c0 + c1).permute(0, 2, 1)
    ref = F.silu(F.group_norm(xc, 32, ga.float(), be.float(), 1e-5)).permute(0, 2, 1).reshape(B * Fr * hw, c0 + c1)
    out.append(_res("groupnorm 5-D two-source silu", y, ref, KTOL))
    # sharded statistics (frame-parallel clips): partial + apply(shards=1) IS the one-call kernel pair (bit-identical);
    # a clip split into two pixel halves, partial sums added as the all-reduce would, equals the unsharded result
    y1 = ops.groupnorm(x0, ga, be, stats, Fr * hw, x1=x1, groups=32, eps=1e-5, silu=True, shard=(1, lambda t: t))
    out.append(_res("groupnorm two-phase (shards=1) == one call", y1, y.float(), 0.0 if DEV != "cpu" else 2e-3))
    xs = x0.view(B, Fr, hw, c0)
    halves = [xs[:, :, i * hw // 2:(i + 1) * hw // 2].reshape(-1, c0).contiguous() for i in range(2)]
    ga0, be0 = ga[:c0].contiguous(), be[:c0].contiguous()
    full = ops.groupnorm(x0, ga0, be0, stats, Fr * hw, groups=32, eps=1e-5, silu=True).view(B, Fr, hw, c0)
    got = gn_sharded_emulated(halves, None, ga0, be0, Fr * hw // 2, eps=1e-5, silu=True)[0]   # rank 0 of 2
    out.append(_res("groupnorm sharded over 2 pixel halves vs unsharded", got,
                    full[:, :, :hw // 2].reshape(-1, c0).float(), 2e-3))
    for (m, c) in [(1000, 320), (77, 1280), (333, 512), (50, 4), (64, 64)]:
        x = rnd(m, c) * 2 + 0.3
        ga, be = rnd(c) + 1.0, rnd(c)
        y = ops.layernorm(x, ga, be, 1e-5)
        out.append(_res(f"layernorm m{m} c{c}", y, F.layer_norm(x.float(), (c,), ga.float(), be.float(), 1e-5), KTOL))
    return out


# ------------------------------------------------------------------------------------------------ norms at production shapes
# References here are float64 two-pass statistics on the GPU, on the same fp16 inputs (not F.group_norm in fp32: MIOpen's fp32
# paths have misbehaved at large sizes, profiles/r04_eager_size_probe_fp32.txt).
def _gn_ref64(x0, x1, ga, be, rpg, groups, eps, silu):
    x = x0.double() if x1 is None else torch.cat([x0.double(), x1.double()], 1)
    M, C = x.shape
    xg = x.view(M // rpg, rpg, groups, C // groups)
    mean = xg.mean((1, 3), keepdim=True)
    var = (xg - mean).square_().mean((1, 3), keepdim=True)
    y = (xg - mean).mul_(torch.rsqrt(var + eps)).view(M, C).mul_(ga.double()).add_(be.double())
    return y * torch.sigmoid(y) if silu else y


def _ln_ref64(x, ga, be, eps):
    xd = x.double()
    mean = xd.mean(1, keepdim=True)
    var = (xd - mean).square_().mean(1, keepdim=True)
    return (xd - mean).mul_(torch.rsqrt(var + eps)).mul_(ga.double()).add_(be.double())


def _gn_run(x0, x1, ga, be, rpg, groups, eps, silu, shard=None):
    M = x0.shape[0]
    stats = torch.zeros(ops.gn_scratch_floats(M, rpg, groups), dtype=torch.float32, device=DEV)
    return ops.groupnorm(x0, ga, be, stats, rpg, x1=x1, groups=groups, eps=eps, silu=silu, shard=shard)


def _gn_row(name, x0, x1, ga, be, rpg, groups, eps, silu, tol=KTOL):
    y = _gn_run(x0, x1, ga, be, rpg, groups, eps, silu)
    return _res(name, y, _gn_ref64(x0, x1, ga, be, rpg, groups, eps, silu), tol)


def _affine(C, seed):
    return (rnd(C, seed=seed) * 0.3 + 1.0).half(), (rnd(C, seed=seed + 1) * 0.2).half()


def _offset_data(nsg, rpg, C, groups, offset, seed, sigma=1.0):
    """Per (statistics group, channel group): a random sign x ``offset`` sigma on top of N(0, sigma^2) noise."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    sign = (torch.randint(0, 2, (nsg, 1, groups, 1), generator=g) * 2 - 1).float().to(DEV)
    x = torch.randn(nsg, rpg, groups, C // groups, generator=g).to(DEV) * sigma + sign * (offset * sigma)
    return x.view(nsg * rpg, C).half()


_NORM_CALLS = None


def recorded_norm_calls():
    """Every distinct ``ops.groupnorm`` signature (C0, C1, rows_per_group, G, eps, silu) and ``ops.layernorm`` signature (C, eps)
    that one forward pass of the product's models issues: the full-width I2VGen-XL UNet at config 1 (8 f x 32^2 latents, B = 1),
    the mini and full-architecture VAE (encode + decode), the ConsistI2V and SEINE UNets at the toy widths of their fixtures.
    Weights are random (the call signatures depend on shapes only)."""
    global _NORM_CALLS
    if _NORM_CALLS is not None:
        return _NORM_CALLS
    import consisti2v_spec as c2spec
    import seine_spec as snspec
    from anyv2v_amd import consisti2v as c2
    from anyv2v_amd import seine as sn
    from anyv2v_amd.unet import I2VGenXLUNet, I2VGenXLUNetConfig
    from anyv2v_amd.vae import AutoencoderKL, VAEConfig
    from oracle import vae_oracle as vo
    from oracle.unet_oracle import UNetConfig
    gn, ln = {}, {}
    real_gn, real_ln = ops.groupnorm, ops.layernorm

    def rec_gn(x0, gamma, beta, stats, rows_per_group, *, x1=None, groups=32, eps=1e-5, silu=False, out=None, shard=None):
        key = (x0.shape[1], 0 if x1 is None else x1.shape[1], rows_per_group, groups, float(eps), bool(silu))
        gn.setdefault(key, 0)
        gn[key] += 1
        return real_gn(x0, gamma, beta, stats, rows_per_group, x1=x1, groups=groups, eps=eps, silu=silu, out=out, shard=shard)

    def rec_ln(x, gamma, beta, eps=1e-5, out=None):
        key = (x.shape[1], float(eps))
        ln.setdefault(key, 0)
        ln[key] += 1
        return real_ln(x, gamma, beta, eps, out)

    ops.groupnorm, ops.layernorm = rec_gn, rec_ln
    try:
        with torch.no_grad():
            # full-width I2VGen-XL UNet: seeded weights drawn on the GPU with random_state_dict's init rule
            with torch.device("meta"):
                unet = I2VGenXLUNet(I2VGenXLUNetConfig())
            gen = torch.Generator(device=DEV).manual_seed(1234)
            sd = {}
            for k, v in unet.state_dict().items():
                t = torch.randn(tuple(v.shape), generator=gen, device=DEV)
                fan_in = max(1, v[0].numel()) if v.dim() > 1 else 1
                sd[k] = (t * 0.02 if k.endswith(".bias") else (1.0 + 0.05 * t) if v.dim() == 1 else t / math.sqrt(fan_in)).half()
            unet = unet.to_empty(device=DEV)
            unet.load_state_dict(sd, strict=True)
            del sd
            inp = config1_inputs(UNetConfig.i2vgen_xl(), 1, 8, 32)
            unet(inp["sample"].half().to(DEV), 981, **_cond_kw({k: (v.half() if v.is_floating_point() else v) for k, v in inp.items()},
                                                               DEV, torch.float16))
            _sync()
            del unet
            for ncfg, ocfg, xs, zs in [(VAEConfig.mini(), vo.VAEConfig.mini(), (1, 3, 32, 48), (1, 4, 8, 12)),
                                       (VAEConfig(), vo.VAEConfig(), (1, 3, 64, 64), (1, 4, 8, 8))]:
                vae = AutoencoderKL(ncfg)
                vae.load_state_dict(vo.random_state_dict(ocfg, 11))
                vae.to(DEV)
                g = torch.Generator().manual_seed(5)
                vae.encode_moments(torch.randn(*xs, generator=g).clamp(-1, 1).to(DEV))
                vae.decode(torch.randn(*zs, generator=g).to(DEV))
                del vae
            cu = c2spec.fill_weights(c2.VideoLDMUNet3DConditionModel(**c2spec.UNET_CFG)).to(DEV)
            sample, first, ehs = c2spec.unet_inputs()
            cu(sample.to(DEV).half(), c2spec.UNET_T, encoder_hidden_states=ehs.to(DEV).half(), first_frame_latents=first.to(DEV).half(),
               frame_stride=c2spec.UNET_STRIDE)
            del cu
            su = snspec.fill_weights(sn.UNet3DConditionModel(**snspec.UNET_CFG), snspec.WEIGHT_SEED).to(DEV)
            sample, ehs = snspec.unet_inputs()
            su(sample.to(DEV).half(), 981, encoder_hidden_states=ehs.to(DEV).half())
            del su
            _sync()
    finally:
        ops.groupnorm, ops.layernorm = real_gn, real_ln
        torch.cuda.empty_cache()
    _NORM_CALLS = (gn, ln)
    return _NORM_CALLS


def check_norms_at_recorded_shapes():
    """Every distinct GroupNorm / LayerNorm signature the product issues (``recorded_norm_calls``), run at its real rows_per_group
    with two statistics groups, plus the bench's 5-D size (16 frames x 64^2 latents) and the VAE's 512^2 groups, against float64
    two-pass statistics.  Inputs carry a per-channel offset of up to ~2 sigma."""
    gn, ln = recorded_norm_calls()
    out = []
    n_two = sum(1 for k in gn if k[1] > 0)
    # a silent change in the hooks must not be able to empty (or thin) the list
    # (73 / 20 / 8 when this was written; the full-width up-block skip concat 1280 + 640 at 8 x 8 latents must be among them)
    out.append(dict(name=f"recorded {len(gn)} GroupNorm signatures ({n_two} two-source), {len(ln)} LayerNorm signatures",
                    err=0.0, tol=0.0, ok=bool(len(gn) >= 70 and n_two >= 20 and len(ln) >= 8 and (1280, 640, 64, 32, 1e-5, True) in gn)))
    cases = sorted(gn)
    cases += [(320, 0, 16 * 4096, 32, 1e-5, True), (320, 0, 16 * 4096, 32, 1e-5, False), (1280, 0, 16 * 64, 32, 1e-5, True),
              (128, 0, 512 * 512, 32, 1e-6, True), (256, 0, 512 * 512, 32, 1e-6, True)]
    for i, (C0, C1, rpg, G, eps, silu) in enumerate(cases):
        nsg = 2 if rpg * (C0 + C1) <= (1 << 24) else 1
        C = C0 + C1
        g = torch.Generator(device="cpu").manual_seed(100 + i)
        off = (torch.randn(C, generator=g) * 2.0).to(DEV)
        x = (rnd(nsg * rpg, C, seed=200 + i).float() + off).half()
        x0, x1 = (x[:, :C0].contiguous(), x[:, C0:].contiguous()) if C1 else (x, None)
        ga, be = _affine(C, 300 + i)
        out.append(_gn_row(f"groupnorm C{C0}+{C1} rows/group {rpg} x {nsg} G{G} eps {eps:g} silu={silu}", x0, x1, ga, be, rpg, G, eps,
                           silu))
        del x, x0, x1
    for i, (C, eps) in enumerate(sorted(ln)):
        M = 2 * 4096 + 3
        x = (rnd(M, C, seed=400 + i).float() + (torch.randn(M, 1, device=DEV) * 2.0)).half()
        ga, be = _affine(C, 500 + i)
        out.append(_res(f"layernorm recorded C{C} eps {eps:g} M{M}", ops.layernorm(x, ga, be, eps), _ln_ref64(x, ga, be, eps), KTOL))
    return out


def check_groupnorm_ill_conditioned():
    """Groups whose mean is large against their spread (offset / sigma up to 1000), near-constant groups (level 3-40, noise
    0.1-1 % of the level), exactly constant and all-zero groups (-> fp16(beta), up to SiLU), and a two-source call whose X0 and
    X1 carry different offsets inside the group that straddles the boundary (1280 + 640: 60 channels per group).  4-D (4096
    rows per group) and 5-D (16 x 1024 rows per group) shapes, with and without SiLU, eps 1e-5 and 1e-6."""
    out = []
    shapes = [("4-D", 2, 4096, 320), ("5-D", 1, 16 * 1024, 320)]
    for tag, nsg, rpg, C in shapes:
        ga, be = _affine(C, 11)
        for offset in (0, 10, 100, 1000):
            x = _offset_data(nsg, rpg, C, 32, offset, seed=offset + rpg)
            for silu in (False, True):
                for eps in (1e-5, 1e-6):
                    out.append(_gn_row(f"groupnorm {tag} rows/group {rpg} offset {offset} sigma silu={silu} eps {eps:g}", x, None,
                                       ga, be, rpg, 32, eps, silu))
        g = torch.Generator(device="cpu").manual_seed(rpg)
        for level in (3.0, 40.0):
            for frac in (1e-3, 1e-2):
                lv = (level * (torch.rand(nsg, 1, 32, 1, generator=g) + 0.5)).to(DEV)
                x = (lv * (1.0 + frac * torch.randn(nsg, rpg, 32, C // 32, generator=g).to(DEV))).view(nsg * rpg, C).half()
                for silu in (False, True):
                    for eps in (1e-5, 1e-6):
                        out.append(_gn_row(f"groupnorm {tag} near-constant level {level:g} noise {frac:g} silu={silu} eps {eps:g}", x,
                                           None, ga, be, rpg, 32, eps, silu))
        # group 0 exactly constant, group 1 all zero, the rest random with an offset
        x = _offset_data(nsg, rpg, C, 32, 5, seed=7).view(nsg, rpg, C)
        cpg = C // 32
        x[:, :, :cpg] = 7.0
        x[:, :, cpg:2 * cpg] = 0.0
        x = x.view(nsg * rpg, C)
        for silu in (False, True):
            for eps in (1e-5, 1e-6):
                y = _gn_run(x, None, ga, be, rpg, 32, eps, silu).view(nsg, rpg, C)[:, :, :2 * cpg].float()
                want = be[:2 * cpg].double()
                want = (want * torch.sigmoid(want) if silu else want).half().float().expand_as(y)
                err = float((y - want).abs().max())
                tol = 0.0 if not silu else 1e-3   # SiLU on the raw v_exp / v_rcp: within 1 fp16 ulp of |beta| <= 1
                out.append(dict(name=f"groupnorm {tag} constant and all-zero groups -> fp16(beta) silu={silu} eps {eps:g}", err=err,
                                tol=tol, ok=bool(torch.isfinite(y).all() and err <= tol)))
    # two sources, different offsets in X0 (+100 sigma) and X1 (-300 sigma)
    B, rpg, c0, c1 = 2, 4096, 1280, 640
    x0 = (rnd(B * rpg, c0, seed=21).float() + 100.0).half()
    x1 = (rnd(B * rpg, c1, seed=22).float() - 300.0).half()
    ga, be = _affine(c0 + c1, 23)
    for silu in (False, True):
        out.append(_gn_row(f"groupnorm two-source 1280 + 640, offsets +100 / -300 sigma, silu={silu}", x0, x1, ga, be, rpg, 32, 1e-5,
                           silu))
    return out


def _guarded(M, C, pad=64, bits=0x7E5A):
    """A [M, C] fp16 output carved as a row slice of a larger buffer filled with a NaN bit pattern no kernel computes."""
    buf = torch.full((M + 2 * pad, C), bits, dtype=torch.int16, device=DEV)
    return buf, buf.view(torch.float16)[pad:pad + M], (pad, bits)


def _guard_intact(buf, M, guard):
    pad, bits = guard
    return bool((buf[:pad] == bits).all() and (buf[pad + M:] == bits).all())


POISON16 = 0x7E5A       # fp16 NaN, the pattern of ``_guarded``
POISON32 = 0x7FC5A5A5   # fp32 NaN


def _framed(M, C, dtype=torch.float16, rows=64, cols=8, bits=None, device=None, aligned=True):
    """``(buf, view, frame)``: ``view`` is an [M, C] window of one larger tensor ``buf`` (integer dtype of the same width) whose
    every element outside the window holds the NaN bit pattern ``bits``: ``rows`` guard rows above and below, ``cols`` guard
    columns on the left and at least as many on the right (the leading dimension is rounded up to a multiple of 8 elements).
    With ``aligned`` the row pitch and the left guard are multiples of 16 bytes, so ``view`` starts 16-byte aligned and keeps
    ``ld % 8 == 0``: a launch on it gets the plan the launch on a fresh contiguous tensor gets."""
    item = torch.empty(0, dtype=dtype).element_size()
    assert item in (2, 4), dtype
    idt = torch.int16 if item == 2 else torch.int32
    if bits is None:
        bits = POISON16 if item == 2 else POISON32
    ld = (2 * cols + C + 7) // 8 * 8
    if aligned:
        assert (cols * item) % 16 == 0 and (rows * ld * item) % 16 == 0
    buf = torch.full((M + 2 * rows, ld), bits, dtype=idt, device=DEV if device is None else device)
    return buf, buf.view(dtype)[rows:rows + M, cols:cols + C], (rows, cols, M, C, bits)


def _frame_intact(buf, frame):
    """Exact bit compare of everything outside the window (the four bands: above, below, left, right)."""
    rows, cols, M, C, bits = frame
    mid = buf[rows:rows + M]
    return bool((buf[:rows] == bits).all() and (buf[rows + M:] == bits).all() and (mid[:, :cols] == bits).all()
                and (mid[:, cols + C:] == bits).all())


def _framed_like(t, flat=False, rows=64, cols=8, device=None, aligned=True):
    """``t`` copied into a frame: a 2-D matrix into an [M, C] window (strided, for operands addressed with a leading dimension); with
    ``flat`` or any other rank the elements stay contiguous, with ``rows`` x row pitch poison elements before and after (weights, 1-D
    operands such as bias / gamma / ``ln_c1``, NCFHW latents)."""
    device = t.device if device is None else device
    if t.dim() == 2 and not flat:
        buf, view, frame = _framed(t.shape[0], t.shape[1], t.dtype, rows, cols, device=device, aligned=aligned)
        view.copy_(t)
        return buf, view, frame
    buf, view, frame = _framed(1, t.numel(), t.dtype, rows=1, cols=64, device=device)
    view.copy_(t.reshape(1, -1))
    return buf, view[0].view(t.shape), frame


def _ld8(t):
    """``t`` as a window of a zero matrix whose leading dimension is a multiple of 8 (what ``_framed`` gives the framed twin)."""
    if t is None or t.dim() != 2 or t.shape[1] % 8 == 0:
        return t
    wide = torch.zeros(t.shape[0], (t.shape[1] + 7) // 8 * 8, dtype=t.dtype, device=t.device)
    wide[:, :t.shape[1]] = t
    return wide[:, :t.shape[1]]


class _PlainOperands:
    """Operands of the plain launch of an edge row: fresh tensors (ragged widths padded to ``ld % 8 == 0``)."""
    framed = False

    def __init__(self, device=None):
        self.device = DEV if device is None else device      # "meta": the layout alone (tests/test_attention_plan_host.py)

    def inp(self, t, flat=False):
        return t if (t is None or flat) else _ld8(t)

    def out(self, M, C, dtype=torch.float16, init=None, cols=8):
        ld = (C + 7) // 8 * 8 + (0 if cols % 8 == 0 else 16)
        off = 0 if cols % 8 == 0 else cols
        y = torch.zeros(M, ld, dtype=dtype, device=self.device)[:, off:off + C]
        if init is not None:
            y.copy_(init)
        return y

    def out_flat(self, shape, dtype=torch.float16):
        return torch.zeros(shape, dtype=dtype, device=DEV)

    def inout(self, t):
        return t.clone()

    def intact(self):
        return True


class _FramedOperands:
    """Operands of the framed launch: every input and output inside a poisoned frame; ``intact()`` checks the frames of the outputs."""
    framed = True

    def __init__(self, device=None):
        self.outs = []
        self.device = DEV if device is None else device

    def inp(self, t, flat=False):
        return None if t is None else _framed_like(t, flat)[1]

    def out(self, M, C, dtype=torch.float16, init=None, cols=8):
        buf, view, frame = _framed(M, C, dtype, cols=cols, aligned=cols % 8 == 0, device=self.device)
        self.outs.append((buf, frame))
        if init is not None:
            view.copy_(init)
        return view

    def out_flat(self, shape, dtype=torch.float16):
        n = 1
        for s in shape:
            n *= s
        buf, view, frame = _framed(1, n, dtype, rows=1, cols=64)
        self.outs.append((buf, frame))
        return view[0].view(shape)

    def inout(self, t):
        buf, view, frame = _framed_like(t, flat=not (t.dim() == 2))
        self.outs.append((buf, frame))
        return view

    def intact(self):
        return all(_frame_intact(buf, frame) for buf, frame in self.outs)


def _edge_rows(name, run, ref, tol=KTOL):
    """The three rows of one edge case.  ``run(f)`` launches with the operands ``f`` hands out (``f.inp`` / ``f.out`` / ...) and returns
    the result; it runs once on plain tensors and once with every operand framed.  Rows: framed result vs ``ref`` (a tensor or a
    function of the result) at ``tol``; framed == plain, bit for bit (the plan depends on shapes, flags and alignment only: a difference
    means poison reached a stored value); the frames of the framed outputs intact."""
    yp = run(_PlainOperands())
    fr = _FramedOperands()
    yf = run(fr)
    torch.cuda.synchronize()
    want = ref(yf) if callable(ref) else ref
    same = bool(torch.equal(yf, yp))
    intact = fr.intact()
    return [_res(name + ": framed vs reference", yf, want, tol),
            dict(name=name + ": framed == plain, bit for bit", err=0.0 if same else float((yf.float() - yp.float()).abs().nan_to_num(nan=float("inf")).max()),
                 tol=0.0, ok=same),
            dict(name=name + ": frames of the outputs intact", err=0.0 if intact else 1.0, tol=0.0, ok=intact)]


def _skip_row(name, why):
    return dict(name=f"{name}: SKIPPED ({why})", err=0.0, l2=0.0, tol=0.0, ok=True, skipped=True)


# (C0, C1, rows_per_group, nsg, G, silu); tests/test_norm_plan_host.py pins the plan of each on the CPU
GN_PLAN_EDGE_CASES = [
    (320, 0, 4099, 2, 32, True),        # 86 chunks of 48 rows, rpb = 6: neither divides 4099
    (640, 0, 1021, 3, 32, False),       # a prime row count, rpb = 3
    (320, 0, 65536 + 37, 1, 32, True),  # the 256-chunk cap, ragged last chunk
    (1280, 640, 12289, 2, 32, True),    # two sources, chunked by the cap (251 chunks of 49 rows)
    (2560, 0, 2053, 2, 32, False),      # V = 320: one row per block
    (2560, 0, 1024, 2, 32, True),
    (8, 0, 3001, 2, 4, True),           # C = 8: one vector per row, 256 rows per block
    (8, 0, 70001, 1, 8, False),
]
GN_PLAN_HINT_CASE = (8, 16 * 1024, 320)   # (nsg, rows_per_group, C): 191 chunks; hinted as 12 groups: 128 chunks


def check_groupnorm_plan_edges():
    """The launch plan's edges: rows_per_group that is not a multiple of the rows per block or of the chunk size, the 256-chunk
    cap, the same tensor under ``batch_hint(3, 2)`` (another chunk count: within KTOL, bit-reproducible call to call, and bit-equal to
    its rows of the 12-group launch it stands for),
    C = 2560 (one row per block), C = 8; every call writes nothing outside its output rows nor past the stats scratch."""
    out = []
    TAIL = 4096
    cases = GN_PLAN_EDGE_CASES
    for C0, C1, rpg, nsg, G, silu in cases:
        C, M = C0 + C1, nsg * rpg
        x = _offset_data(nsg, rpg, C, G, 3, seed=rpg)
        x0, x1 = (x[:, :C0].contiguous(), x[:, C0:].contiguous()) if C1 else (x, None)
        ga, be = _affine(C, 31)
        buf, y, guard = _guarded(M, C)
        need = ops.gn_scratch_floats(M, rpg, G)
        stats = torch.full((need + TAIL,), -1234.5, dtype=torch.float32, device=DEV)
        ops.groupnorm(x0, ga, be, stats, rpg, x1=x1, groups=G, eps=1e-5, silu=silu, out=y)
        ref = _gn_ref64(x0, x1, ga, be, rpg, G, 1e-5, silu)
        name = f"groupnorm edge C{C0}+{C1} rows/group {rpg} x {nsg} G{G} silu={silu}"
        out.append(_res(name, y, ref, KTOL))
        out.append(dict(name=name + ": output guard rows and stats tail untouched", err=0.0, tol=0.0,
                        ok=_guard_intact(buf, M, guard) and bool((stats[need:] == -1234.5).all())))
    # batch hint: 8 groups of 16 x 1024 rows -> 191 chunks (of 86 rows: a target of 192); hinted as 12 groups -> 128 chunks
    nsg, rpg, C = GN_PLAN_HINT_CASE
    x = _offset_data(nsg, rpg, C, 32, 50, seed=99)
    ga, be = _affine(C, 41)
    ref = _gn_ref64(x, None, ga, be, rpg, 32, 1e-5, True)
    plain = _gn_run(x, None, ga, be, rpg, 32, 1e-5, True)
    with ops.batch_hint(3, 2):
        h1 = _gn_run(x, None, ga, be, rpg, 32, 1e-5, True)
        h2 = _gn_run(x, None, ga, be, rpg, 32, 1e-5, True)
    out.append(_res("groupnorm 8 x 16384 rows, offset 50 sigma: plain", plain, ref, KTOL))
    out.append(_res("groupnorm 8 x 16384 rows, offset 50 sigma: under batch_hint(3, 2)", h1, ref, KTOL))
    out.append(dict(name="groupnorm under batch_hint(3, 2): bit-reproducible call to call", err=0.0, tol=0.0, ok=bool(torch.equal(h1, h2))))
    # ... and what the hint is for: the 8 groups are the last 8 of a 12-group launch, and their rows of that launch have the same bits
    x12 = torch.cat([_offset_data(nsg // 2, rpg, C, 32, 50, seed=98), x], 0)
    full = _gn_run(x12, None, ga, be, rpg, 32, 1e-5, True)
    out.append(_res("groupnorm 12 x 16384 rows, offset 50 sigma: plain", full, _gn_ref64(x12, None, ga, be, rpg, 32, 1e-5, True), KTOL))
    same = bool(torch.equal(h1, full[(nsg // 2) * rpg:]))
    out.append(dict(name="groupnorm under batch_hint(3, 2) == rows [4 rpg, 12 rpg) of the 12-group launch, bit for bit", err=0.0 if same else 1.0, tol=0.0, ok=same))
    return out


def check_groupnorm_from_records_ragged():
    """``groupnorm_from_stats`` on hand-built records at the edges of the run folding: 256 records per statistics group (no fold), 257
    (runs of 2, the last run one record), 513 (171 full runs of 3), 514 (runs of 3, the last run one record).  Records as a GEMM
    writes them: per 16 rows and channel group (K, s, q) about K = the block's first row, the group's first channel; computed in
    float64, rounded to fp32.  Group offsets of 3 sigma make the pivots differ.  Nothing is written past ``gn_stats_floats``."""
    out = []
    C, G, nsg, TAIL = 64, 32, 2, 4096
    cpg = C // G
    ga, be = _affine(C, 71)
    for nrec in (256, 257, 513, 514):
        rpg = 16 * nrec
        M = nsg * rpg
        x = _offset_data(nsg, rpg, C, G, 3, seed=nrec)
        xb = x.double().view(nsg, nrec, 16, G, cpg)
        K = xb[:, :, 0, :, 0]
        d = xb - K[:, :, None, :, None]
        records = torch.stack([K, d.sum((2, 4)), d.square().sum((2, 4))], -1).float()    # [nsg][nrec][G][3]
        need = ops.gn_stats_floats(M, rpg, G)
        stats = torch.full((need + TAIL,), -1234.5, dtype=torch.float32, device=DEV)
        stats[:records.numel()] = records.reshape(-1)
        buf, y, guard = _guarded(M, C)
        ops.groupnorm_from_stats(x, ga, be, stats, rpg, groups=G, eps=1e-5, silu=True, out=y)
        name = f"groupnorm from {nrec} hand-built records x {nsg} groups"
        out.append(_res(name, y, _gn_ref64(x, None, ga, be, rpg, G, 1e-5, True), KTOL))
        out.append(dict(name=name + ": output guard rows and stats tail untouched", err=0.0, tol=0.0,
                        ok=_guard_intact(buf, M, guard) and bool((stats[need:] == -1234.5).all())
                        and bool(torch.equal(stats[:records.numel()], records.reshape(-1)))))
    return out


def gn_sharded_emulated(xs0, xs1, ga, be, rpg_local, *, groups=32, eps=1e-5, silu=False):
    """``len(xs0)`` ranks of a sharded GroupNorm run in one process through ``ops.groupnorm(shard=...)``.  The all-reduce callback
    is emulated in passes: in pass p every rank's callback answers rounds < p with the sums agreed so far, records its own
    buffer of round p, and leaves later rounds alone; the recorded buffers are added in rank order and the next pass starts.  The
    pass in which no rank reaches a new round returns the ranks' outputs.  (Works for any number of all-reduce rounds.)"""
    S = len(xs0)
    stats = [torch.zeros(ops.gn_scratch_floats(x.shape[0], rpg_local, groups), dtype=torch.float32, device=DEV) for x in xs0]
    agreed = []
    while True:
        contrib = [None] * S
        ys = []
        for r in range(S):
            k = [0]

            def cb(t, r=r, k=k):
                if k[0] < len(agreed):
                    t.copy_(agreed[k[0]])
                elif k[0] == len(agreed):
                    contrib[r] = t.clone()
                k[0] += 1
            ys.append(ops.groupnorm(xs0[r], ga, be, stats[r], rpg_local, x1=None if xs1 is None else xs1[r], groups=groups, eps=eps,
                                    silu=silu, shard=(S, cb)))
        if contrib[0] is None:
            return ys
        tot = contrib[0].clone()
        for c in contrib[1:]:
            tot += c
        agreed.append(tot)


def check_groupnorm_sharded_offsets():
    """Sharded GroupNorm (frame-parallel clips) on data with large group offsets: a clip split into 2 and 4 pixel ranges over
    emulated ranks equals the unsharded call and the float64 reference; shards = 1 through the same path is the one call, bit for
    bit."""
    out = []
    B, Fr, hw, c0, c1 = 1, 16, 1024, 320, 320
    rpg = Fr * hw
    x = _offset_data(B, rpg, c0 + c1, 32, 200, seed=5)
    x0, x1 = x[:, :c0].contiguous(), x[:, c0:].contiguous()
    ga, be = _affine(c0 + c1, 51)
    full = _gn_run(x0, x1, ga, be, rpg, 32, 1e-5, True)
    ref = _gn_ref64(x0, x1, ga, be, rpg, 32, 1e-5, True)
    out.append(_res("groupnorm 5-D two-source offset 200 sigma, unsharded", full, ref, KTOL))
    one = gn_sharded_emulated([x0], [x1], ga, be, rpg, silu=True)[0]
    out.append(_res("groupnorm sharded path, shards = 1 == one call (bit-equal)", one, full.float(), 0.0 if DEV != "cpu" else 2e-3))
    for S in (2, 4):
        def split(t):
            v = t.view(B, Fr, hw, t.shape[1])
            return [v[:, :, i * hw // S:(i + 1) * hw // S].reshape(-1, t.shape[1]).contiguous() for i in range(S)]
        ys = gn_sharded_emulated(split(x0), split(x1), ga, be, rpg // S, silu=True)
        got = torch.cat([y.view(B, Fr, hw // S, c0 + c1) for y in ys], 2).reshape(B * rpg, c0 + c1)
        out.append(_res(f"groupnorm sharded over {S} pixel ranges, offset 200 sigma, vs unsharded", got, full.float(), 2e-3))
        out.append(_res(f"groupnorm sharded over {S} pixel ranges, offset 200 sigma, vs float64", got, ref, KTOL))
    if DEV == "cpu":   # (the op emulation has no counterpart of the raw C entry points below)
        return out
    # the pre-104 one-all-reduce pair (pivot 0, no longer used by ops) on moderately offset data: two identical shards, the
    # 'all-reduce' doubling the partial sums
    from anyv2v_amd import _lib
    lib = _lib.load()
    xm = (rnd(2 * 4096, 320, seed=61).float() + 0.5).half()
    gam, bet = _affine(320, 62)
    st = torch.zeros(ops.gn_scratch_floats(xm.shape[0], 4096), dtype=torch.float32, device=DEV)
    ym = torch.empty_like(xm)
    n = int(lib.anyv2v_groupnorm_partial_floats(xm.shape[0], 4096, 32, 320))
    _lib.check(lib.anyv2v_groupnorm_partial_f16(xm.data_ptr(), None, 320, 0, st.data_ptr(), xm.shape[0], 4096, 32, ops._stream()))
    st[:n].mul_(2)
    _lib.check(lib.anyv2v_groupnorm_apply_f16(xm.data_ptr(), None, 320, 0, ym.data_ptr(), gam.data_ptr(), bet.data_ptr(), st.data_ptr(),
                                              xm.shape[0], 4096, 32, 1e-5, 1, 2, ops._stream()))
    out.append(_res("groupnorm pre-104 sharded pair (one all-reduce), 2 identical shards", ym,
                    _gn_ref64(xm, None, gam, bet, 4096, 32, 1e-5, True), KTOL))
    return out


def check_layernorm_large():
    """LayerNorm beyond the 8192-block grid cap (several grid-stride iterations per wave), at C = 1024 / 1280 / 2048 (largest
    fast-kernel row) / 2056 and 12 (the one-thread-per-row kernel), with row offsets of 100 and 1000 sigma; outputs carved from a
    guarded buffer (nothing written outside the rows)."""
    out = []
    cases = [(3 * 16 * 4096, 320, 0.0), (100001, 320, 0.0), (100001, 320, 100.0), (100001, 320, 1000.0), (66001, 1024, 0.0),
             (4099, 1280, 1000.0), (20001, 2048, 0.0), (20001, 2048, 100.0), (20001, 2056, 0.0), (20001, 2056, 1000.0),
             (70001, 12, 0.0), (70001, 12, 100.0)]
    for i, (M, C, offset) in enumerate(cases):
        g = torch.Generator(device="cpu").manual_seed(i)
        sign = (torch.randint(0, 2, (M, 1), generator=g) * 2 - 1).float().to(DEV)
        x = (rnd(M, C, seed=600 + i).float() + sign * offset).half()
        ga, be = _affine(C, 700 + i)
        buf, y, guard = _guarded(M, C)
        ops.layernorm(x, ga, be, 1e-5, out=y)
        name = f"layernorm M{M} C{C} offset {offset:g} sigma"
        out.append(_res(name, y, _ln_ref64(x, ga, be, 1e-5), KTOL))
        out.append(dict(name=name + ": output guard rows untouched", err=0.0, tol=0.0, ok=_guard_intact(buf, M, guard)))
    return out


# ------------------------------------------------------------------------------------------------ attention
def _sdpa(q, k, v):  # [b, h, s, d] fp32
    return F.scaled_dot_product_attention(q.float(), k.float(), v.float())


def check_attention_forced_rescale():
    """The flash kernel exponentiates every 16-key step against the OLD running maximum and uses the partial row sum as the
    range check; the textbook path (true maximum, rescale of O and l, re-exponentiation) only runs when that check trips and
    on the very first step.  Bounded random data never takes the branch after the first step, so it is forced here (MI355X
    guide rule 26): spiked keys at chosen positions (start / middle of a tile, last key, ragged tail), a first step whose
    scores sit far BELOW the rest (maximum has to climb), far ABOVE the rest (everything after underflows), and scores that
    overflow fp32 exp2 against the old maximum (inf in the check).  Reference: fp32 SDPA on the same fp16 inputs."""
    out = []
    for name, S, Sk, build in forced_rescale_specs():
        b, h = 2, 2
        C = 64 * h
        q2 = rnd(b * S, C, scale=1.0, seed=1234)
        kv = rnd(b * Sk, 2 * C, scale=1.0, seed=4321)
        build(q2.view(b, S, h, 64), kv[:, :C].view(b, Sk, h, 64))
        q = q2.view(b, S, h, 64).transpose(1, 2)
        k = kv[:, :C].reshape(b, Sk, h, 64).transpose(1, 2)
        v = kv[:, C:].reshape(b, Sk, h, 64).transpose(1, 2)
        ref = _sdpa(q, k, v).transpose(1, 2).reshape(b * S, C)
        o = torch.zeros(b * S, C, dtype=torch.float16, device=DEV)
        ops.attention(q2, kv[:, :C], kv[:, C:], o, batch=b, heads=h, Sq=S, Sk=Sk, inner=1, q_strides=(S, 0, 1),
                      kv_strides=(Sk, 0, 1))
        out.append(_res(f"attn[flash] forced rescale: {name}", o, ref, KTOL))
        if S == Sk:  # the shared-softmax kernel on the same Q / K (three V streams)
            b3 = 3
            qkv3 = rnd(b3 * S, 3 * C, scale=1.0, seed=99)
            qkv3[:S, :C] = q2[:S]
            qkv3[:S, C:2 * C] = kv[:S, :C]
            o3 = torch.zeros(b3 * S, C, dtype=torch.float16, device=DEV)
            ops.attention(qkv3[:, :C], qkv3[:, C:2 * C], qkv3[:, 2 * C:], o3, batch=b3, heads=h, Sq=S, Sk=S, inner=1,
                          q_strides=(S, 0, 1), kv_strides=(S, 0, 1), qk_mod=1)
            q3, k3, v3 = (qkv3[:, i * C:(i + 1) * C].view(b3, S, h, 64).transpose(1, 2).clone() for i in range(3))
            q3[1], k3[1], q3[2], k3[2] = q3[0], k3[0], q3[0], k3[0]
            out.append(_res(f"attn[shared softmax] forced rescale: {name}", o3,
                            _sdpa(q3, k3, v3).transpose(1, 2).reshape(b3 * S, C), KTOL))
    return out


def forced_rescale_specs():
    """(name, Sq, Sk, what to do to q / k) of ``check_attention_forced_rescale``: b2 h2 on the 4-wave flash kernel, and where Sq == Sk also
    b3 h2 qk_mod 1 on the shared-softmax 4-wave kernel."""
    return (
        ("spike at key 70 (2nd tile, 1st step)", 256, 256, lambda q, k: _spike(q, k, [70], 6.0)),
        ("spikes at keys 5, 200, 255 (every path of a tile)", 256, 256, lambda q, k: _spike(q, k, [5, 200, 255], 5.0)),
        ("spike in the ragged tail (key 144 of 145)", 128, 145, lambda q, k: _spike(q, k, [144], 6.0)),
        ("first 16 keys far below the rest", 128, 512, lambda q, k: _shift_first(q, k, -4.0)),
        ("first 16 keys far above the rest", 128, 512, lambda q, k: _shift_first(q, k, 4.0)),
        ("exp2 overflow against the old maximum (|s c| ~ 400)", 128, 320, lambda q, k: _spike(q, k, [100, 300], 40.0)),
    )


def _spike(q, k, keys, gain):
    """k[:, key] := gain * (a query row's direction): that row's score at `key` dwarfs the others (in place, views of fp16)."""
    for n, key in enumerate(keys):
        rows = q[:, (7 + 13 * n) % q.shape[1]]            # [b, h, 64]: a different query row per spike
        k[:, key] = (gain * rows.float()).half()


def _shift_first(q, k, gain):
    """The first 16 keys get scores far below (gain < 0) / above (gain > 0) all later ones for EVERY query: both q and the
    first keys receive a large common component."""
    q[..., 0] = 6.0
    k[:, :16, :, 0] = gain * 6.0


# The rows of ``check_attention`` that name a kernel: "PnP shared-softmax b.. h.. S.." (and its "aliasing form", flag bit3), the "8-wave
# blocks" rows (and the 4-wave twin, flag bit2) and the "attn[flash] b.. h.. S.. Sk.." KV-loop sweep.  (b, h, S) / (b, h, S, Sk, kv_div, qk_mod)
ATTN_PNP_SHARED_SHAPES = [(3, 1, 333), (6, 5, 1024), (48, 1, 130)]
ATTN_8WAVE_SHAPES = {"shared-softmax": (48, 5, 4096), "shared-softmax, ragged": (96, 4, 2100), "plain": (13, 5, 4096)}
ATTN_FLASH_KV_LOOP_SHAPES = [(2, 1, 20, 3, 1, 0), (2, 2, 130, 17, 1, 0), (1, 1, 33, 63, 1, 0),  # tiny ragged KV: whole steps masked
                             (2, 1, 128, 64, 1, 0), (2, 2, 128, 128, 1, 0), (4, 1, 256, 145, 2, 0),
                             (1, 2, 128, 200, 1, 0), (2, 1, 128, 320, 1, 0), (1, 1, 256, 384, 1, 0),
                             (4, 2, 128, 448, 1, 2), (1, 5, 4096, 4096, 1, 0)]


def check_attention(naive_too=True):
    out = []
    for naive in ((False, True) if naive_too else (False,)):
        tag = "naive" if naive else "flash"
        # spatial self-attention out of a fused QKV buffer
        for (b, h, S) in [(3, 2, 200), (2, 5, 1024), (6, 1, 64), (1, 2, 4096)]:
            C = 64 * h
            qkv = rnd(b * S, 3 * C, scale=1.0)
            o = torch.zeros(b * S, C, dtype=torch.float16, device=DEV)
            ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, batch=b, heads=h, Sq=S, Sk=S, inner=1,
                          q_strides=(S, 0, 1), kv_strides=(S, 0, 1), naive=naive)
            q, k, v = (qkv[:, i * C:(i + 1) * C].view(b, S, h, 64).transpose(1, 2) for i in range(3))
            ref = _sdpa(q, k, v).transpose(1, 2).reshape(b * S, C)
            out.append(_res(f"attn[{tag}] spatial b{b} h{h} S{S}", o, ref, KTOL))
        # PnP aliasing: Q,K of branches 1,2 come from branch 0
        b, h, S = 6, 2, 192
        C = 64 * h
        qkv = rnd(b * S, 3 * C)
        o = torch.zeros(b * S, C, dtype=torch.float16, device=DEV)
        ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, batch=b, heads=h, Sq=S, Sk=S, inner=1,
                      q_strides=(S, 0, 1), kv_strides=(S, 0, 1), qk_mod=b // 3, naive=naive)
        q, k, v = (qkv[:, i * C:(i + 1) * C].view(b, S, h, 64).transpose(1, 2).clone() for i in range(3))
        c3 = b // 3
        q[c3:2 * c3], k[c3:2 * c3], q[2 * c3:], k[2 * c3:] = q[:c3], k[:c3], q[:c3], k[:c3]  # pnp_utils.py:192-196
        out.append(_res(f"attn[{tag}] spatial PnP q/k injection", o, _sdpa(q, k, v).transpose(1, 2).reshape(b * S, C), KTOL))
        # shared-softmax PnP kernel (one S/P per source element, three V streams): ragged and multi-tile shapes, and
        # agreement with the aliasing form of the same launch (flag bit3), which runs the plain kernel per branch
        for (b, h, S) in ATTN_PNP_SHARED_SHAPES:
            C = 64 * h
            qkv = rnd(b * S, 3 * C, scale=1.0)
            o = torch.zeros(b * S, C, dtype=torch.float16, device=DEV)
            kw = dict(batch=b, heads=h, Sq=S, Sk=S, inner=1, q_strides=(S, 0, 1), kv_strides=(S, 0, 1), qk_mod=b // 3)
            ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, naive=naive, **kw)
            q, k, v = (qkv[:, i * C:(i + 1) * C].view(b, S, h, 64).transpose(1, 2).clone() for i in range(3))
            c3 = b // 3
            q[c3:2 * c3], k[c3:2 * c3], q[2 * c3:], k[2 * c3:] = q[:c3], k[:c3], q[:c3], k[:c3]
            out.append(_res(f"attn[{tag}] PnP shared-softmax b{b} h{h} S{S}", o,
                            _sdpa(q, k, v).transpose(1, 2).reshape(b * S, C), KTOL))
            if not naive:
                o2 = torch.zeros_like(o)
                saved, ops.ATTN_FLAGS = ops.ATTN_FLAGS, ops.ATTN_FLAGS | 8
                try:
                    ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o2, **kw)
                finally:
                    ops.ATTN_FLAGS = saved
                out.append(_res(f"attn PnP shared-softmax == aliasing form b{b} h{h} S{S}", o, o2.float(), 1e-6))
        if not naive:
            # the 64x64-level launch itself (48 x 5 x 4096: the 8-wave / 3-stage form of the shared-softmax kernel): against the
            # aliasing form (plain kernel per branch) everywhere, against fp32 SDPA on one (source element, head)
            b, h, S = ATTN_8WAVE_SHAPES["shared-softmax"]
            C = 64 * h
            qkv = rnd(b * S, 3 * C, scale=1.0, seed=77)
            o = torch.zeros(b * S, C, dtype=torch.float16, device=DEV)
            kw = dict(batch=b, heads=h, Sq=S, Sk=S, inner=1, q_strides=(S, 0, 1), kv_strides=(S, 0, 1), qk_mod=b // 3)
            ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, **kw)
            o2 = torch.zeros_like(o)
            saved, ops.ATTN_FLAGS = ops.ATTN_FLAGS, ops.ATTN_FLAGS | 8
            try:
                ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o2, **kw)
            finally:
                ops.ATTN_FLAGS = saved
            out.append(_res(f"attn PnP shared-softmax == aliasing form b{b} h{h} S{S} (8-wave blocks)", o, o2.float(), 1e-6))
            # ... and with a ragged last block / last tile on both 8-wave kernels (2100 = 8 x 256 + 52 queries, 32 x 64 + 52 keys)
            br, hr, Sr = ATTN_8WAVE_SHAPES["shared-softmax, ragged"]
            Cr = 64 * hr
            qkvr = rnd(br * Sr, 3 * Cr, scale=1.0, seed=78)
            kwr = dict(batch=br, heads=hr, Sq=Sr, Sk=Sr, inner=1, q_strides=(Sr, 0, 1), kv_strides=(Sr, 0, 1), qk_mod=br // 3)
            o_r = torch.zeros(br * Sr, Cr, dtype=torch.float16, device=DEV)
            ops.attention(qkvr[:, :Cr], qkvr[:, Cr:2 * Cr], qkvr[:, 2 * Cr:], o_r, **kwr)
            o_r2 = torch.zeros_like(o_r)
            saved, ops.ATTN_FLAGS = ops.ATTN_FLAGS, ops.ATTN_FLAGS | 8
            try:
                ops.attention(qkvr[:, :Cr], qkvr[:, Cr:2 * Cr], qkvr[:, 2 * Cr:], o_r2, **kwr)
            finally:
                ops.ATTN_FLAGS = saved
            out.append(_res(f"attn PnP shared-softmax == aliasing form b{br} h{hr} S{Sr} (8-wave blocks, ragged)", o_r, o_r2.float(), 1e-6))
            xr = qkvr.view(br, Sr, 3, hr, 64)
            out.append(_res(f"attn PnP shared-softmax b{br} h{hr} S{Sr}, element 7 head 1 branch 2 vs fp32 SDPA",
                            o_r.view(br, Sr, hr, 64)[7 + 2 * (br // 3), :, 1],
                            _sdpa(xr[7, :, 0, 1][None, None], xr[7, :, 1, 1][None, None], xr[7 + 2 * (br // 3), :, 2, 1][None, None])[0, 0], KTOL))
            del qkvr, o_r, o_r2
            i0, hh = 5, 3
            x = qkv.view(b, S, 3, h, 64)
            q1, k1 = x[i0, :, 0, hh][None, None], x[i0, :, 1, hh][None, None]
            for br in range(3):
                v1 = x[i0 + br * (b // 3), :, 2, hh][None, None]
                got = o.view(b, S, h, 64)[i0 + br * (b // 3), :, hh]
                out.append(_res(f"attn PnP shared-softmax b{b} h{h} S{S}, element {i0} head {hh} branch {br} vs fp32 SDPA", got, _sdpa(q1, k1, v1)[0, 0], KTOL))
        # cross-attention: Sk=145, K/V shared by the F frames of a clip
        B_, Fr, S, h, Sk = 2, 3, 100, 2, 145
        C = 64 * h
        q2 = rnd(B_ * Fr * S, C)
        kv = rnd(B_ * Sk, 2 * C + 64)  # wider buffer: K at cols [0,C), V at [C,2C)
        o = torch.zeros(B_ * Fr * S, C, dtype=torch.float16, device=DEV)
        ops.attention(q2, kv[:, :C], kv[:, C:2 * C], o, batch=B_ * Fr, heads=h, Sq=S, Sk=Sk, inner=1,
                      q_strides=(S, 0, 1), kv_strides=(Sk, 0, 1), kv_div=Fr, naive=naive)
        q = q2.view(B_ * Fr, S, h, 64).transpose(1, 2)
        k = kv[:, :C].reshape(B_, Sk, h, 64).transpose(1, 2).repeat_interleave(Fr, 0)
        v = kv[:, C:2 * C].reshape(B_, Sk, h, 64).transpose(1, 2).repeat_interleave(Fr, 0)
        out.append(_res(f"attn[{tag}] cross Sk=145 kv_div", o, _sdpa(q, k, v).transpose(1, 2).reshape(-1, C), KTOL))
        # temporal: sequences stride by HW rows inside the [(b f) hw, C] matrix; with and without PnP
        for Fr in (16, 8, 40):
            for inj in (False, True):
                B_, HW, h = 3, 20, 2
                C = 64 * h
                qkv = rnd(B_ * Fr * HW, 3 * C)
                o = torch.zeros(B_ * Fr * HW, C, dtype=torch.float16, device=DEV)
                st = (Fr * HW, 1, HW)
                ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, batch=B_ * HW, heads=h, Sq=Fr, Sk=Fr,
                              inner=HW, q_strides=st, kv_strides=st, qk_mod=HW if inj else 0, naive=naive)
                # reference layout of pnp_utils.py: [(B HW), F, C]
                def seq(x):
                    return x.reshape(B_, Fr, HW, h, 64).permute(0, 2, 3, 1, 4).reshape(B_ * HW, h, Fr, 64).clone()
                q, k, v = (seq(qkv[:, i * C:(i + 1) * C]) for i in range(3))
                if inj:
                    c3 = HW
                    q[c3:2 * c3], k[c3:2 * c3], q[2 * c3:], k[2 * c3:] = q[:c3], k[:c3], q[:c3], k[:c3]
                ref = _sdpa(q, k, v).reshape(B_, HW, h, Fr, 64).permute(0, 3, 1, 2, 4).reshape(B_ * Fr * HW, C)
                out.append(_res(f"attn[{tag}] temporal F{Fr} inject={inj}", o, ref, KTOL))
                if inj and not naive:   # the shared-softmax forms (one wave / block per source sequence) == per-branch aliasing, bit for bit
                    o2 = torch.zeros_like(o)
                    saved, ops.ATTN_FLAGS = ops.ATTN_FLAGS, ops.ATTN_FLAGS | 8
                    try:
                        ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o2, batch=B_ * HW, heads=h, Sq=Fr, Sk=Fr,
                                      inner=HW, q_strides=st, kv_strides=st, qk_mod=HW)
                    finally:
                        ops.ATTN_FLAGS = saved
                    out.append(_res(f"attn temporal F{Fr} PnP shared-softmax == aliasing form", o, o2.float(), 1e-6 if Fr > 16 else 0.0))
    # deferred rescale (the running maximum only advances when a probability would exceed 2^8): wide score ranges, and
    # keys whose scores grow along the sequence so that the maximum keeps jumping by more than the threshold
    for name, qs, ramp in (("wide scores (|s c| up to ~60)", 3.0, False), ("ramped keys (max jumps every tile)", 1.0, True)):
        b, h, S = 2, 2, 1024
        C = 64 * h
        qkv = rnd(b * S, 3 * C, scale=qs, seed=4242)
        if ramp:
            grow = torch.linspace(0.0, 12.0, S, device=DEV).repeat(b).unsqueeze(1).half()
            qkv[:, C:2 * C] = (qkv[:, C:2 * C].float() * (1.0 + grow.float())).half()
        o = torch.zeros(b * S, C, dtype=torch.float16, device=DEV)
        ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, batch=b, heads=h, Sq=S, Sk=S, inner=1,
                      q_strides=(S, 0, 1), kv_strides=(S, 0, 1))
        q, k, v = (qkv[:, i * C:(i + 1) * C].view(b, S, h, 64).transpose(1, 2) for i in range(3))
        out.append(_res(f"attn[flash] {name}", o, _sdpa(q, k, v).transpose(1, 2).reshape(b * S, C), KTOL))
        # the shared-softmax kernel on the same data (three V streams, branch 0's Q / K)
        b3 = 3
        qkv3 = rnd(b3 * S, 3 * C, scale=qs, seed=777)
        if ramp:
            grow3 = torch.linspace(0.0, 12.0, S, device=DEV).repeat(b3).unsqueeze(1)
            qkv3[:, C:2 * C] = (qkv3[:, C:2 * C].float() * (1.0 + grow3)).half()
        o3 = torch.zeros(b3 * S, C, dtype=torch.float16, device=DEV)
        ops.attention(qkv3[:, :C], qkv3[:, C:2 * C], qkv3[:, 2 * C:], o3, batch=b3, heads=h, Sq=S, Sk=S, inner=1,
                      q_strides=(S, 0, 1), kv_strides=(S, 0, 1), qk_mod=1)
        q, k, v = (qkv3[:, i * C:(i + 1) * C].view(b3, S, h, 64).transpose(1, 2).clone() for i in range(3))
        q[1], k[1], q[2], k[2] = q[0], k[0], q[0], k[0]
        out.append(_res(f"attn[shared softmax] {name}", o3, _sdpa(q, k, v).transpose(1, 2).reshape(b3 * S, C), KTOL))
    out += check_attention_forced_rescale()
    # 8-wave (256-query) blocks: taken for launches with >= 1024 such blocks and Sq, Sk >= 1024; the same launch forced onto
    # 4-wave blocks (flag bit2) must give the same bits (a wave's instruction stream does not depend on the block shape)
    b, h, S = ATTN_8WAVE_SHAPES["plain"]
    C = 64 * h
    qkv = rnd(b * S, 3 * C, scale=1.0, seed=2024)
    o8 = torch.zeros(b * S, C, dtype=torch.float16, device=DEV)
    o4 = torch.zeros_like(o8)
    kw8 = dict(batch=b, heads=h, Sq=S, Sk=S, inner=1, q_strides=(S, 0, 1), kv_strides=(S, 0, 1))
    ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o8, **kw8)
    saved, ops.ATTN_FLAGS = ops.ATTN_FLAGS, ops.ATTN_FLAGS | 4
    try:
        ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o4, **kw8)
    finally:
        ops.ATTN_FLAGS = saved
    out.append(_res("attn[flash] 8-wave blocks == 4-wave blocks (b13 h5 S4096)", o8, o4.float(), 1e-6))
    q, k, v = (qkv[:2 * S, i * C:(i + 1) * C].view(2, S, h, 64).transpose(1, 2) for i in range(3))
    out.append(_res("attn[flash] 8-wave blocks vs fp32 SDPA (first 2 of b13 h5 S4096)", o8[:2 * S],
                    _sdpa(q, k, v).transpose(1, 2).reshape(2 * S, C), KTOL))
    B_, HW, h, Fr = 2, 12, 2, 128  # temporal sequences of 128 frames (BASELINE config 5): frame stride HW
    C = 64 * h
    qkv = rnd(B_ * Fr * HW, 3 * C)
    st = (Fr * HW, 1, HW)
    o = torch.zeros(B_ * Fr * HW, C, dtype=torch.float16, device=DEV)
    ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, batch=B_ * HW, heads=h, Sq=Fr, Sk=Fr, inner=HW, q_strides=st,
                  kv_strides=st)
    def seq128(x):
        return x.reshape(B_, Fr, HW, h, 64).permute(0, 2, 3, 1, 4).reshape(B_ * HW, h, Fr, 64)
    q, k, v = (seq128(qkv[:, i * C:(i + 1) * C]) for i in range(3))
    ref = _sdpa(q, k, v).reshape(B_, HW, h, Fr, 64).permute(0, 3, 1, 2, 4).reshape(B_ * Fr * HW, C)
    out.append(_res("attn[flash] temporal F128 (frame stride)", o, ref, KTOL))
    # every KV-loop length 1 .. 7 tiles with ragged last tiles, shared K/V (kv_div), Q/K aliasing on the plain kernel
    for (b, h, S, Sk, kv_div, qk_mod) in ATTN_FLASH_KV_LOOP_SHAPES:
        C = 64 * h
        q2 = rnd(b * S, C, scale=1.0)
        kv = rnd((b // kv_div) * Sk, 2 * C, scale=1.0)
        o = torch.zeros(b * S, C, dtype=torch.float16, device=DEV)
        ops.attention(q2, kv[:, :C], kv[:, C:], o, batch=b, heads=h, Sq=S, Sk=Sk, inner=1, q_strides=(S, 0, 1),
                      kv_strides=(Sk, 0, 1), kv_div=kv_div, qk_mod=qk_mod)
        q = q2.view(b, S, h, 64).transpose(1, 2).clone()
        k = kv[:, :C].reshape(b // kv_div, Sk, h, 64).transpose(1, 2).repeat_interleave(kv_div, 0).clone()
        v = kv[:, C:].reshape(b // kv_div, Sk, h, 64).transpose(1, 2).repeat_interleave(kv_div, 0)
        if qk_mod:
            for i in range(b):
                q[i], k[i] = q[i % qk_mod], k[i % qk_mod]
        out.append(_res(f"attn[flash] b{b} h{h} S{S} Sk{Sk} kv_div{kv_div} qk_mod{qk_mod}", o,
                        _sdpa(q, k, v).transpose(1, 2).reshape(b * S, C), KTOL))
    # small-head generic kernel (image_latents_temporal_encoder: 2 heads x dim 4)
    B_, Fr, HW, h, d = 2, 6, 10, 2, 4
    qkv = rnd(B_ * Fr * HW, 3 * h * d)
    C = h * d
    o = torch.zeros(B_ * Fr * HW, C, dtype=torch.float16, device=DEV)
    st = (Fr * HW, 1, HW)
    ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, batch=B_ * HW, heads=h, Sq=Fr, Sk=Fr, inner=HW,
                  q_strides=st, kv_strides=st, scale=d ** -0.5, head_dim=d)
    def seq(x):
        return x.reshape(B_, Fr, HW, h, d).permute(0, 2, 3, 1, 4).reshape(B_ * HW, h, Fr, d)
    q, k, v = (seq(qkv[:, i * C:(i + 1) * C]) for i in range(3))
    ref = _sdpa(q, k, v).reshape(B_, HW, h, Fr, d).permute(0, 3, 1, 2, 4).reshape(-1, C)
    out.append(_res("attn small head_dim 4", o, ref, KTOL))
    return out



# ------------------------------------------------------------------------------------------------ CLIP towers (F1)
def attention_small_mfma_specs():
    """(B, heads, S, head_dim, causal, kernel) of ``check_attention_small_mfma``'s self-attention rows."""
    W, L = "whole-sequence MFMA", "96-key loop"
    # (head_dim 40 / 160: ConsistI2V's temporal attention at C = 320 / 1280 with 8 heads -- not multiples of 16 / five 32-column groups)
    return [(2, 16, 257, 80, False, W), (3, 16, 77, 64, True, W), (1, 4, 200, 128, False, W), (2, 3, 50, 96, True, W),
            (1, 2, 288, 64, True, W), (3, 8, 24, 40, False, W), (2, 8, 77, 160, False, W), (5, 8, 16, 160, True, W),
            (2, 4, 90, 56, False, W),      # (head_dim 64 reaches this entry point with the causal mask only: S288 d64 ran the flash kernel without it)
            # longer than 288 keys (or 96 at head_dim 160): the 96-key loop kernel with the online softmax -- SEINE's
            # spatial attention (8 heads x 40 / 80 / 160 over 2560 / 640 / 160 tokens)
            (1, 8, 2560, 40, False, L), (2, 8, 640, 80, False, L), (3, 8, 160, 160, False, L), (1, 2, 401, 56, True, L),
            (2, 3, 289, 24, False, L), (1, 4, 1000, 128, True, L)]


def check_attention_small_mfma():
    """Whole-sequence MFMA attention of the CLIP towers (``anyv2v_attention_small_f16``: head_dim a multiple of 8 up to 160, Sk <= 288) vs
    fp32 SDPA and vs the one-thread-per-query kernel it replaces: ViT-H/14 (257 tokens, 16 x 80), the text tower (77 tokens, 16 x 64,
    causal), head_dim 128, query counts that are not multiples of the 64-query block, column windows of a fused QKV matrix."""
    out = []
    for (B, h, S, d, causal, _kernel) in attention_small_mfma_specs():
        H = h * d
        qkv = rnd(B * S, 3 * H, seed=S + d)
        o = torch.zeros(B * S, H, dtype=torch.float16, device=DEV)
        kw = dict(batch=B, heads=h, Sq=S, Sk=S, inner=1, q_strides=(S, 0, 1), kv_strides=(S, 0, 1), scale=d ** -0.5, head_dim=d,
                  causal=causal)
        ops.attention(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], o, **kw)
        sp = lambda x: x.float().view(B, S, h, d).transpose(1, 2)
        ref = F.scaled_dot_product_attention(sp(qkv[:, :H]), sp(qkv[:, H:2 * H]), sp(qkv[:, 2 * H:]), is_causal=causal)
        ref = ref.transpose(1, 2).reshape(B * S, H)
        out.append(_res(f"attention[small mfma] B{B} h{h} S{S} d{d} causal={causal} vs fp32 SDPA", o, ref, KTOL))
        o2 = torch.zeros_like(o)
        ops.attention(qkv[:, :H], qkv[:, H:2 * H], qkv[:, 2 * H:], o2, naive=True, **kw)
        out.append(_res(f"attention[small mfma] == one-thread-per-query kernel S{S} d{d}", o, o2.float(), 1.5e-3))
    # the temporal layout of the ConsistI2V blocks: one sequence per (clip, pixel), its F rows HW apart; keys = F frames + 8 gathered rows
    Bc, Fr, HW, h, d = 2, 16, 48, 8, 40
    C = h * d
    q = rnd(Bc * Fr * HW, C, seed=5)
    kv = rnd(Bc * HW * (Fr + 8), 2 * C, seed=6)
    o = torch.zeros(Bc * Fr * HW, C, dtype=torch.float16, device=DEV)
    kw = dict(batch=Bc * HW, heads=h, Sq=Fr, Sk=Fr + 8, inner=HW, q_strides=(Fr * HW, 1, HW), kv_strides=(HW * (Fr + 8), Fr + 8, 1),
              scale=d ** -0.5, head_dim=d)
    ops.attention(q, kv[:, :C], kv[:, C:], o, **kw)
    qs = q.float().view(Bc, Fr, HW, h, d).permute(0, 2, 3, 1, 4)                      # [B, HW, h, F, d]
    ks = kv[:, :C].float().view(Bc, HW, Fr + 8, h, d).permute(0, 1, 3, 2, 4)
    vs = kv[:, C:].float().view(Bc, HW, Fr + 8, h, d).permute(0, 1, 3, 2, 4)
    ref = F.scaled_dot_product_attention(qs, ks, vs).permute(0, 3, 1, 2, 4).reshape(Bc * Fr * HW, C)
    out.append(_res("attention[small mfma] temporal layout (inner = HW), 8 x 40, 16 queries x 24 keys vs fp32 SDPA", o, ref, KTOL))
    return out


def check_clip():
    """``anyv2v_amd.clip`` on the real kernels vs ``transformers``' CLIPTextModel / CLIPVisionModelWithProjection in
    fp32 on the CPU, same weights: a tiny pair (3 / 2 layers) and the checkpoint's widths (text 1024 / 16 heads x 64 / 4096 with
    77 tokens and the causal mask; vision ViT-H/14: 1280 / 16 heads x 80 / 5120, 257 tokens, projection 1024) at 2 layers."""
    import transformers
    from anyv2v_amd.clip import CLIPTextTower, CLIPTowerConfig, CLIPVisionTower
    out = []
    for tag, tk, vk in (
        ("tiny", dict(vocab_size=100, hidden_size=128, intermediate_size=256, num_hidden_layers=3, num_attention_heads=2,
                      max_position_embeddings=16),
         dict(hidden_size=160, intermediate_size=320, num_hidden_layers=2, num_attention_heads=2, image_size=224, patch_size=32,
              projection_dim=24)),
        ("checkpoint widths, 2 layers", dict(vocab_size=1000, hidden_size=1024, intermediate_size=4096, num_hidden_layers=2,
                                             num_attention_heads=16, max_position_embeddings=77),
         dict(hidden_size=1280, intermediate_size=5120, num_hidden_layers=2, num_attention_heads=16, image_size=224, patch_size=14,
              projection_dim=1024)),
    ):
        torch.manual_seed(7)
        tcfg = transformers.CLIPTextConfig(bos_token_id=1, eos_token_id=2, hidden_act="gelu", **tk)
        vcfg = transformers.CLIPVisionConfig(hidden_act="gelu", **vk)
        tm, vm = transformers.CLIPTextModel(tcfg).eval(), transformers.CLIPVisionModelWithProjection(vcfg).eval()
        with torch.no_grad():
            for m in (tm, vm):
                for n_, p_ in m.named_parameters():
                    if p_.dim() >= 2:
                        p_.normal_(0, 0.6 / p_.shape[-1] ** 0.5 if p_.dim() == 2 else 0.02)
                    elif "bias" in n_:
                        p_.normal_(0, 0.05)
            # the comparison is against fp32 on the weights the towers hold in fp16
            for m in (tm, vm):
                for p_ in m.parameters():
                    p_.copy_(p_.half().float())
        S = tk["max_position_embeddings"]
        ids = torch.randint(3, tk["vocab_size"], (3, S))
        ids[:, -2:] = 2
        text = CLIPTextTower(CLIPTowerConfig.from_hf(tcfg.to_dict()), tm.state_dict()).to(DEV)
        with torch.no_grad():
            want = tm(ids, output_hidden_states=True)
        ln = getattr(tm, "text_model", tm).final_layer_norm
        hs = text.hidden_states(ids)
        out.append(_res(f"clip text [{tag}] last hidden state (pre-LN, causal)", hs[-1], want.hidden_states[-1], 6e-3))
        for skip in (None, 1):
            with torch.no_grad():
                ref = want.last_hidden_state if skip is None else ln(want.hidden_states[-(skip + 1)])
            out.append(_res(f"clip text [{tag}] encode clip_skip={skip}", text.encode_ids(ids, skip), ref, 8e-3))
        vis = CLIPVisionTower(CLIPTowerConfig.from_hf(vcfg.to_dict()), vm.state_dict()).to(DEV)
        px = torch.randn(2, 3, 224, 224)
        with torch.no_grad():
            ref = vm(pixel_values=px.half().float()).image_embeds
        out.append(_res(f"clip vision [{tag}] image_embeds", vis.image_embeds(px), ref, 8e-3))
    return out

# ------------------------------------------------------------------------------------------------ activations, every fp16 input
def _fp16_key(h):
    """Monotone integer key of an fp16 value (-0 and +0 share key 0): a difference of two keys counts fp16 steps."""
    i = h.view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


def _fp16_ulps(y, exact16):
    """Distance of ``y`` from the correctly rounded result ``exact16`` in fp16 steps (broadcasts)."""
    return (_fp16_key(y) - _fp16_key(exact16)).abs()


def _finite_fp16():
    bits = torch.arange(0, 65536, dtype=torch.int32, device=DEV).to(torch.int16)
    x = bits.view(torch.float16)
    return x[torch.isfinite(x)]                           # 63 488 values


def _round_once_fp16(exact64):
    """float64 -> fp16 in ONE rounding (numpy converts the bits directly; torch's ``.to(float16)`` goes through fp32 and rounds twice:
    2 of the 63 488 exact SiLU values land on the other side of an fp16 tie that way)."""
    import numpy as np
    return torch.from_numpy(exact64.cpu().numpy().astype(np.float16)).to(exact64.device)


def _ulp_row(out, what, tag, y, exact16, digits=2):
    """The activation gate: every element of ``y`` at most 1 fp16 step from ``exact16`` (broadcast), fewer than 1 % of them off at all."""
    d = _fp16_ulps(y, exact16)
    frac = float((d > 0).double().mean())
    worst = int(d.max())
    out.append(dict(name=f"{what} over all {exact16.shape[0]} finite fp16 inputs, {tag}: {100 * frac:.{digits}f} % differ, worst {worst} ulp",
                    err=float(worst), tol=1.0, ok=worst <= 1 and frac < 0.01))


# The activation launches below: each value reaches the activation as the fp32 number equal to the fp16 input.
#  * row-vector form: A = 0 (every product and every partial tile is an exact +0), the values in ``rowvec`` with rowvec_div = 1,
#    M x N of them per launch;
#  * column form (GEGLU takes no rowvec): a[:, 0] = x, w[:, 0] = 1 on the gate rows, the value half = 1 through the bias.
# Families (pinned on the CPU by tests/test_gemm_plan_host.py, rows act_*): 496 x 128 x 64 -> 128-row kernel, unsplit; 64 x 1024 x 2048
# -> 128-row kernel, 4 splits (8 tiles, 32 K-tiles), the activation in gemm_splitk_reduce_kernel.
_ACT_TILE_SHAPE = (496, 128, 64)
_ACT_SPLIT_SHAPE = (64, 1024, 2048)


def _act_rowvec_gemm(x, shape, act, naive=False):
    M, N, K = shape
    n = x.numel()
    rv = torch.zeros(M * N, dtype=torch.float16, device=DEV)
    rv[:n] = x
    a = torch.zeros(M, K, dtype=torch.float16, device=DEV)
    w = torch.ones(N, K, dtype=torch.float16, device=DEV)
    return ops.gemm(a, w, rowvec=rv.view(M, N), rowvec_div=1, act=act, naive=naive).reshape(-1)[:n]


def _act_geglu_gemm(x, N, K, naive=False):
    """[n, N / 2] outputs, every column = 1 * gelu(x).  Packed layout: groups of [16 value | 16 gate] columns."""
    a = torch.zeros(x.numel(), K, dtype=torch.float16, device=DEV)
    a[:, 0] = x
    w = torch.zeros(N, K, dtype=torch.float16, device=DEV)
    b = torch.zeros(N, dtype=torch.float16, device=DEV)
    for g in range(N // 32):
        w[g * 32 + 16:g * 32 + 32, 0] = 1.0
        b[g * 32:g * 32 + 16] = 1.0
    return ops.gemm(a, w, bias=b, act=ops.ACT_GEGLU, naive=naive)


def check_gelu_all_inputs():
    """The GEMM epilogues' erf-GELU (``av_gelu`` in csrc/common.h: max(x,0) - |x| q with the Abramowitz-Stegun 7.1.26 tail) on
    EVERY finite fp16 input, through the GELU and the GEGLU epilogue of the tile kernel and the GEGLU epilogue of the
    weight-stationary one: at most 1 ulp from the correctly rounded exact GELU (float64 erf), and that on < 1 % of the inputs
    (the reference's activation is ``F.gelu`` with the exact erf, diffusers GEGLU; VERDICT r2 #4: no change of semantics).
    The same gate on every other place that evaluates ``av_gelu``: the naive kernel (GELU, GEGLU), the split-K reduce kernel, the
    GEGLU epilogues of the persistent kernel, of the one-wave-per-SIMD kernel and of its stream-K form (main kernel and fix-up
    kernel), and the fused feed-forward kernel -- all output columns of those launches, not one."""
    out = []
    x = _finite_fp16()
    n = x.numel()
    exact = (0.5 * x.double() * (1.0 + torch.erf(x.double() / math.sqrt(2.0))))
    exact16 = exact.to(torch.float16)

    def report(tag, y):
        _ulp_row(out, "erf-GELU", tag, y, exact16 if y.dim() == 1 else exact16[:, None])

    for K, M_pad in ((64, 0), (320, 32768)):   # K = 320 with >= 32768 rows: the weight-stationary kernel
        M = max(n, M_pad)
        a = torch.zeros(M, K, dtype=torch.float16, device=DEV)
        a[:n, 0] = x
        if K == 64:
            w = torch.zeros(128, K, dtype=torch.float16, device=DEV)
            w[:, 0] = 1.0
            report("GELU epilogue (tile kernel)", ops.gemm(a, w, act=ops.ACT_GELU)[:n, 5])
        # GEGLU: value column = 1 (through the bias), gate column = x.  Packed layout: groups of [16 value | 16 gate] columns
        N = 320 if K == 320 else 128
        w = torch.zeros(N, K, dtype=torch.float16, device=DEV)
        b = torch.zeros(N, dtype=torch.float16, device=DEV)
        for g in range(N // 32):
            w[g * 32 + 16:g * 32 + 32, 0] = 1.0
            b[g * 32:g * 32 + 16] = 1.0
        y = ops.gemm(a, w, bias=b, act=ops.ACT_GEGLU)
        report("GEGLU epilogue (%s)" % ("weight-stationary kernel" if K == 320 else "tile kernel"), y[:n, 3])
    from anyv2v_amd import _lib
    saved, saved_glds = ops.GEMM_FLAGS, ops.USE_GLDS
    try:
        ops.USE_GLDS = True   # (split-K and the persistent kernels exist in the LDS-DMA form only)
        report("GELU (naive kernel)", _act_rowvec_gemm(x, _ACT_TILE_SHAPE, ops.ACT_GELU, naive=True))
        report("GEGLU (naive kernel)", _act_geglu_gemm(x, 128, 64, naive=True))
        report("GELU (split-K reduce kernel, 4 splits)", _act_rowvec_gemm(x, _ACT_SPLIT_SHAPE, ops.ACT_GELU))
        # 63488 x 640 (320 outputs per row): 331 x 2 tiles of 192 x 320 on 256 blocks; the one-wave kernel needs two K-tiles; its
        # stream-K form deals the 1324 (tile, K-tile) units to 256 blocks, so whole tiles (main kernel's epilogue) and cut tiles
        # (fix-up kernel's) both occur
        ops.GEMM_FLAGS = (saved & ~_lib.ANYV2V_GEMM_NO_BIG) | _lib.ANYV2V_GEMM_FORCE_BIG
        report("GEGLU epilogue (persistent kernel, forced)", _act_geglu_gemm(x, 640, 64))
        ops.GEMM_FLAGS = saved | _lib.ANYV2V_GEMM_SW
        report("GEGLU epilogue (one-wave-per-SIMD kernel)", _act_geglu_gemm(x, 640, 128))
        ops.GEMM_FLAGS = saved | _lib.ANYV2V_GEMM_FORCE_STREAMK
        report("GEGLU epilogue (one-wave kernel, stream-K: main + fix-up kernels)", _act_geglu_gemm(x, 640, 128))
    finally:
        ops.GEMM_FLAGS, ops.USE_GLDS = saved, saved_glds
    # fused feed-forward (C = 320, hidden = 1280), 320 values per row: gate unit j < 320 copies x[:, j] (an identity block in W1's
    # gate half), every value unit is 1 through the bias, hidden units >= 320 are 1 * gelu(0) = 0; the down-projection is the 0/1
    # matrix that copies hidden unit c to output c.  The kernel rounds the hidden value to fp16 once; 1 x that value + 0 is exact.
    C, H = 320, 1280
    M = (n + C - 1) // C
    xp = torch.zeros(M * C, dtype=torch.float16, device=DEV)
    xp[:n] = x
    w1, b1 = torch.zeros(2 * H, C, dtype=torch.float16, device=DEV), torch.zeros(2 * H, dtype=torch.float16, device=DEV)
    b1[:H] = 1.0
    w1[H:H + C] = torch.eye(C, dtype=torch.float16, device=DEV)
    w2 = torch.zeros(C, H, dtype=torch.float16, device=DEV)
    w2[:, :C] = torch.eye(C, dtype=torch.float16, device=DEV)
    w1p, b1p = _geglu_pack(w1, b1, H)
    y = ops.ff_geglu(xp.view(M, C), w1p, b1p, ops.ff_pack_w2(w2), torch.zeros(C, dtype=torch.float16, device=DEV))
    report("GEGLU (fused feed-forward kernel)", y.reshape(-1)[:n])
    return out


# ------------------------------------------------------------------------------------------------ SiLU, every fp16 input
def _gn_beta_launches(C, rows, x, const, run):
    """The 63 488 values ``x`` through a GroupNorm kernel, C per launch: ``run(X, gamma, beta, out)`` with the constant input
    ``const``, gamma = -0 and beta = the next C values.  (x - mean) rstd is an exact +0 (sums about a pivot taken from the data are
    s = q = 0, so mean = the constant; sums about 0 need const = 0), times -0 is -0, and -0 + beta = beta for every beta, -0
    included: the kernel's pre-activation is beta[c], bit for bit, in every row.  Returns (outputs [launches, rows, C], betas)."""
    n = x.numel()
    L = (n + C - 1) // C
    betas = torch.zeros(L * C, dtype=torch.float16, device=DEV)
    betas[:n] = x
    betas = betas.view(L, C)
    X = torch.full((rows, C), const, dtype=torch.float16, device=DEV)
    gamma = torch.full((C,), -0.0, dtype=torch.float16, device=DEV)
    ys = torch.empty(L, rows, C, dtype=torch.float16, device=DEV)
    for i in range(L):
        run(X, gamma, betas[i], ys[i])
    return ys, betas


def check_silu_all_inputs():
    """SiLU on EVERY finite fp16 input through every kernel that computes it, against x / (1 + exp(-x)) in float64 rounded ONCE to
    fp16: at most 1 ulp, on fewer than 1 % of the inputs (the erf-GELU gate).  4 855 of the exact results are fp16 subnormals (a
    kernel that flushes them fails), 12 013 round to +-0 (the key treats -0 and +0 alike).  fp32 torch evaluations of the kernels'
    formulas differ from the exact result on 1 to 3 inputs, by 1 ulp.

    ``av_silu`` (csrc/common.h, x / (1 + __expf(-x))): the elementwise kernel; the 128-row GEMM kernel's epilogue with register and
    with LDS-DMA staging; the naive kernel; the split-K reduce kernel.  ``gn_silu`` (norm.hip, x * v_rcp(1 + v_exp(-x log2 e))):
    the apply kernel of the one-call GroupNorm in three launch plans (C = 320: 6 rows per block; C = 1280 and C = 2560: one row
    per block, 160 / 320 threads; each with the 4-row unrolled loop and its tail), of the one-all-reduce sharded pair (sums about 0:
    its input is 0, not 0.5), of the pivoted sharded path, and the apply-from-records kernel (records written by hand: pivot = the
    constant, s = q = 0).  Every GroupNorm kernel also runs without SiLU: its output must be beta, bit for bit, which proves
    that the values reach the activation intact."""
    from anyv2v_amd import _lib
    out = []
    x = _finite_fp16()
    n = x.numel()
    x64 = x.double()
    exact16 = _round_once_fp16(x64 / (1.0 + torch.exp(-x64)))

    def report(tag, y):   # (three decimals: a correct kernel is off on a handful of inputs, 1 of 63 488 = 0.002 %)
        _ulp_row(out, "SiLU", tag, y, exact16 if y.dim() == 1 else exact16[:, None], digits=3)

    report("elementwise kernel", ops.silu(x.contiguous()))
    saved_glds = ops.USE_GLDS
    try:
        for glds in (False, True):
            ops.USE_GLDS = glds
            report("GEMM epilogue (128-row kernel, %s staging)" % ("LDS-DMA" if glds else "register"),
                   _act_rowvec_gemm(x, _ACT_TILE_SHAPE, ops.ACT_SILU))
        report("GEMM epilogue (naive kernel)", _act_rowvec_gemm(x, _ACT_TILE_SHAPE, ops.ACT_SILU, naive=True))
        report("split-K reduce kernel, 4 splits", _act_rowvec_gemm(x, _ACT_SPLIT_SHAPE, ops.ACT_SILU))
    finally:
        ops.USE_GLDS = saved_glds

    lib = _lib.load()
    G, eps, nsg = 32, 1e-5, 2

    def one_call(silu, rpg, stats):
        return lambda X, ga, be, y: ops.groupnorm(X, ga, be, stats, rpg, groups=G, eps=eps, silu=silu, out=y)

    def pivoted(silu, rpg, stats):   # anyv2v_groupnorm_pivot_f16 / _partial_pivot_f16 / _apply_pivot_f16, one shard
        return lambda X, ga, be, y: ops.groupnorm(X, ga, be, stats, rpg, groups=G, eps=eps, silu=silu, out=y, shard=(1, lambda t: t))

    def one_all_reduce(silu, rpg, stats):   # anyv2v_groupnorm_partial_f16 / _apply_f16, one shard: sums about 0
        def run(X, ga, be, y):
            M, C = X.shape
            _lib.check(lib.anyv2v_groupnorm_partial_f16(X.data_ptr(), None, C, 0, stats.data_ptr(), M, rpg, G, ops._stream()))
            _lib.check(lib.anyv2v_groupnorm_apply_f16(X.data_ptr(), None, C, 0, y.data_ptr(), ga.data_ptr(), be.data_ptr(), stats.data_ptr(),
                                                      M, rpg, G, eps, int(silu), 1, ops._stream()))
        return run

    def from_records(silu, rpg, stats):   # anyv2v_groupnorm_apply_stats_f16; hand-written records [16 rows][G][3] = (pivot 0.5, s 0, q 0)
        rec = torch.zeros(ops.gn_stats_floats(nsg * rpg, rpg, G), dtype=torch.float32, device=DEV)
        rec[:3 * (nsg * rpg // 16) * G].view(-1, 3)[:, 0] = 0.5
        return lambda X, ga, be, y: ops.groupnorm_from_stats(X, ga, be, rec, rpg, groups=G, eps=eps, silu=silu, out=y)

    # (kernel, C, rows per statistics group, constant input) x 2 statistics groups.  C = 320, 64 rows: 6 rows per block, 2 blocks of 32
    # rows per group: every thread runs the 4-row unrolled loop once and then its tail.  One row per block at C >= 1280: 42 rows
    # -> 6 blocks of 7 rows, unrolled loop + tail again.
    sites = [("one-call GroupNorm, C 320 (6 rows per block)", one_call, 320, 64, 0.5),
             ("one-call GroupNorm, C 1280 (1 row per block)", one_call, 1280, 42, 0.5),
             ("one-call GroupNorm, C 2560 (320 threads)", one_call, 2560, 42, 0.5),
             ("sharded GroupNorm, one all-reduce (groupnorm_apply_f16)", one_all_reduce, 320, 64, 0.0),
             ("sharded GroupNorm, pivoted (groupnorm_apply_pivot_f16)", pivoted, 320, 64, 0.5),
             ("GroupNorm from GEMM records (groupnorm_apply_stats_f16)", from_records, 320, 64, 0.5)]
    for tag, make, C, rpg, const in sites:
        rows = nsg * rpg
        stats = torch.zeros(ops.gn_scratch_floats(rows, rpg, G), dtype=torch.float32, device=DEV)
        ys, betas = _gn_beta_launches(C, rows, x, const, make(False, rpg, stats))
        same = bool(torch.equal(ys.view(torch.int16), betas.view(torch.int16)[:, None, :].expand_as(ys)))
        out.append(dict(name=f"{tag}, silu=0: every output row == beta, bit for bit ({ys.shape[0]} launches)", err=0.0 if same else 1.0,
                        l2=0.0, tol=0.0, ok=same))
        ys, _ = _gn_beta_launches(C, rows, x, const, make(True, rpg, stats))
        L = ys.shape[0]
        got = ys.permute(1, 0, 2).reshape(rows, L * C)[:, :n]   # [row, value]
        report(f"{tag}, all {rows} rows", got.t())
    return out


# ------------------------------------------------------------------------------------------------ timestep embedding, every timestep
def check_timestep_embedding_all_timesteps():
    """The sinusoidal embedding at t = 0 ... 999 in one launch, at every width the three model families pass (320: all released
    configurations; 64: the mini I2VGen-XL and the SEINE toy UNet; 32: the ConsistI2V toy UNet) and at the edge widths 2 and 1280,
    against float64 cos / sin(t exp(-ln 10000 f / half)).  Per element |got - ref| <= 2^-11 + |arg| 2^-21: the fp16 rounding of a value
    in [-1, 1], plus 4 fp32 ulps on the argument for the kernel's fp32 expf and product (the same formula in fp32 torch on the CPU
    uses 0.50 of the bound).  err = the worst ratio of error to bound."""
    out = []
    t = torch.arange(1000, device=DEV, dtype=torch.float32)
    for dim in (320, 64, 32, 2, 1280):
        half = dim // 2
        arg = t.double()[:, None] * torch.exp(-math.log(10000.0) * torch.arange(half, device=DEV).double() / half)[None]
        ref = torch.cat([arg.cos(), arg.sin()], -1)
        bound = 2.0 ** -11 + torch.cat([arg, arg], -1).abs() * 2.0 ** -21
        got = ops.timestep_embedding(t, dim)
        finite = bool(torch.isfinite(got.float()).all())
        ratio = float(((got.double() - ref).abs() / bound).max()) if finite else float("nan")
        out.append(dict(name=f"timestep embedding dim {dim}, t = 0 ... 999: worst |error| / (2^-11 + |arg| 2^-21) = {ratio:.3f}", err=ratio, l2=0.0,
                        tol=1.0, ok=finite and ratio <= 1.0))
    return out


# ------------------------------------------------------------------------------------------------ elementwise
def check_elementwise():
    out = []
    x = rnd(1000, 33)
    out.append(_res("silu", ops.silu(x), F.silu(x.float()), 2e-3))
    a, b = rnd(777, 13), rnd(777, 13)
    out.append(_res("add", ops.add(a, b), a.float() + b.float(), 2e-3))
    t = torch.tensor([981.0, 1.0, 500.0], device=DEV)
    e = ops.timestep_embedding(t, 320)
    half = 160
    fr = torch.exp(-math.log(10000.0) * torch.arange(half, device=DEV).float() / half)
    arg = t[:, None] * fr[None]
    out.append(_res("timestep embedding", e, torch.cat([arg.cos(), arg.sin()], -1), 2e-3))
    B, C, Fr, H, W = 2, 4, 3, 5, 6
    lat = rnd(B, C, Fr, H, W)
    tok = torch.zeros(B * Fr * H * W, 16, dtype=torch.float16, device=DEV)
    ops.ncfhw_to_tokens(lat, tok, col0=4)
    ref = lat.permute(0, 2, 3, 4, 1).reshape(-1, C)
    out.append(_res("ncfhw_to_tokens", tok[:, 4:8], ref, 0.0))
    back = ops.tokens_to_ncfhw(tok, B, C, Fr, H, W, col0=4)
    out.append(_res("tokens_to_ncfhw", back, lat, 0.0))
    xp = rnd(2 * 8 * 8, 32)
    y = ops.adaptive_avgpool(xp, 2, 8, 8, 32, 32)
    ref = F.adaptive_avg_pool2d(xp.float().view(2, 8, 8, 32).permute(0, 3, 1, 2), (32, 32)).permute(0, 2, 3, 1).reshape(-1, 32)
    out.append(_res("adaptive_avgpool 8->32", y, ref, 2e-3))
    xp = rnd(2 * 64 * 64, 8)
    y = ops.adaptive_avgpool(xp, 2, 64, 64, 32, 32)
    ref = F.adaptive_avg_pool2d(xp.float().view(2, 64, 64, 8).permute(0, 3, 1, 2), (32, 32)).permute(0, 2, 3, 1).reshape(-1, 8)
    out.append(_res("adaptive_avgpool 64->32", y, ref, 2e-3))
    # fused CFG + DDIM step
    Fr, H, W = 3, 4, 5
    vt = rnd(3 * Fr * H * W, 8)
    latx = rnd(1, 4, Fr, H, W)
    coef = torch.tensor([0.8, 0.6, 0.9, math.sqrt(1 - 0.81)], dtype=torch.float32, device=DEV)
    o = torch.zeros_like(latx)
    ops.cfg_ddim_step(vt, 1, 2, 9.0, coef, latx, o)
    v3 = vt[:, :4].float().view(3, Fr, H * W, 4).permute(0, 3, 1, 2).reshape(3, 4, Fr, H, W)
    v = v3[1] + 9.0 * (v3[2] - v3[1])
    xx = latx.float()[0]
    x0 = 0.8 * xx - 0.6 * v
    eps = 0.8 * v + 0.6 * xx
    out.append(_res("cfg + ddim step", o[0], 0.9 * x0 + float(coef[3]) * eps, KTOL))
    o2 = ops.ddim_step(v3[2].half(), latx[0], 0.8, 0.6, 0.9, float(coef[3]))
    x0 = 0.8 * xx - 0.6 * v3[2]
    eps = 0.8 * v3[2] + 0.6 * xx
    out.append(_res("ddim step", o2, 0.9 * x0 + float(coef[3]) * eps, 3e-3))
    # row gather with column windows (ConsistI2V's [own frame ; first frame] / [frames ; first-frame window] key sequences)
    src = rnd(300, 96)
    idx = torch.randint(0, 300, (517,), device=DEV, dtype=torch.int32)
    dst = torch.zeros(517, 80, dtype=torch.float16, device=DEV)
    ops.gather_rows(src, 32, idx, dst, 16, 64)
    want = torch.zeros_like(dst)
    want[:, 16:80] = src[idx.long(), 32:96]
    out.append(dict(name="gather_rows (column windows)", err=float((dst.float() - want.float()).abs().max()), tol=0.0,
                    ok=bool(torch.equal(dst, want))))
    # rotary position embedding in place vs the formula of rotary_embedding.py:29-49 in fp32
    HW_, F_, C_ = 6, 5, 96
    xr = rnd(2 * F_ * HW_, C_)
    got = ops.rotary(xr.clone(), 32, 48, HW_, F_)
    pos = ((torch.arange(xr.shape[0], device=DEV) // HW_) % F_).float()
    freq = 10000.0 ** (-torch.arange(0, 48, 2, device=DEV).float() / 48)
    ang = (pos[:, None] * freq[None]).repeat_interleave(2, dim=1)
    t = xr[:, 32:80].float()
    rot = torch.stack([-t[:, 1::2], t[:, 0::2]], -1).reshape(t.shape)
    want = xr.float().clone()
    want[:, 32:80] = t * ang.cos() + rot * ang.sin()
    out.append(_res("rotary (window of columns, frame positions)", got, want, 2e-3))
    out.append(dict(name="rotary leaves the other columns alone", err=0.0, tol=0.0,
                    ok=bool(torch.equal(got[:, :32], xr[:, :32]) and torch.equal(got[:, 80:], xr[:, 80:]))))
    return out


# ------------------------------------------------------------------------------------------------ model level
def build_pair(cfg_name="mini", seed=1234, oracle_device="cpu"):
    from anyv2v_amd.unet import I2VGenXLUNet, I2VGenXLUNetConfig
    from oracle.unet_oracle import UNetConfig, build_oracle, random_state_dict
    ocfg = UNetConfig.mini() if cfg_name == "mini" else UNetConfig.i2vgen_xl()
    ncfg = I2VGenXLUNetConfig.mini() if cfg_name == "mini" else I2VGenXLUNetConfig()
    sd = random_state_dict(ocfg, seed)
    oracle = build_oracle(ocfg, sd, dtype=torch.float32, device=oracle_device)
    with torch.device("meta"):
        native = I2VGenXLUNet(ncfg)
    native = native.to_empty(device=DEV)
    native.load_state_dict({k: v.to(DEV) for k, v in sd.items()}, strict=True)
    return native, oracle, ocfg


def check_unet_golden():
    """Native UNet + native PnP hooks vs the fixture produced by the reference's own pnp_utils.py on the oracle.  On the GPU
    the bound is 2 x the error of the torch-eager fp16 oracle (with ``oracle.pnp_oracle`` hooks) against the same fixture."""
    import types
    from anyv2v_amd import pnp_utils
    from oracle import pnp_oracle
    out = []
    gold = torch.load(os.path.join(ROOT, "tests", "golden", "pnp_hooks_mini.pt"))
    calibrate = DEV != "cpu"
    m = full_models("mini", gold["mini_seed"], want=("native",) + (("o16",) if calibrate else ()))
    native, o16 = m["native"], m.get("o16")
    inp = {k: v.to(DEV) for k, v in gold["inputs"].items()}
    kw = dict(fps=inp["fps"], image_latents=inp["image_latents"].half(), image_embeddings=inp["image_embeddings"].half(),
              encoder_hidden_states=inp["encoder_hidden_states"].half())
    sample = inp["sample"].half()

    def compare(name, t, ref):
        v = native(sample, t, **kw)[0]
        if calibrate:
            with torch.no_grad():
                v16 = o16(sample, t, **kw)[0]
            out.append(_calibrated(name, v, ref, v16))
        else:
            out.append(_res(name, v.cpu(), ref, 3e-2))

    pipe = types.SimpleNamespace(unet=native)
    pnp_utils.clear_time(pipe)
    compare("unet mini (no hooks) vs reference-run fixture", 981, gold["v_nohook_t981"])
    n, p = gold["n_steps"], gold["pnp"]
    pipe = _hook_all(m, ("o16",) if calibrate else (), n_steps=n, ratios=(p["pnp_f_t"], p["pnp_spatial_attn_t"], p["pnp_temp_attn_t"]))
    try:
        for t in (981, 701, 301, 101):
            pnp_utils.register_time(pipe, t)
            if calibrate:
                pnp_oracle.register_time(o16, t)
            compare(f"unet mini + native PnP hooks t={t} vs reference pnp_utils fixture", t, gold[f"v_hook_t{t}"])
    finally:
        _unhook_all(m, ("o16",) if calibrate else (), pipe)
    return out


def check_foreign_hooks(source="oracle"):
    """Seams B1 / B2: torch-style hook code from OUTSIDE the product package drives the native UNet.

    ``source="reference"``: the reference's own ``i2vgen-xl/pnp_utils.py`` (imported verbatim through
    ``oracle.ref_stubs``; only where /root/reference exists, i.e. the CPU suite) -- its ``register_conv_injection``
    replaces ``up_blocks[1].resnets[1].forward`` (``pnp_utils.py:130-131``) and its ``register_*_attention_pnp`` plug
    ``ModifiedSpaAttnProcessor`` / ``ModifiedTmpAttnProcessor`` objects into 16 ``attn1.processor`` slots (``:235-242,340-347``).
    ``source="oracle"``: ``oracle.pnp_oracle``'s restatement of the same hooks (pinned to the reference by the golden
    fixture) -- what the GPU box can run.  The result must equal the fixture produced by the reference hooks on the oracle
    UNet, and the native hooks' result on the same model."""
    import types
    from anyv2v_amd import pnp_utils
    from anyv2v_amd.unet import Attention, ResnetBlock2D
    out = []
    gold = torch.load(os.path.join(ROOT, "tests", "golden", "pnp_hooks_mini.pt"))
    inp = {k: v.to(DEV) for k, v in gold["inputs"].items()}
    kw = dict(fps=inp["fps"], image_latents=inp["image_latents"].half(), image_embeddings=inp["image_embeddings"].half(),
              encoder_hidden_states=inp["encoder_hidden_states"].half())
    sample = inp["sample"].half()
    n, p = gold["n_steps"], gold["pnp"]
    ts = torch.arange(n).flip(0) * (1000 // n) + 1
    k = lambda name: ts[: int(n * p[name])]
    # native hooks first (reference result for "same model, same kernels")
    native, _, _ = build_pair("mini", gold["mini_seed"])
    pipe = types.SimpleNamespace(unet=native)
    pnp_utils.register_conv_injection(pipe, k("pnp_f_t"))
    pnp_utils.register_spatial_attention_pnp(pipe, k("pnp_spatial_attn_t"))
    pnp_utils.register_temp_attention_pnp(pipe, k("pnp_temp_attn_t"))
    v_native = {}
    for t in (981, 701, 301, 101):
        pnp_utils.register_time(pipe, t)
        v_native[t] = native(sample, t, **kw)[0].float().cpu()
    # foreign hooks on a fresh native model
    native, _, _ = build_pair("mini", gold["mini_seed"])
    pipe = types.SimpleNamespace(unet=native)
    calls = {"attn": 0, "resnet": 0}
    orig_a, orig_r = Attention._run_foreign, ResnetBlock2D._run_foreign

    def count_a(self, *a, **kk):
        calls["attn"] += 1
        return orig_a(self, *a, **kk)

    def count_r(self, *a, **kk):
        calls["resnet"] += 1
        return orig_r(self, *a, **kk)

    Attention._run_foreign, ResnetBlock2D._run_foreign = count_a, count_r
    try:
        if source == "reference":
            from oracle import ref_stubs
            ref = ref_stubs.load_reference_pnp_utils()
            ref.register_conv_injection(pipe, k("pnp_f_t"))
            ref.register_spatial_attention_pnp(pipe, k("pnp_spatial_attn_t"))
            ref.register_temp_attention_pnp(pipe, k("pnp_temp_attn_t"))
            reg_time = lambda t: ref.register_time(pipe, t)
        else:
            from oracle import pnp_oracle
            pnp_oracle.register_conv_injection(native, k("pnp_f_t"))
            pnp_oracle.register_spatial_attention_pnp(native, k("pnp_spatial_attn_t"))
            pnp_oracle.register_temp_attention_pnp(native, k("pnp_temp_attn_t"))
            reg_time = lambda t: pnp_oracle.register_time(native, t)
        assert pnp_utils.has_foreign_hooks(native)
        for t in (981, 701, 301, 101):
            reg_time(t)
            v = native(sample, t, **kw)[0].float().cpu()
            out.append(_res(f"native UNet driven by the {source} hook code t={t} vs reference pnp_utils fixture", v, gold[f"v_hook_t{t}"], 3e-2))
            out.append(_res(f"native UNet: {source} hook code == native hooks t={t}", v, v_native[t], 6e-3))
    finally:
        Attention._run_foreign, ResnetBlock2D._run_foreign = orig_a, orig_r
    # 16 foreign processors + 1 replaced ResNet forward, 4 forwards
    out.append(dict(name=f"seam B1: Attention._run_foreign ran 16 x 4 times ({calls['attn']})", err=float(calls["attn"] != 64), l2=0.0, tol=0.5,
                    ok=calls["attn"] == 64))
    out.append(dict(name=f"seam B2: ResnetBlock2D replaced forward ran 4 times ({calls['resnet']})", err=float(calls["resnet"] != 4), l2=0.0,
                    tol=0.5, ok=calls["resnet"] == 4))
    # the module's own torch-style forward (NCHW in / out) == its token-layout run
    blk = native.up_blocks[2].resnets[0]
    del_forward = native.up_blocks[1].resnets[1].__dict__.pop("forward", None)  # noqa: F841 (restore the class forward)
    g = torch.Generator().manual_seed(3)
    N_, H_ = 4, 8
    x = (torch.randn(N_, blk.in_channels, H_, H_, generator=g)).half().to(DEV)
    temb = torch.randn(N_, native.cfg.time_embed_dim, generator=g).half().to(DEV)
    y = blk(x, temb)
    xf, tf = x.float().cpu(), temb.float().cpu()
    P = {kk: vv.float().cpu() for kk, vv in blk.state_dict().items()}
    h = F.conv2d(F.silu(F.group_norm(xf, 32, P["norm1.weight"], P["norm1.bias"], 1e-5)), P["conv1.weight"], P["conv1.bias"], padding=1)
    h = h + F.linear(F.silu(tf), P["time_emb_proj.weight"], P["time_emb_proj.bias"])[:, :, None, None]
    h = F.conv2d(F.silu(F.group_norm(h, 32, P["norm2.weight"], P["norm2.bias"], 1e-5)), P["conv2.weight"], P["conv2.bias"], padding=1)
    ref_y = F.conv2d(xf, P["conv_shortcut.weight"], P["conv_shortcut.bias"]) + h
    out.append(_res("ResnetBlock2D torch-style forward(NCHW, temb) vs torch fp32", y.float().cpu(), ref_y, 4e-3))
    return out


def config1_inputs(cfg, B, Fr=8, hw=32, seed=8888):
    """BASELINE config 1 inputs: random latents, frame-position planes, seed 8888."""
    g = torch.Generator().manual_seed(seed)
    h, w = (hw, hw) if isinstance(hw, int) else hw
    sample = torch.randn(B, 4, Fr, h, w, generator=g)
    il = torch.randn(B, 4, Fr, h, w, generator=g)
    for i in range(1, Fr):
        il[:, :, i] = i / (Fr - 1)
    ehs = torch.randn(B, 77, cfg.cross_attention_dim, generator=g)
    ie = torch.randn(B, 1, cfg.cross_attention_dim, generator=g)
    return dict(sample=sample, image_latents=il, encoder_hidden_states=ehs, image_embeddings=ie, fps=torch.tensor([8] * B))


def check_unet_vs_oracle(cfg_name="mini", B=3, Fr=4, hw=8, with_pnp=True, tol=3e-2, report=None, calibrate=True):
    """Single denoise step, HIP UNet (fp16) vs CPU oracle (fp32) on identical fp16-rounded weights and inputs.  On the GPU
    every comparison is bounded by 2 x the error of the same oracle model run by PyTorch-ROCm eager in fp16 on this GPU --
    the stand-in for "the reference's fp16 path" (SURVEY.md 8(c) tolerance policy); ``tol`` only applies to the CPU
    emulation of the ops (host-logic tests)."""
    import time
    import types
    from anyv2v_amd import pnp_utils
    from oracle import pnp_oracle
    out = []
    calibrate = calibrate and DEV != "cpu"
    m = full_models(cfg_name, 1234, want=("native", "ocpu") + (("o16",) if calibrate else ()))
    native, oracle, ocfg = m["native"], m["ocpu"], m["ocfg"]
    o16 = m.get("o16")
    inp = config1_inputs(ocfg, B, Fr, hw)
    inp16 = {k: (v.half() if v.is_floating_point() else v) for k, v in inp.items()}
    kw_o = _cond_kw(inp16, "cpu", torch.float32)
    kw_n = _cond_kw(inp16, DEV, torch.float16)

    def compare(name, t):
        with torch.no_grad():
            t0 = time.time()
            vo = oracle(inp16["sample"].float(), t, **kw_o)[0]
            t_cpu = time.time() - t0
            v16 = o16(inp16["sample"].to(DEV), t, **kw_n)[0] if calibrate else None
        vn = native(inp16["sample"].to(DEV), t, **kw_n)[0]
        _sync()
        out.append(_calibrated(name, vn, vo, v16) if calibrate else _res(name, vn.cpu(), vo, tol))
        return t_cpu

    hw_ = (hw, hw) if isinstance(hw, int) else tuple(hw)
    hw = f"{hw_[0]}x{hw_[1]}"
    t_cpu = compare(f"unet {cfg_name} B{B} F{Fr} {hw} step vs oracle", 981)
    if report is not None:
        report[f"cpu_oracle_seconds_{cfg_name}_B{B}"] = t_cpu
    if with_pnp and B == 3:
        ts = [981 - 20 * i for i in range(50)]
        pipe = _hook_all(m, ("ocpu",) + (("o16",) if calibrate else ()), ratios=(0.2, 0.5, 0.8))
        try:
            for t in (981, 301):
                pnp_utils.register_time(pipe, t)
                pnp_oracle.register_time(oracle, t)
                if calibrate:
                    pnp_oracle.register_time(o16, t)
                compare(f"unet {cfg_name} B3 F{Fr} {hw} PnP step t={t} vs oracle", t)
            # shared stem: with branches 1 and 2 fed the same latent / image latents (as the edit loop does), the stem up to
            # the first cross-attention may run on [source, shared]; same result as the full three-branch stem
            smp = inp16["sample"].clone()
            smp[2] = smp[1]
            il = inp16["image_latents"].clone()
            il[2] = il[1]
            kw_s = dict(kw_n, image_latents=il.to(DEV))
            for t in (981, 1):
                pnp_utils.register_time(pipe, t)
                outs = []
                for shared in (False, True):
                    ctx = native._prepare_clip(3, Fr, hw_[0], hw_[1], kw_s["encoder_hidden_states"], kw_s["fps"], kw_s["image_latents"],
                                               kw_s["image_embeddings"])
                    ctx.t_buf.fill_(float(t))
                    ctx.shared_stem = shared
                    outs.append(native._forward_core(ctx, smp.to(DEV).contiguous()).clone())
                out.append(_res(f"unet {cfg_name} shared stem == full stem (t={t}, inject={t == 981})", outs[1][:, :4], outs[0][:, :4].float(),
                                0.0 if DEV != "cpu" else 2e-2))
        finally:
            _unhook_all(m, ("ocpu",) + (("o16",) if calibrate else ()), pipe)
    return out


def check_engine_reuse_across_clips():
    """Multi-clip jobs keep the step engines (static buffers + HIP graphs) and re-point them at the next clip
    (``step_engine.cached_engine`` / ``_StepEngine.rebind``): clip B through engines captured for clip A must be BIT-equal to clip B on a
    fresh pipeline -- any step-invariant tensor left over from clip A would show here.  Covers inversion, the PnP edit with its
    [negative, editing]-only engine (schedules ending early) and the plain CFG loop."""
    from anyv2v_amd import pnp_utils
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMInverseScheduler, DDIMScheduler
    out = []
    native, _, ocfg = build_pair("mini", 1234)
    Fr, hw, n_steps = 4, 8, 6
    h = lambda x: x.half().to(DEV)

    def clip(seed):
        torch.manual_seed(seed)
        inp = config1_inputs(ocfg, 3, Fr, hw)
        return h(inp["sample"][:1]) * (1.0 + 0.1 * seed), h(inp["encoder_hidden_states"]) + 0.05 * seed, h(inp["image_embeddings"]) * (1 + 0.2 * seed), \
            h(inp["image_latents"]) - 0.1 * seed

    def run(pipe, c):
        lat0, ehs, ie, il = c
        pnp_utils.clear_time(pipe)
        pipe.register_modules(scheduler=DDIMInverseScheduler())
        traj = pipe.invert(prompt_embeds=ehs[:1], image_embeddings=ie[:1], image_latents=il[:1], height=hw * 8, width=hw * 8,
                           num_frames=Fr, num_inference_steps=n_steps, guidance_scale=1.0, target_fps=8, latents=lat0,
                           return_trajectory=True)
        T = max(traj.keys())
        sched = DDIMScheduler()
        sched.set_timesteps(n_steps)
        k = lambda r: sched.timesteps[: int(n_steps * r)]
        pnp_utils.register_conv_injection(pipe, k(0.2))
        pnp_utils.register_spatial_attention_pnp(pipe, k(0.4))
        pnp_utils.register_temp_attention_pnp(pipe, k(0.5))
        pipe.register_modules(scheduler=sched)
        ed = pipe.sample_with_pnp(prompt_embeds=ehs[2:3], negative_prompt_embeds=ehs[1:2], image_embeddings=ie[2:3],
                                  image_latents=il[2:3], height=hw * 8, width=hw * 8, num_frames=Fr, num_inference_steps=n_steps,
                                  guidance_scale=9.0, target_fps=8, latents=traj[T].clone(), output_type="latent",
                                  ddim_init_latents_t_idx=0, ddim_inv_latents_path=traj, ddim_inv_prompt_embeds=ehs[:1],
                                  ddim_inv_image_embeddings=ie[:1], ddim_inv_image_latents=il[:1]).frames
        pnp_utils.clear_time(pipe)
        rec = pipe(prompt_embeds=ehs[:1], negative_prompt_embeds=ehs[1:2], image_embeddings=ie[:1], image_latents=il[:1],
                   height=hw * 8, width=hw * 8, num_frames=Fr, num_inference_steps=n_steps, guidance_scale=9.0, target_fps=8,
                   latents=traj[T].clone(), output_type="latent", ddim_init_latents_t_idx=0).frames
        return traj[T].clone(), ed.clone(), rec.clone()

    saved = os.environ.get("ANYV2V_ENGINE_CACHE")
    try:
        os.environ["ANYV2V_ENGINE_CACHE"] = "1"
        pipe = I2VGenXLPipeline(unet=native, scheduler=DDIMInverseScheduler())
        pipe._device = torch.device(DEV)
        a1 = run(pipe, clip(1))
        engines = {k: id(v) for k, v in pipe._engines.items()}
        b1 = run(pipe, clip(2))
        reused = {k: id(v) for k, v in pipe._engines.items()} == engines and len(engines) == 3
        a2 = run(pipe, clip(1))
        os.environ["ANYV2V_ENGINE_CACHE"] = "0"
        fresh = I2VGenXLPipeline(unet=native, scheduler=DDIMInverseScheduler())
        fresh._device = torch.device(DEV)
        b0 = run(fresh, clip(2))
        a0 = run(fresh, clip(1))
    finally:
        if saved is None:
            os.environ.pop("ANYV2V_ENGINE_CACHE", None)
        else:
            os.environ["ANYV2V_ENGINE_CACHE"] = saved
    out.append(dict(name="engines of clip A are the ones clip B runs on (3 kept: inversion, PnP edit, CFG)", err=0.0 if reused else 1.0,
                    l2=0.0, tol=0.0, ok=bool(reused)))
    for tag, got, ref in (("clip B on clip A's engines", b1, b0), ("clip A again after clip B", a2, a0), ("clip A, first use", a1, a0)):
        for name, g, r in zip(("inversion", "PnP edit", "CFG reconstruction"), got, ref):
            out.append(_res(f"engine reuse: {tag}: {name} == fresh pipeline (bitwise)", g, r.float(), 0.0))
    # weights reloaded between clips: the kept engines (their graphs point at the old packed tensors) must not be reused
    try:
        os.environ["ANYV2V_ENGINE_CACHE"] = "1"
        sd = {k: v.clone() for k, v in native.state_dict().items()}
        sd2 = {k: (v * 1.01 if v.is_floating_point() and v.dim() >= 2 else v) for k, v in sd.items()}
        native.load_state_dict(sd2)
        c1 = run(pipe, clip(1))
        os.environ["ANYV2V_ENGINE_CACHE"] = "0"
        c0 = run(fresh, clip(1))
        native.load_state_dict(sd)
    finally:
        if saved is None:
            os.environ.pop("ANYV2V_ENGINE_CACHE", None)
        else:
            os.environ["ANYV2V_ENGINE_CACHE"] = saved
    for name, g, r in zip(("inversion", "PnP edit", "CFG reconstruction"), c1, c0):
        out.append(_res(f"engine reuse: after load_state_dict the kept engines are rebuilt: {name} == fresh pipeline", g, r.float(), 0.0))
    changed = float((c0[0].float() - a0[0].float()).abs().max()) > 1e-4
    out.append(dict(name="engine reuse: the reloaded weights do change the result", err=0.0 if changed else 1.0, l2=0.0, tol=0.0, ok=bool(changed)))
    differs = float((b0[1].float() - a0[1].float()).abs().max()) > 1e-3
    out.append(dict(name="engine reuse: the two clips do differ", err=0.0 if differs else 1.0, l2=0.0, tol=0.0, ok=bool(differs)))
    return out



def check_loops_mini():
    """Multi-step: inversion -> PnP edit with the pipeline (HIP graphs) vs the oracle loops; plus graph == eager."""
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMInverseScheduler, DDIMScheduler
    from anyv2v_amd import pnp_utils
    from oracle import pnp_oracle
    out = []
    native, oracle, ocfg = build_pair("mini", 1234)
    Fr, hw, n_steps = 4, 8, 10
    inp = config1_inputs(ocfg, 3, Fr, hw)
    h = lambda x: x.half()
    lat0 = h(inp["sample"][:1])
    ehs, ie, il = h(inp["encoder_hidden_states"]), h(inp["image_embeddings"]), h(inp["image_latents"])
    # oracle: inversion with the source conditioning (branch 0), then PnP edit
    cond_src = dict(fps=torch.tensor([8]), image_latents=il[:1].float(), image_embeddings=ie[:1].float(),
                    encoder_hidden_states=ehs[:1].float())
    traj_o = pnp_oracle.invert_loop(oracle, lat0.float(), cond_src, n_steps)
    ie_all = torch.cat([ie[:1], torch.zeros_like(ie[2:3]), ie[2:3]])
    il_all = torch.cat([il[:1], il[2:3], il[2:3]])
    cond_all = dict(fps=torch.tensor([8] * 3), image_latents=il_all.float(), image_embeddings=ie_all.float(),
                    encoder_hidden_states=ehs.float())
    pnp_oracle.init_pnp(oracle, n_steps, 0.3, 0.6, 1.0)
    T = max(traj_o.keys())
    edited_o = pnp_oracle.pnp_loop(oracle, traj_o[T].clone(), traj_o, cond_all, n_steps, 9.0, t_idx=0)
    # calibration (GPU only): the same loops with the torch-eager fp16 oracle on this GPU; every multi-step bound below is
    # 2 x its drift against the fp32 oracle
    cal = DEV != "cpu"
    if cal:
        o16 = full_models("mini", 1234, want=("o16",))["o16"]
        d16 = lambda c: {k: (v.to(DEV, torch.float16) if v.is_floating_point() else v.to(DEV)) for k, v in c.items()}
        pnp_oracle.clear_hooks(o16)
        traj_e = pnp_oracle.invert_loop(o16, lat0.to(DEV), d16(cond_src), n_steps)
        pnp_oracle.init_pnp(o16, n_steps, 0.3, 0.6, 1.0)
        edited_e = pnp_oracle.pnp_loop(o16, traj_e[T].clone(), traj_e, d16(cond_all), n_steps, 9.0, t_idx=0)
        pnp_oracle.init_pnp(o16, n_steps, 0.2, 0.4, 0.5)
        edited_e2 = pnp_oracle.pnp_loop(o16, traj_e[T].clone(), traj_e, d16(cond_all), n_steps, 9.0, t_idx=0)
        pnp_oracle.clear_hooks(o16)
    bound = lambda name, got, ref, eager, tol: _calibrated(name, got, ref, eager, floor=1e-3) if cal else _res(name, got.cpu(), ref, tol)
    # native pipeline
    for graphs in ((True, False) if DEV != "cpu" else (False,)):
        os.environ["ANYV2V_NO_GRAPH"] = "0" if graphs else "1"
        pipe = I2VGenXLPipeline(unet=native, scheduler=DDIMInverseScheduler())
        pipe._device = torch.device(DEV)
        traj = pipe.invert(prompt_embeds=ehs[:1].to(DEV), image_embeddings=ie[:1].to(DEV), image_latents=il[:1].to(DEV),
                           height=hw * 8, width=hw * 8, num_frames=Fr, num_inference_steps=n_steps, guidance_scale=1.0,
                           target_fps=8, latents=lat0.to(DEV), return_trajectory=True)
        tag = "graph" if graphs else "eager"
        out.append(bound(f"pipeline.invert {n_steps} steps [{tag}] final latent vs oracle", traj[T], traj_o[T], traj_e[T] if cal else None, 5e-2))
        sched = DDIMScheduler()
        sched.set_timesteps(n_steps)
        k = lambda r: sched.timesteps[: int(n_steps * r)]
        pnp_utils.register_conv_injection(pipe, k(0.3))
        pnp_utils.register_spatial_attention_pnp(pipe, k(0.6))
        pnp_utils.register_temp_attention_pnp(pipe, k(1.0))
        pipe.register_modules(scheduler=sched)
        res = pipe.sample_with_pnp(prompt_embeds=ehs[2:3].to(DEV), negative_prompt_embeds=ehs[1:2].to(DEV),
                                   image_embeddings=ie[2:3].to(DEV), image_latents=il[2:3].to(DEV), height=hw * 8,
                                   width=hw * 8, num_frames=Fr, num_inference_steps=n_steps, guidance_scale=9.0,
                                   target_fps=8, latents=traj[T].clone(), output_type="latent", ddim_init_latents_t_idx=0,
                                   ddim_inv_latents_path=traj, ddim_inv_prompt_embeds=ehs[:1].to(DEV),
                                   ddim_inv_image_embeddings=ie[:1].to(DEV), ddim_inv_image_latents=il[:1].to(DEV)).frames
        out.append(bound(f"pipeline.sample_with_pnp {n_steps} steps [{tag}] vs oracle", res, edited_o, edited_e if cal else None, 8e-2))
        if graphs:
            res_graph = res.clone()
        elif DEV != "cpu":
            out.append(_res("pipeline graph replay == eager", res_graph.cpu(), res.cpu(), 1e-3))  # no atomics anywhere: deterministic
        if graphs or DEV == "cpu":
            # schedules that end early: the last steps lie outside every schedule, where the pipeline runs the
            # [negative, editing] branches only (exact: nothing reads the source branch there)
            def edit(skip):
                os.environ["ANYV2V_SRC_SKIP"] = "1" if skip else "0"
                pnp_utils.register_conv_injection(pipe, k(0.2))
                pnp_utils.register_spatial_attention_pnp(pipe, k(0.4))
                pnp_utils.register_temp_attention_pnp(pipe, k(0.5))
                return pipe.sample_with_pnp(prompt_embeds=ehs[2:3].to(DEV), negative_prompt_embeds=ehs[1:2].to(DEV),
                                            image_embeddings=ie[2:3].to(DEV), image_latents=il[2:3].to(DEV), height=hw * 8,
                                            width=hw * 8, num_frames=Fr, num_inference_steps=n_steps, guidance_scale=9.0,
                                            target_fps=8, latents=traj[T].clone(), output_type="latent",
                                            ddim_init_latents_t_idx=0, ddim_inv_latents_path=traj,
                                            ddim_inv_prompt_embeds=ehs[:1].to(DEV), ddim_inv_image_embeddings=ie[:1].to(DEV),
                                            ddim_inv_image_latents=il[:1].to(DEV)).frames
            r_skip, r_full = edit(True), edit(False)
            os.environ["ANYV2V_SRC_SKIP"] = "1"
            # the source branch's dead tail (behind the last hook site) dropped / computed: same latents.  On the GPU bit for bit
            # (the shortened launches run under the batch hint (3, 2)); the CPU emulation's BLAS depends on M
            os.environ["ANYV2V_DROP_SRC_TAIL"] = "0"
            r_tail = edit(True)
            os.environ["ANYV2V_DROP_SRC_TAIL"] = "1"
            if DEV == "cpu":
                out.append(_res(f"source-branch tail dropped == computed [{tag}]", r_skip.cpu(), r_tail.cpu(), 2e-2))
            else:
                out.append(dict(name=f"source-branch tail dropped == computed, bit for bit [{tag}]", tol=0.0,
                                err=float((r_skip.float() - r_tail.float()).abs().max()), ok=bool(torch.equal(r_skip, r_tail))))
            pnp_oracle.init_pnp(oracle, n_steps, 0.2, 0.4, 0.5)
            edited_o2 = pnp_oracle.pnp_loop(oracle, traj_o[T].clone(), traj_o, cond_all, n_steps, 9.0, t_idx=0)
            out.append(bound(f"sample_with_pnp early-ending schedules [{tag}] vs oracle", r_skip, edited_o2, edited_e2 if cal else None, 8e-2))
            out.append(_res(f"source-branch skip on schedule-free steps == full B=3 steps [{tag}]", r_skip.cpu(), r_full.cpu(), 2e-2))  # not bitwise: GEMM tiling (and the CPU BLAS in the emulation) depends on M
    os.environ["ANYV2V_NO_GRAPH"] = "0"
    # A3: plain CFG sampling (DDIM reconstruction), B = 2 [negative, positive]; shared stem on / off
    cond2 = dict(fps=torch.tensor([8] * 2), image_latents=torch.cat([il[2:3], il[2:3]]).float(),
                 image_embeddings=torch.cat([torch.zeros_like(ie[2:3]), ie[2:3]]).float(),
                 encoder_hidden_states=torch.cat([ehs[1:2], ehs[2:3]]).float())
    _, oracle_plain, _ = build_pair("mini", 1234)  # same weights, no hooks registered
    rec_o = pnp_oracle.sample_loop(oracle_plain, traj_o[T].clone(), cond2, n_steps, 9.0, t_idx=0)
    if cal:
        rec_e = pnp_oracle.sample_loop(o16, traj_o[T].clone().to(DEV, torch.float16), d16(cond2), n_steps, 9.0, t_idx=0)
    recs = []
    for shared in ("1", "0"):
        os.environ["ANYV2V_SHARED_STEM"] = shared
        pipe = I2VGenXLPipeline(unet=native, scheduler=DDIMScheduler())
        pipe._device = torch.device(DEV)
        recs.append(pipe(prompt_embeds=ehs[2:3].to(DEV), negative_prompt_embeds=ehs[1:2].to(DEV), image_embeddings=ie[2:3].to(DEV),
                         image_latents=il[2:3].to(DEV), height=hw * 8, width=hw * 8, num_frames=Fr, num_inference_steps=n_steps,
                         guidance_scale=9.0, target_fps=8, latents=traj_o[T].clone().half().to(DEV), output_type="latent",
                         ddim_init_latents_t_idx=0).frames)
    os.environ["ANYV2V_SHARED_STEM"] = "1"
    out.append(bound(f"pipeline.__call__ (CFG sampling) {n_steps} steps vs oracle", recs[0], rec_o, rec_e if cal else None, 8e-2))
    out.append(_res("CFG sampling: shared stem == separate stems", recs[0].cpu(), recs[1].cpu().float(), 0.0 if DEV != "cpu" else 2e-2))
    return out


# ------------------------------------------------------------------------------------------------ N1: full model, benchmarked sizes
_MODELS = {}


def check_source_cache(cfg_name="mini", Fr=4, hw=8, n_steps=6):
    """Multi-edit job (``step_engine.SourceFeatureCache``): three edits of ONE clip -- different prompts and edited frames, the third
    also with shorter injection schedules -- with the cache (the first records, the others replay and run [negative, editing]
    only) must be BIT-EQUAL to the same three edits without it; the cache really is used (replayed steps counted) and is dropped
    when the clip changes."""
    from anyv2v_amd import pnp_utils
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMInverseScheduler, DDIMScheduler
    out = []
    if cfg_name == "full":   # (the full-width model without its CPU oracle: this check compares the product with itself)
        m = full_models("full", 1234, want=("native",))
        native, ocfg = m["native"], m["ocfg"]
    else:
        native, _, ocfg = build_pair(cfg_name, 1234)
    inp = config1_inputs(ocfg, 3, Fr, hw)
    g = lambda x: x.half().to(DEV)
    lat0, ehs, ie, il = g(inp["sample"][:1]), g(inp["encoder_hidden_states"]), g(inp["image_embeddings"]), g(inp["image_latents"])
    gen = torch.Generator().manual_seed(77)
    edits = []
    for k in range(3):   # (prompt embeds, negative embeds, image embedding, image latents of the edited frame, schedule ratios)
        r = lambda *sh: torch.randn(*sh, generator=gen).half().to(DEV)
        il_k = il[2:3].clone()
        il_k[:, :, 0] = r(*il_k[:, :, 0].shape)
        edits.append((r(*ehs[2:3].shape), ehs[1:2], r(*ie[2:3].shape), il_k, (0.5, 0.67, 1.0) if k < 2 else (0.2, 0.34, 0.5)))

    def run_all(use_cache):
        pipe = I2VGenXLPipeline(unet=native, scheduler=DDIMInverseScheduler())
        pipe._device = torch.device(DEV)
        cache = pipe.enable_source_cache(True) if use_cache else None
        traj = pipe.invert(prompt_embeds=ehs[:1], image_embeddings=ie[:1], image_latents=il[:1], height=hw * 8, width=hw * 8,
                           num_frames=Fr, num_inference_steps=n_steps, guidance_scale=1.0, target_fps=8, latents=lat0,
                           return_trajectory=True)
        T = max(traj.keys())
        res = []
        for (pe, npe, ie_k, il_k, ratios) in edits:
            sched = DDIMScheduler()
            sched.set_timesteps(n_steps)
            pipe.register_modules(scheduler=sched)
            k = lambda r_: sched.timesteps[: int(n_steps * r_)]
            pnp_utils.register_conv_injection(pipe, k(ratios[0]))
            pnp_utils.register_spatial_attention_pnp(pipe, k(ratios[1]))
            pnp_utils.register_temp_attention_pnp(pipe, k(ratios[2]))
            res.append(pipe.sample_with_pnp(prompt_embeds=pe, negative_prompt_embeds=npe, image_embeddings=ie_k, image_latents=il_k,
                                            height=hw * 8, width=hw * 8, num_frames=Fr, num_inference_steps=n_steps,
                                            guidance_scale=9.0, target_fps=8, latents=traj[T].clone(), output_type="latent",
                                            ddim_init_latents_t_idx=0, ddim_inv_latents_path=traj, ddim_inv_prompt_embeds=ehs[:1],
                                            ddim_inv_image_embeddings=ie[:1], ddim_inv_image_latents=il[:1]).frames.float().cpu())
            pnp_utils.clear_time(pipe)
        return res, cache, pipe, traj

    plain, _, _, _ = run_all(False)
    cached, cache, pipe, traj = run_all(True)
    # On the GPU the kernels' arithmetic per output element does not depend on the batch, so the replayed two-branch steps are
    # BIT-equal to the three-branch ones.  The CPU op emulation (torch matmul picks its summation order by shape) is not: there
    # the first edit (recorded, three-branch) must still be bit-equal and the replayed ones agree to fp16 rounding amplified by
    # cfg 9 over the steps -- a wrong feature at any site is an O(1) error (the single-forward check below is the sharp one).
    exact = DEV != "cpu"
    for k in range(3):
        out.append(_res(f"source cache: edit {k} with the cache == without ({'bit-equal' if exact or k == 0 else 'fp16 drift'})",
                        cached[k], plain[k], 0.0 if (exact or k == 0) else 0.12))
    # one forward, every site type on: [negative, editing] with replayed source features vs branches 1, 2 of the three-branch forward
    import types
    smp = torch.cat([lat0, lat0 * 0.7, lat0 * 0.7])
    il3 = torch.cat([il[:1], il[2:3], il[2:3]])
    kw = dict(fps=torch.tensor([8, 8, 8], device=DEV), image_latents=il3, image_embeddings=ie, encoder_hidden_states=ehs)
    p2 = types.SimpleNamespace(unet=native)
    tsl = [981 - 20 * i for i in range(50)]
    pnp_utils.register_conv_injection(p2, tsl)
    pnp_utils.register_spatial_attention_pnp(p2, tsl)
    pnp_utils.register_temp_attention_pnp(p2, tsl)
    pnp_utils.register_time(p2, 981)
    sites = pnp_utils.injection_sites(p2)
    full = Fr * hw * hw
    bufs = {n: torch.zeros((full // {"1": 16, "2": 4, "3": 1}[n.split(".up")[1][0]], c), dtype=torch.float16, device=DEV) for n, _o, c in sites}
    for n, o, _c in sites:
        o.src_io = ("record", bufs[n])
    v3 = native(smp, 981, **kw)[0].float().cpu()
    for n, o, _c in sites:
        o.src_io = ("replay", bufs[n])
    with ops.batch_hint(3, 2):   # (what the replay engine runs under: every launch plans as the three-branch launch it stands for)
        v2 = native(smp[1:], 981, **{k_: v_[1:] for k_, v_ in kw.items()})[0].float().cpu()
    for n, o, _c in sites:
        o.src_io = None
    pnp_utils.clear_time(p2)
    out.append(_res("source cache: one forward, 17 sites replayed ([negative, editing]) vs the three-branch forward", v2, v3[1:],
                    0.0 if exact else 4e-3))
    out.append(_res("source cache: the edits differ from each other (not vacuous)", (plain[0] - plain[1]).abs().max().reshape(1),
                    torch.zeros(1), float("inf")))
    out[-1]["ok"] = bool((plain[0] - plain[1]).abs().max() > 1e-3)
    n_inj = n_steps  # schedules of edit 0 / 1 cover every step at ratio 1.0 for the temporal sites
    ok = cache.recorded_steps >= n_inj and cache.replayed_steps >= n_inj
    out.append(dict(name=f"source cache: recorded {cache.recorded_steps} steps, replayed {cache.replayed_steps} ({cache.nbytes() / 2**20:.1f} MiB)",
                    err=0.0 if ok else 1.0, l2=0.0, tol=0.5, ok=ok))
    # another clip (other trajectory object): the signature changes, nothing of the old clip is replayed
    before = cache.replayed_steps
    traj2 = pipe.invert(prompt_embeds=ehs[:1], image_embeddings=ie[:1], image_latents=il[:1], height=hw * 8, width=hw * 8,
                        num_frames=Fr, num_inference_steps=n_steps, guidance_scale=1.0, target_fps=8, latents=lat0 * 0.5,
                        return_trajectory=True)
    sched = DDIMScheduler()
    sched.set_timesteps(n_steps)
    pipe.register_modules(scheduler=sched)
    pnp_utils.register_conv_injection(pipe, sched.timesteps)
    pnp_utils.register_spatial_attention_pnp(pipe, sched.timesteps)
    pnp_utils.register_temp_attention_pnp(pipe, sched.timesteps)
    pe, npe, ie_k, il_k, _ = edits[0]
    pipe.sample_with_pnp(prompt_embeds=pe, negative_prompt_embeds=npe, image_embeddings=ie_k, image_latents=il_k, height=hw * 8,
                         width=hw * 8, num_frames=Fr, num_inference_steps=n_steps, guidance_scale=9.0, target_fps=8,
                         latents=traj2[max(traj2.keys())].clone(), output_type="latent", ddim_init_latents_t_idx=0,
                         ddim_inv_latents_path=traj2, ddim_inv_prompt_embeds=ehs[:1], ddim_inv_image_embeddings=ie[:1],
                         ddim_inv_image_latents=il[:1])
    pnp_utils.clear_time(pipe)
    ok = cache.replayed_steps == before
    out.append(dict(name="source cache: a new clip empties it (no replay of the old clip's features)", err=0.0 if ok else 1.0, l2=0.0,
                    tol=0.5, ok=ok))
    return out


def full_models(cfg_name="full", seed=1234, want=("native", "o32", "o16")):
    """One set of models per process, shared by the full-size parity checks: the native HIP UNet, the oracle in fp32 on
    the GPU (the CHECKER at sizes the CPU cannot reach in test time; validated against the CPU oracle in
    ``check_n1_config1``), the same oracle run by PyTorch-ROCm eager in fp16 (the stand-in for "the reference's fp16
    path", SURVEY.md 8(c): calibrates every tolerance), and the fp32 CPU oracle -- all from ONE seeded fp16-rounded
    state dict."""
    from anyv2v_amd.unet import I2VGenXLUNet, I2VGenXLUNetConfig
    from oracle.unet_oracle import UNetConfig, build_oracle, random_state_dict
    key = (cfg_name, seed)
    m = _MODELS.setdefault(key, {})
    ocfg = UNetConfig.mini() if cfg_name == "mini" else UNetConfig.i2vgen_xl()
    m["ocfg"] = ocfg
    if any(w not in m for w in want) and "sd" not in m:
        m["sd"] = random_state_dict(ocfg, seed)
    for w in want:
        if w in m:
            continue
        if w == "native":
            ncfg = I2VGenXLUNetConfig.mini() if cfg_name == "mini" else I2VGenXLUNetConfig()
            with torch.device("meta"):
                n = I2VGenXLUNet(ncfg)
            n = n.to_empty(device=DEV)
            n.load_state_dict({k: v.to(DEV) for k, v in m["sd"].items()}, strict=True)
            m[w] = n
        elif w == "o32":
            m[w] = build_oracle(ocfg, m["sd"], dtype=torch.float32, device=DEV)
        elif w == "o16":
            m[w] = build_oracle(ocfg, m["sd"], dtype=torch.float16, device=DEV)
        elif w == "ocpu":
            m[w] = build_oracle(ocfg, m["sd"], dtype=torch.float32, device="cpu")
    return m


def release_models():
    _MODELS.clear()
    if torch.cuda.is_available():
        torch.cuda.empty_cache()


def _sync():
    if DEV != "cpu":
        torch.cuda.synchronize()


_CAPS = None


def _recorded_caps():
    """tests/golden/hip_error_caps.json: the HIP path's own error per whole-model check as last recorded on an MI355X
    (``ANYV2V_RECORD_ERRS=<file> pytest -m gpu`` / ``tools/gpu_check.py`` writes it).  A calibrated bound is never looser than
    3 x that record, so a 3 x regression of the HIP path fails even where eager fp16 is far worse."""
    global _CAPS
    if _CAPS is None:
        import json
        path = os.path.join(ROOT, "tests", "golden", "hip_error_caps.json")
        _CAPS = json.load(open(path)) if os.path.isfile(path) else {}
    return _CAPS


_RECORD = {}


def _calibrated(name, got, ref, eager, factor=2.0, floor=5e-4, key=None, gap_cap=None, max_tol=None):
    """SURVEY.md 8(c) tolerance policy: |HIP fp16 - fp32 oracle| <= 2 x |torch-eager fp16 oracle - fp32 oracle| (+ a floor
    for the cases where both are at rounding level), all three on the same inputs in the same test -- for the max-abs metric AND
    for relative L2 -- and, with ``key``, additionally <= 3 x the HIP error recorded for this check (``_recorded_caps``).
    Every row also reports |HIP - eager fp16| (same normalisation): when both fp16 paths sit far from the fp32 checker but close to
    each other, the CHECKER is the outlier; ``gap_cap`` bounds that distance.  ``max_tol``: a fixed bound the
    calibrated one may not exceed (a calibration arm that shares the model code must not LOOSEN an older fixed bound)."""
    got, ref, eager = got.float().cpu(), ref.float().cpu(), eager.float().cpu()
    if not torch.isfinite(got).all():
        return dict(name=name, err=float("nan"), l2=float("nan"), tol=0.0, ok=False)
    e_h, l2 = _rel(got, ref)
    e_e, l2_e = _rel(eager, ref)
    e_g, l2_g = _rel(got, eager)
    tol = factor * e_e + floor
    tol_l2 = factor * l2_e + floor
    if max_tol is not None:
        tol, tol_l2 = min(tol, max_tol), min(tol_l2, max_tol)
    cap = None
    if key is not None:
        _RECORD[key] = {"err": e_h, "l2": l2, "eager": e_e, "eager_l2": l2_e, "hip_vs_eager": e_g, "hip_vs_eager_l2": l2_g}
        rec = _recorded_caps().get(key)
        if rec is not None:
            cap = 3.0 * rec["err"] + floor
            tol, tol_l2 = min(tol, cap), min(tol_l2, 3.0 * rec["l2"] + floor)
        path = os.environ.get("ANYV2V_RECORD_ERRS")
        if path:
            import json
            json.dump(_RECORD, open(path, "w"), indent=1, sort_keys=True)
    ok = bool(e_h <= tol and l2 <= tol_l2 and (gap_cap is None or e_g <= gap_cap))
    return dict(name=f"{name}  [HIP {e_h:.2e} (l2 {l2:.2e}) | eager fp16 {e_e:.2e} (l2 {l2_e:.2e}) | HIP-vs-eager {e_g:.2e} (l2 {l2_g:.2e})"
                     + (f" <= {gap_cap:.2e}" if gap_cap is not None else "") + (f" | cap {cap:.2e}" if cap else "") + "]",
                err=e_h, l2=l2, tol=tol, tol_l2=tol_l2, ok=ok, eager=e_e, gap=e_g)


def _emulated(fn):
    """Runs ``fn`` with ``anyv2v_amd.ops`` replaced by tests/cpu_ops_emulation.py (plain torch on the CPU, fp32 arithmetic with the
    kernels' fp16 storage points, no HIP graphs) and restores the kernels: an INDEPENDENT fp16-storage implementation of the same model
    on the same weights -- the "eager fp16" arm of ``_calibrated`` for the sibling pipelines, whose reference classes do not exist on
    the GPU box (the fixtures hold their fp32 outputs)."""
    import cpu_ops_emulation as emu
    names = ["gemm", "groupnorm", "layernorm", "softmax_rows", "attention", "silu", "add", "timestep_embedding", "ncfhw_to_tokens",
             "tokens_to_ncfhw", "adaptive_avgpool", "copy_cols", "gather_rows", "rotary", "cfg_ddim_step", "ddim_step", "guided_step", "ff_geglu"]
    saved = {n: getattr(ops, n) for n in names}
    saved_env = os.environ.get("ANYV2V_NO_GRAPH")
    os.environ["ANYV2V_NO_GRAPH"] = "1"
    emu.install()
    try:
        return fn()
    finally:
        for n, f in saved.items():
            setattr(ops, n, f)
        if saved_env is None:
            os.environ.pop("ANYV2V_NO_GRAPH", None)
        else:
            os.environ["ANYV2V_NO_GRAPH"] = saved_env


def _cond_kw(inp16, device, dtype):
    return dict(fps=inp16["fps"].to(device), image_latents=inp16["image_latents"].to(device, dtype),
                image_embeddings=inp16["image_embeddings"].to(device, dtype),
                encoder_hidden_states=inp16["encoder_hidden_states"].to(device, dtype))


def _hook_all(models, names, n_steps=50, ratios=(0.2, 0.5, 0.8)):
    """Native hooks on the native UNet, ``oracle.pnp_oracle`` hooks on the oracles; same schedules (10 / 25 / 40 steps of 50:
    t=981 on all 17 sites, t=701 spatial + temporal, t=301 temporal only, t=101 none)."""
    import types
    from anyv2v_amd import pnp_utils
    from oracle import pnp_oracle
    ts = [981 - 20 * i for i in range(50)] if n_steps == 50 else None
    assert ts is not None
    k = lambda r: ts[: int(n_steps * r)]
    pipe = types.SimpleNamespace(unet=models["native"])
    pnp_utils.register_conv_injection(pipe, k(ratios[0]))
    pnp_utils.register_spatial_attention_pnp(pipe, k(ratios[1]))
    pnp_utils.register_temp_attention_pnp(pipe, k(ratios[2]))
    for n in names:
        pnp_oracle.register_conv_injection(models[n], k(ratios[0]))
        pnp_oracle.register_spatial_attention_pnp(models[n], k(ratios[1]))
        pnp_oracle.register_temp_attention_pnp(models[n], k(ratios[2]))
    return pipe


def _unhook_all(models, names, pipe):
    from anyv2v_amd import pnp_utils
    from oracle import pnp_oracle
    pnp_utils.clear_time(pipe)
    for n in names:
        pnp_oracle.clear_hooks(models[n])


def check_n1_config1(cfg_name="full", Fr=8, hw=32, golden=True, report=None):
    """VERDICT r1 N1 (a)+(b): the FULL 1.42 B model at BASELINE config 1 (8 f x 256^2), B=1 and B=3 with all 17 hook sites
    registered, t in {981, 301} -- the exact ``cpu_baseline`` workload -- HIP fp16 vs (i) the fp32 CPU oracle driven by
    ``oracle.pnp_oracle``, (ii) the full-width fixture generated by the REFERENCE's own ``pnp_utils.py`` on the oracle
    (``tests/golden/make_golden.py`` -> ``pnp_hooks_full_config1.pt``); tolerance = 2 x the eager-fp16 error measured here.
    Also validates the GPU-resident fp32 oracle (the checker of the config-3 tests) against the CPU oracle."""
    import time
    from anyv2v_amd import pnp_utils
    from oracle import pnp_oracle
    out = []
    m = full_models(cfg_name, 1234, want=("native", "o32", "o16", "ocpu"))
    native, o32, o16, ocpu, ocfg = m["native"], m["o32"], m["o16"], m["ocpu"], m["ocfg"]
    inp = config1_inputs(ocfg, 3, Fr, hw)
    inp16 = {k: (v.half() if v.is_floating_point() else v) for k, v in inp.items()}
    sl = lambda d, s: {k: v[s] for k, v in d.items()}
    smp = inp16["sample"]

    def run_all(B, t):
        i16 = sl(inp16, slice(0, B))
        t0 = time.time()
        with torch.no_grad():
            v_cpu = ocpu(i16["sample"].float(), t, **_cond_kw(i16, "cpu", torch.float32))[0]
            t_cpu = time.time() - t0
            v32 = o32(i16["sample"].float().to(DEV), t, **_cond_kw(i16, DEV, torch.float32))[0]
            v16 = o16(i16["sample"].to(DEV), t, **_cond_kw(i16, DEV, torch.float16))[0]
        vn = native(i16["sample"].to(DEV), t, **_cond_kw(i16, DEV, torch.float16))[0]
        return v_cpu, v32, v16, vn, t_cpu

    v_cpu, v32, v16, vn, t_cpu = run_all(1, 981)
    if report is not None:
        report[f"cpu_oracle_seconds_{cfg_name}_B1"] = t_cpu
    out.append(_res(f"fp32 oracle on the GPU == fp32 oracle on the CPU ({cfg_name}, config 1, B=1)", v32.cpu(), v_cpu, 2e-4))
    out.append(_calibrated(f"unet {cfg_name} config 1 B=1 t=981 vs CPU fp32 oracle", vn, v_cpu, v16, key=f"n1c1:{cfg_name}:F{Fr}x{hw}:B1:t981"))
    pipe = _hook_all(m, ("o32", "o16", "ocpu"))
    gold = None
    gpath = os.path.join(ROOT, "tests", "golden", "pnp_hooks_full_config1.pt")
    if golden and cfg_name == "full" and (Fr, hw) == (8, 32):
        gold = torch.load(gpath)
        assert gold["weights_seed"] == 1234 and gold["input_seed"] == 8888 and tuple(gold["shape"]) == (3, 4, Fr, hw, hw)
    try:
        for t in (981, 301):
            pnp_utils.register_time(pipe, t)
            for n in ("o32", "o16", "ocpu"):
                pnp_oracle.register_time(m[n], t)
            v_cpu, v32, v16, vn, t_cpu = run_all(3, t)
            if report is not None:
                report[f"cpu_oracle_seconds_{cfg_name}_B3_t{t}"] = t_cpu
            out.append(_res(f"fp32 oracle GPU == CPU ({cfg_name}, config 1, B=3 + hooks, t={t})", v32.cpu(), v_cpu, 2e-4))
            out.append(_calibrated(f"unet {cfg_name} config 1 B=3 + 17 hook sites t={t} vs CPU fp32 oracle (pnp_oracle)", vn, v_cpu, v16,
                                   key=f"n1c1:{cfg_name}:F{Fr}x{hw}:B3:t{t}"))
            if gold is not None:
                out.append(_res(f"CPU oracle + pnp_oracle == fixture of the reference's pnp_utils on the oracle, t={t}", v_cpu,
                                gold[f"v_hook_t{t}"], 1e-4))
                out.append(_calibrated(f"unet full config 1 B=3 + hooks t={t} vs reference-pnp_utils fixture", vn,
                                       gold[f"v_hook_t{t}"], v16, key=f"n1c1:fixture:t{t}"))
    finally:
        _unhook_all(m, ("o32", "o16", "ocpu"), pipe)
    return out


def check_n1_config3_step(cfg_name="full", Fr=16, hw=64, report=None, hooked_ts=(981, 301), chunked=None, plain_fp32_too=False,
                          batches=(1, 3)):
    """ONE step at the benchmarked size -- BASELINE config 3, latents [B,4,16,64,64] -- B=1 (inversion
    step) and B=3 with all 17 hook sites (PnP step; t=981 every site on, t=301 temporal only), HIP fp16 vs the fp32 oracle
    run by torch-eager on the GPU (checker only), tolerance 2 x the eager-fp16 oracle's error at this size.

    ``chunked`` (default: for clips longer than 16 frames, i.e. the config-5 geometry): both eager oracles are evaluated through
    ``oracle/chunked.py`` -- pieces no larger than the config-3 rows' tensors, same arithmetic per output element -- because a plain
    eager activation at [3,4,128,64,64] reaches 4.03 G elements / 16 GB (the un-chunked fp32 checker was the
    suspected outlier of the 0.142 row).  ``plain_fp32_too`` also runs the un-chunked fp32 oracle and reports it against the
    chunked one (diagnostic: locates the checker's own error).  The B=3 rows additionally bound |HIP - eager fp16| by 3 x the
    eager-vs-fp32 error of the B=1 row: the two fp16 implementations must stay as close to each other as one of them is to fp32."""
    import time
    from anyv2v_amd import pnp_utils
    from oracle import chunked as ch
    from oracle import pnp_oracle
    out = []
    m = full_models(cfg_name, 1234, want=("native", "o32", "o16"))
    native, o32, o16, ocfg = m["native"], m["o32"], m["o16"], m["ocfg"]
    inp = config1_inputs(ocfg, 3, Fr, hw)
    inp16 = {k: (v.half() if v.is_floating_point() else v) for k, v in inp.items()}
    sl = lambda d, s: {k: v[s] for k, v in d.items()}
    if chunked is None:
        chunked = Fr > 16
    tag = " (chunked eager oracles)" if chunked else ""

    def run_oracle(o, dt, i16, t, B, use_chunks):
        if use_chunks:
            ch.enable_chunking(o, B, Fr, frame_chunk=16, row_chunk=max(1, 65536 // (hw * Fr)))
        try:
            with torch.no_grad():
                x = i16["sample"].to(DEV, dt)
                return o(x, t, **_cond_kw(i16, DEV, dt))[0].cpu()
        finally:
            if use_chunks:
                ch.disable_chunking(o)

    def run_all(B, t):
        i16 = sl(inp16, slice(0, B))
        _sync()
        t0 = time.time()
        v32 = run_oracle(o32, torch.float32, i16, t, B, chunked)
        _sync()
        t32 = time.time() - t0
        v16 = run_oracle(o16, torch.float16, i16, t, B, chunked)
        vn = native(i16["sample"].to(DEV), t, **_cond_kw(i16, DEV, torch.float16))[0]
        _sync()
        if report is not None:
            report[f"gpu_fp32_oracle_seconds_{cfg_name}_B{B}_F{Fr}_{hw}"] = t32
        print(f"     [B={B} t={t}: fp32 oracle{tag} {t32:.1f} s]", flush=True)
        return v32, v16.cpu(), vn.cpu()

    gap_cap = None
    if 1 in batches:
        v32, v16, vn = run_all(1, 981)
        r = _calibrated(f"unet {cfg_name} [1,4,{Fr},{hw},{hw}] t=981 vs fp32 oracle{tag}", vn, v32, v16, key=f"n1step:{cfg_name}:F{Fr}x{hw}:B1:t981")
        out.append(r)
        gap_cap = 3.0 * r["eager"] + 5e-4
    if 3 not in batches:
        return out
    if gap_cap is None:   # B=1 row skipped: its recorded eager-fp16 error
        rec = _recorded_caps().get(f"n1step:{cfg_name}:F{Fr}x{hw}:B1:t981")
        gap_cap = 3.0 * rec["eager"] + 5e-4 if rec is not None else None
    pipe = _hook_all(m, ("o32", "o16"))
    try:
        for t in hooked_ts:
            pnp_utils.register_time(pipe, t)
            for n in ("o32", "o16"):
                pnp_oracle.register_time(m[n], t)
            v32, v16, vn = run_all(3, t)
            # (the distance between the two fp16 implementations cannot be asked to be smaller than the eager one's own error on THIS
            #  row: at [3,4,128,64,64] eager fp16 has isolated outliers -- max-rel 2.8e-2 at rel-L2 6.7e-3 -- that the HIP path, 2.1e-3 /
            #  2.1e-3 from fp32, does not share; profiles/r04_gputest_n1_log.txt)
            cap_t = None if gap_cap is None else max(gap_cap, 3.0 * _rel(v16, v32)[0] + 5e-4)
            out.append(_calibrated(f"unet {cfg_name} [3,4,{Fr},{hw},{hw}] + 17 hook sites t={t} vs fp32 oracle{tag}", vn, v32, v16,
                                   key=f"n1step:{cfg_name}:F{Fr}x{hw}:B3:t{t}", gap_cap=cap_t))
            if plain_fp32_too and chunked:
                i16 = sl(inp16, slice(0, 3))
                t0 = time.time()
                p32 = run_oracle(o32, torch.float32, i16, t, 3, False)
                _sync()
                e, l2 = _rel(p32, v32)
                print(f"     [diagnostic, B=3 t={t}: UN-chunked fp32 eager oracle vs chunked fp32 oracle: max-rel {e:.3e}, rel-L2 {l2:.3e} "
                      f"({time.time() - t0:.1f} s); HIP vs un-chunked fp32: {_rel(vn, p32)[0]:.3e}]", flush=True)
                p16 = run_oracle(o16, torch.float16, i16, t, 3, False)
                e, l2 = _rel(p16, v16)
                print(f"     [diagnostic, B=3 t={t}: UN-chunked fp16 eager oracle vs chunked fp16 eager oracle: max-rel {e:.3e}, rel-L2 {l2:.3e}]",
                      flush=True)
                if report is not None:
                    report[f"plain_fp32_vs_chunked_fp32_B3_F{Fr}_{hw}_t{t}"] = _rel(p32, v32)
                    report[f"plain_fp16_vs_chunked_fp16_B3_F{Fr}_{hw}_t{t}"] = (e, l2)
    finally:
        _unhook_all(m, ("o32", "o16"), pipe)
    return out


def check_n1_drift(cfg_name="full", Fr=16, hw=64, n_steps=50, every=10, report=None):
    """n-step DDIM inversion -> n-step PnP edit, and inversion -> plain CFG reconstruction, through the
    product pipeline (HIP graphs) vs the oracle loops in fp32 on the GPU; latent drift reported every ``every`` steps and
    bounded by 2 x the drift of the torch-eager fp16 oracle run through the SAME oracle loops.  Schedules 0.2 / 0.5 / 0.8
    (so injected, partly injected and injection-free steps all occur), cfg 9.0, seed-8888 inputs."""
    from anyv2v_amd import pnp_utils
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMInverseScheduler, DDIMScheduler
    from oracle import pnp_oracle
    out = []
    m = full_models(cfg_name, 1234, want=("native", "o32", "o16"))
    native, ocfg = m["native"], m["ocfg"]
    inp = config1_inputs(ocfg, 3, Fr, hw)
    h = lambda x: x.half()
    lat0 = h(inp["sample"][:1])
    ehs, ie, il = h(inp["encoder_hidden_states"]), h(inp["image_embeddings"]), h(inp["image_latents"])
    ie_all = torch.cat([ie[:1], torch.zeros_like(ie[2:3]), ie[2:3]])
    il_all = torch.cat([il[:1], il[2:3], il[2:3]])
    ratios = (0.2, 0.5, 0.8)

    def oracle_run(o, dt):
        d = lambda x: x.to(DEV, dt)
        cond_src = dict(fps=torch.tensor([8], device=DEV), image_latents=d(il[:1]), image_embeddings=d(ie[:1]),
                        encoder_hidden_states=d(ehs[:1]))
        cond_all = dict(fps=torch.tensor([8] * 3, device=DEV), image_latents=d(il_all), image_embeddings=d(ie_all),
                        encoder_hidden_states=d(ehs))
        cond2 = dict(fps=torch.tensor([8] * 2, device=DEV), image_latents=d(il_all[1:]), image_embeddings=d(ie_all[1:]),
                     encoder_hidden_states=d(ehs[1:]))
        pnp_oracle.clear_hooks(o)
        traj = pnp_oracle.invert_loop(o, d(lat0), cond_src, n_steps)
        T = max(traj.keys())
        rec = {}
        pnp_oracle.sample_loop(o, traj[T].clone(), cond2, n_steps, 9.0, t_idx=0, trace=rec)
        pnp_oracle.init_pnp(o, n_steps, *ratios)
        ed = {}
        pnp_oracle.pnp_loop(o, traj[T].clone(), traj, cond_all, n_steps, 9.0, t_idx=0, trace=ed)
        pnp_oracle.clear_hooks(o)
        return traj, rec, ed

    traj32, rec32, ed32 = oracle_run(m["o32"], torch.float32)
    traj16, rec16, ed16 = oracle_run(m["o16"], torch.float16)
    # product pipeline
    g = lambda x: x.to(DEV)
    pipe = I2VGenXLPipeline(unet=native, scheduler=DDIMInverseScheduler())
    pipe._device = torch.device(DEV)
    traj = pipe.invert(prompt_embeds=g(ehs[:1]), image_embeddings=g(ie[:1]), image_latents=g(il[:1]), height=hw * 8, width=hw * 8,
                       num_frames=Fr, num_inference_steps=n_steps, guidance_scale=1.0, target_fps=8, latents=g(lat0),
                       return_trajectory=True)
    T = max(traj.keys())
    sched = DDIMScheduler()
    sched.set_timesteps(n_steps)
    pipe.register_modules(scheduler=sched)
    rec = {}
    pipe(prompt_embeds=g(ehs[2:3]), negative_prompt_embeds=g(ehs[1:2]), image_embeddings=g(ie[2:3]), image_latents=g(il[2:3]),
         height=hw * 8, width=hw * 8, num_frames=Fr, num_inference_steps=n_steps, guidance_scale=9.0, target_fps=8,
         latents=traj[T].clone(), output_type="latent", ddim_init_latents_t_idx=0, latents_trace=rec)
    k = lambda r: sched.timesteps[: int(n_steps * r)]
    pnp_utils.register_conv_injection(pipe, k(ratios[0]))
    pnp_utils.register_spatial_attention_pnp(pipe, k(ratios[1]))
    pnp_utils.register_temp_attention_pnp(pipe, k(ratios[2]))
    ed = {}
    pipe.sample_with_pnp(prompt_embeds=g(ehs[2:3]), negative_prompt_embeds=g(ehs[1:2]), image_embeddings=g(ie[2:3]),
                         image_latents=g(il[2:3]), height=hw * 8, width=hw * 8, num_frames=Fr, num_inference_steps=n_steps,
                         guidance_scale=9.0, target_fps=8, latents=traj[T].clone(), output_type="latent",
                         ddim_init_latents_t_idx=0, ddim_inv_latents_path=traj, ddim_inv_prompt_embeds=g(ehs[:1]),
                         ddim_inv_image_embeddings=g(ie[:1]), ddim_inv_image_latents=g(il[:1]), latents_trace=ed)
    pnp_utils.clear_time(pipe)
    inv_ts = sorted(traj32.keys())
    fwd_ts = sorted(ed32.keys(), reverse=True)
    tag = f"{cfg_name} [{Fr}f x {hw * 8}^2]"
    rows = []
    for name, order, hip, o32_, o16_ in (("inversion", inv_ts, traj, traj32, traj16), ("reconstruction (inversion -> CFG sampling)", fwd_ts, rec, rec32, rec16),
                                         ("PnP edit (inversion -> sample_with_pnp)", fwd_ts, ed, ed32, ed16)):
        for i in range(every - 1, n_steps, every):
            t = order[i]
            # every row is enforced (round 2: only the final latent): bound = min(2 x eager-fp16 drift, 3 x the HIP drift on record)
            rows.append(_calibrated(f"{tag} {name}: drift after {i + 1} steps (t={t})", hip[t], o32_[t], o16_[t], floor=1e-3,
                                    key=f"drift:{cfg_name}:F{Fr}x{hw}:n{n_steps}:{name.split()[0]}:{i + 1}"))
    out.extend(rows)
    # the round trip itself (how well n-step reconstruction returns to the clean latent) -- same for all three paths
    for nm, r_ in (("HIP", rec[fwd_ts[-1]]), ("fp32 oracle", rec32[fwd_ts[-1]]), ("eager fp16 oracle", rec16[fwd_ts[-1]])):
        e = _res(f"{tag} round trip: {nm} reconstruction vs the clean latent", r_.float().cpu(), lat0.float(), 10.0)
        e["informational"] = True
        out.append(e)
    if report is not None:
        report["drift"] = [(r["name"], r["err"], r.get("eager")) for r in rows]
    return out


def check_inversion_500(cfg_name="full", Fr=16, hw=64, n_steps=500, every=100, report=None):
    """BASELINE config 2 as the reference ships it (configs/group_ddim_inversion/template.yaml:33: 500 inversion steps,
    timesteps 1, 3, ..., 999): the product pipeline's ``invert`` (HIP graphs) vs the oracle's ``invert_loop`` in fp32 on the GPU,
    latent drift every ``every`` steps, bounded by 2 x the eager-fp16 oracle's drift through the same loop."""
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMInverseScheduler
    from oracle import pnp_oracle
    out = []
    m = full_models(cfg_name, 1234, want=("native", "o32", "o16"))
    native, ocfg = m["native"], m["ocfg"]
    inp = config1_inputs(ocfg, 3, Fr, hw)
    h = lambda x: x.half()
    lat0 = h(inp["sample"][:1])
    ehs, ie, il = h(inp["encoder_hidden_states"]), h(inp["image_embeddings"]), h(inp["image_latents"])

    def oracle_run(o, dt):
        d = lambda x: x.to(DEV, dt)
        cond_src = dict(fps=torch.tensor([8], device=DEV), image_latents=d(il[:1]), image_embeddings=d(ie[:1]),
                        encoder_hidden_states=d(ehs[:1]))
        pnp_oracle.clear_hooks(o)
        return pnp_oracle.invert_loop(o, d(lat0), cond_src, n_steps)

    traj32 = {t: v.cpu() for t, v in oracle_run(m["o32"], torch.float32).items()}
    traj16 = {t: v.cpu() for t, v in oracle_run(m["o16"], torch.float16).items()}
    g = lambda x: x.to(DEV)
    pipe = I2VGenXLPipeline(unet=native, scheduler=DDIMInverseScheduler())
    pipe._device = torch.device(DEV)
    traj = pipe.invert(prompt_embeds=g(ehs[:1]), image_embeddings=g(ie[:1]), image_latents=g(il[:1]), height=hw * 8, width=hw * 8,
                       num_frames=Fr, num_inference_steps=n_steps, guidance_scale=1.0, target_fps=8, latents=g(lat0),
                       return_trajectory=True)
    ts = sorted(traj32.keys())
    assert len(ts) == n_steps and sorted(traj.keys()) == ts
    for i in range(every - 1, n_steps, every):
        t = ts[i]
        out.append(_calibrated(f"{cfg_name} [{Fr}f x {hw * 8}^2] {n_steps}-step inversion: drift after {i + 1} steps (t={t})", traj[t],
                               traj32[t], traj16[t], floor=1e-3, key=f"inv{n_steps}:{cfg_name}:F{Fr}x{hw}:{i + 1}"))
    if report is not None:
        report["inversion_500"] = [(r["name"], r["err"], r.get("eager")) for r in out]
    return out


def check_pipeline_vs_reference_fixture(name="mini"):
    """The product pipeline (HIP kernels + HIP graphs on the GPU; op emulation in the CPU suite) vs a fixture produced by the
    REFERENCE'S OWN PIPELINE CLASS on the CPU in fp32 (``tests/golden/make_golden.py --pipeline[-full]``: pipeline_i2vgen_xl.py
    verbatim around the oracle UNet): n-step inversion (every trajectory latent), CFG reconstruction and PnP edit from the
    reference's noisiest latent, on the conditioning tensors the reference's glue code built.  On the GPU every bound is 2 x the
    error of the same oracle model run through the oracle loops in eager fp16 on this GPU; on the CPU emulation a fixed bound."""
    from anyv2v_amd import pnp_utils
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMInverseScheduler, DDIMScheduler
    from oracle import pnp_oracle
    fx = torch.load(os.path.join(ROOT, "tests", "golden", "ref_pipeline_mini.pt" if name == "mini" else "ref_pipeline_full_config1.pt"))
    sp = fx["spec"]
    calibrate = DEV != "cpu"
    m = full_models(sp["cfg"], sp["seed"], want=("native",) + (("o16",) if calibrate else ()))
    native, o16 = m["native"], m.get("o16")
    n_steps, size, Fr, ratios = sp["n_steps"], sp["size"], sp["frames"], sp["ratios"]
    g = lambda x: x.to(DEV)
    inv_ts, T = fx["inv_ts"], fx["T"]
    traj_ref = {t: fx["trajectory"][i] for i, t in enumerate(inv_ts)}
    pipe = I2VGenXLPipeline(unet=native, scheduler=DDIMInverseScheduler())
    pipe._device = torch.device(DEV)
    traj = pipe.invert(prompt_embeds=g(fx["src_pe"]), image_embeddings=g(fx["src_ie"]), image_latents=g(fx["src_il"]), height=size,
                       width=size, num_frames=Fr, num_inference_steps=n_steps, guidance_scale=1.0, target_fps=8, latents=g(fx["lat0"]),
                       return_trajectory=True)
    sched = DDIMScheduler()
    sched.set_timesteps(n_steps)
    pipe.register_modules(scheduler=sched)
    start = g(traj_ref[T])  # both sampling runs start from the REFERENCE's noisiest latent, as its own stage 2 does
    rec = pipe(prompt_embeds=g(fx["rec_pe"]), negative_prompt_embeds=g(fx["rec_npe"]), image_embeddings=g(fx["src_ie"]),
               image_latents=g(fx["src_il"]), height=size, width=size, num_frames=Fr, num_inference_steps=n_steps, guidance_scale=9.0,
               target_fps=8, latents=start.clone(), output_type="latent", ddim_init_latents_t_idx=0).frames
    k = lambda r: sched.timesteps[: int(n_steps * r)]
    pnp_utils.register_conv_injection(pipe, k(ratios[0]))
    pnp_utils.register_spatial_attention_pnp(pipe, k(ratios[1]))
    pnp_utils.register_temp_attention_pnp(pipe, k(ratios[2]))
    from anyv2v_amd.utils import LatentTrajectory
    src = LatentTrajectory()
    for t in inv_ts:
        src[t] = g(traj_ref[t])
    ed = pipe.sample_with_pnp(prompt_embeds=g(fx["pe"]), negative_prompt_embeds=g(fx["npe"]), image_embeddings=g(fx["ie_pos"]),
                              image_latents=g(fx["il_edit"]), height=size, width=size, num_frames=Fr, num_inference_steps=n_steps,
                              guidance_scale=9.0, target_fps=8, latents=start.clone(), output_type="latent",
                              ddim_init_latents_t_idx=0, ddim_inv_latents_path=src, ddim_inv_prompt_embeds=g(fx["src_pe"]),
                              ddim_inv_image_embeddings=g(fx["src_ie"]), ddim_inv_image_latents=g(fx["src_il"])).frames
    pnp_utils.clear_time(pipe)
    tag = f"{name} [{Fr}f x {size}^2, {n_steps} steps]"
    rows = [(f"{tag} pipe.invert vs the reference pipeline's trajectory, t={t}", traj[t], traj_ref[t]) for t in inv_ts]
    rows += [(f"{tag} pipe.__call__ (CFG reconstruction) vs the reference pipeline", rec, fx["rec_ref"]),
             (f"{tag} pipe.sample_with_pnp vs the reference pipeline", ed, fx["edit_ref"])]
    if not calibrate:
        return [_res(n_, a, b.float(), 5e-2) for n_, a, b in rows]
    # eager-fp16 calibration: the same oracle model through the oracle loops on this GPU, same inputs
    d = lambda x: x.to(DEV, torch.float16)
    with torch.no_grad():
        c1 = dict(fps=torch.tensor([8], device=DEV), image_latents=d(fx["src_il"]), image_embeddings=d(fx["src_ie"]),
                  encoder_hidden_states=d(fx["src_pe"]))
        t16 = pnp_oracle.invert_loop(o16, d(fx["lat0"]), c1, n_steps)
        c2 = dict(fps=torch.tensor([8, 8], device=DEV), image_latents=d(torch.cat([fx["src_il"]] * 2)),
                  image_embeddings=d(torch.cat([torch.zeros_like(fx["src_ie"]), fx["src_ie"]])),
                  encoder_hidden_states=d(torch.cat([fx["rec_npe"], fx["rec_pe"]])))
        r16 = pnp_oracle.sample_loop(o16, d(traj_ref[T]).clone(), c2, n_steps, 9.0, t_idx=0)
        c3 = dict(fps=torch.tensor([8, 8, 8], device=DEV), image_latents=d(torch.cat([fx["src_il"], fx["il_edit"], fx["il_edit"]])),
                  image_embeddings=d(torch.cat([fx["src_ie"], torch.zeros_like(fx["ie_pos"]), fx["ie_pos"]])),
                  encoder_hidden_states=d(torch.cat([fx["src_pe"], fx["npe"], fx["pe"]])))
        pnp_oracle.init_pnp(o16, n_steps, *ratios)
        e16 = pnp_oracle.pnp_loop(o16, d(traj_ref[T]).clone(), {t: d(v) for t, v in traj_ref.items()}, c3, n_steps, 9.0, t_idx=0)
        pnp_oracle.clear_hooks(o16)
    eager = [t16[t] for t in inv_ts] + [r16, e16]
    return [_calibrated(n_, a, b, e_, floor=1e-3) for (n_, a, b), e_ in zip(rows, eager)]


def check_full_size_properties():
    """BASELINE config 3 sizes (T = 196608 tokens, N = 48 images, S = 4096), where the CPU oracle is far too slow:
    size-independent identities of each kernel family."""
    out = []
    T, C = 196608, 320
    g = torch.Generator(device="cpu").manual_seed(7)
    r = lambda *sh, scale=1.0: (torch.randn(*sh, generator=g) * scale).to(torch.float16).to(DEV)
    # attention: softmax rows sum to one -> with V == 1 every output is exactly 1; key order does not matter
    N, h, S = 48, 5, 4096
    qk = r(N * S, 2 * C)
    ones = torch.ones(N * S, C, dtype=torch.float16, device=DEV)
    o = torch.empty(N * S, C, dtype=torch.float16, device=DEV)
    kw = dict(batch=N, heads=h, Sq=S, Sk=S, inner=1, q_strides=(S, 0, 1), kv_strides=(S, 0, 1))
    ops.attention(qk[:, :C], qk[:, C:], ones, o, **kw)
    out.append(_res("attention full size: V == 1 -> O == 1 (plain kernel)", o, ones.float(), 2e-3))
    ops.attention(qk[:, :C], qk[:, C:], ones, o, qk_mod=N // 3, **kw)
    out.append(_res("attention full size: V == 1 -> O == 1 (shared-softmax PnP kernel)", o, ones.float(), 2e-3))
    v = r(N * S, C)
    o1 = torch.empty_like(o)
    ops.attention(qk[:, :C], qk[:, C:], v, o1, **kw)
    perm = torch.randperm(S, generator=g).to(DEV)
    idx = (torch.arange(N, device=DEV)[:, None] * S + perm[None, :]).reshape(-1)
    o2 = torch.empty_like(o)
    ops.attention(qk[:, :C], qk[idx, C:].contiguous(), v[idx].contiguous(), o2, **kw)
    out.append(_res("attention full size: invariant under a permutation of the keys", o2, o1.float(), KTOL))
    # GEMM / conv linearity in the activations (fp32 accumulate, one rounding): f(a) + f(b) ~= f(a + b) with exact inputs
    a = (torch.randint(-8, 9, (T, C), generator=g).float() / 8).to(torch.float16).to(DEV)   # sums exact in fp16
    b = (torch.randint(-8, 9, (T, C), generator=g).float() / 8).to(torch.float16).to(DEV)
    w = (torch.randint(-4, 5, (C, C), generator=g).float() / 64).to(torch.float16).to(DEV)
    ya, yb, yab = ops.gemm(a, w), ops.gemm(b, w), ops.gemm((a + b), w)
    out.append(_res("linear 320->320 full size: f(a) + f(b) == f(a + b) on exactly representable data", yab, ya.float() + yb.float(), 1e-3))
    w9 = (torch.randint(-2, 3, (C, 9 * C), generator=g).float() / 64).to(torch.float16).to(DEV)
    cv = dict(mode=ops.MODE_CONV2D, conv=(64, 64, 64, 64, 1, 0))
    ca, cb, cab = ops.gemm(a, w9, **cv), ops.gemm(b, w9, **cv), ops.gemm((a + b), w9, **cv)
    out.append(_res("conv3x3 320->320 @64x64 full size: additive in the input", cab, ca.float() + cb.float(), 2e-3))
    # conv: shifting every image by one pixel row shifts the output (interior rows), i.e. the gather indexes correctly
    x4 = a.view(48, 64, 64, C)
    xs = torch.zeros_like(x4)
    xs[:, 1:] = x4[:, :-1]
    cs = ops.gemm(xs.reshape(T, C).contiguous(), w9, **cv).view(48, 64, 64, C)
    out.append(_res("conv3x3 full size: translation equivariance (rows 2..62)", cs[:, 3:62], ca.view(48, 64, 64, C)[:, 2:61].float(), 1e-3))
    # GroupNorm: per (frame, group) the normalised output has mean 0 / variance 1; LayerNorm likewise per row
    x = r(T, C) * 3 + 1
    stats = torch.empty(ops.gn_scratch_floats(48, 1), dtype=torch.float32, device=DEV)
    one, zero = torch.ones(C, dtype=torch.float16, device=DEV), torch.zeros(C, dtype=torch.float16, device=DEV)
    y = ops.groupnorm(x, one, zero, stats, 4096, groups=32, eps=1e-5).float().view(48, 4096, 32, 10)
    m, v_ = y.mean((1, 3)), y.var((1, 3), unbiased=False)
    out.append(_res("groupnorm full size: group means == 0", m + 1, torch.ones_like(m), 2e-3))
    out.append(_res("groupnorm full size: group variances == 1", v_, torch.ones_like(v_), KTOL))
    yl = ops.layernorm(x, one, zero, 1e-5).float()
    out.append(_res("layernorm full size: row means == 0", yl.mean(1) + 1, torch.ones(T, device=DEV), 2e-3))
    out.append(_res("layernorm full size: row variances == 1", yl.var(1, unbiased=False), torch.ones(T, device=DEV), KTOL))
    return out


def check_vae_kernels():
    """The kernel modes added for the AutoencoderKL: one-sided-pad stride-2 conv, fp32-output GEMM, row softmax, and the
    logits -> softmax -> value chain as one 512-wide attention head."""
    out = []
    for naive in (False, True):
        tag = "naive" if naive else "mfma"
        n, ci, co, H, W = 4, 64, 128, 16, 12
        x, w, b = rnd(n, ci, H, W), rnd(co, ci, 3, 3, scale=1 / math.sqrt(9 * ci)), rnd(co)
        y = ops.gemm(_to_tokens(x), _pack_conv(w), bias=b, mode=ops.MODE_CONV2D, conv=(H, W, H // 2, W // 2, 2, 0, 1),
                     M=n * (H // 2) * (W // 2), naive=naive)
        ref = F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), w.float(), b.float(), stride=2)
        out.append(_res(f"conv3x3[{tag}] stride 2, pad (0,1,0,1) (VAE Downsample2D)", y, _to_tokens(ref), KTOL))
        a, wk = rnd(300, 128), rnd(256, 128, scale=1 / math.sqrt(128))
        bias = rnd(256)
        s32 = ops.gemm(a, wk, bias=bias, act=ops.ACT_F32OUT, naive=naive)
        ref32 = a.float() @ wk.float().t() + bias.float()
        out.append(_res(f"gemm[{tag}] fp32 output", s32, ref32, 2e-5))
    s32 = torch.randn(500, 1000, device=DEV) * 30
    p = ops.softmax_rows(s32, 0.0442)
    out.append(_res("softmax rows fp32 -> fp16", p, torch.softmax(s32 * 0.0442, -1), 2e-3))
    out.append(_res("softmax rows sum to 1", p.float().sum(-1), torch.ones(500, device=DEV), 2e-3))
    # single head, d = 512, S = 1024: logits GEMM (fp32) -> softmax -> value GEMM
    S, C = 1024, 512
    q, k, v = rnd(S, C), rnd(S, C), rnd(S, C)
    logits = ops.gemm(q, k, act=ops.ACT_F32OUT)
    o = ops.gemm(ops.softmax_rows(logits, C ** -0.5), v.t().contiguous())
    ref = F.scaled_dot_product_attention(q.float()[None, None], k.float()[None, None], v.float()[None, None])[0, 0]
    out.append(_res("single 512-wide attention head via GEMM / softmax / GEMM", o, ref, KTOL))
    return out


def check_vae(full: bool = True):
    """Native AutoencoderKL vs the CPU oracle on identical fp16-rounded random weights: mini config, and the full SD-VAE
    architecture (83.65 M parameters) on 2 x 64x64 images / 2 x 8x8 latents."""
    from anyv2v_amd.vae import AutoencoderKL, VAEConfig
    from oracle import vae_oracle as vo
    out = []
    cases = [("mini", VAEConfig.mini(), vo.VAEConfig.mini(), (2, 3, 32, 48), (2, 4, 8, 12))]
    if full:
        cases.append(("full", VAEConfig(), vo.VAEConfig(), (2, 3, 64, 64), (2, 4, 8, 8)))
    for name, ncfg, ocfg, xs, zs in cases:
        oracle = vo.AutoencoderKLOracle(ocfg)
        sd = vo.random_state_dict(ocfg, 11)
        oracle.load_state_dict(sd)
        native = AutoencoderKL(ncfg)
        native.load_state_dict(sd)
        native.to(DEV)
        g = torch.Generator().manual_seed(5)
        x = torch.randn(*xs, generator=g).clamp(-1, 1).half().float()
        z = torch.randn(*zs, generator=g).half().float()
        m0, l0 = oracle.encode_moments(x)
        m1, l1 = native.encode_moments(x.to(DEV))
        # bounds = 3 x the measured error of the full-width model on an MI355X (round 4: mean 1.6e-3, logvar 1.2e-3, decode 2.3e-3)
        out.append(_res(f"vae[{name}] encode: posterior mean vs oracle", m1.cpu(), m0, 5e-3))
        out.append(_res(f"vae[{name}] encode: posterior logvar vs oracle", l1.cpu(), l0, 4e-3))
        d0 = oracle.decode(z)
        d1 = native.decode(z.to(DEV))
        out.append(_res(f"vae[{name}] decode vs oracle", d1.cpu(), d0, 7e-3))
    return out


def check_vae_blocks_vs_reference_fixture():
    """The NATIVE VAE blocks (``anyv2v_amd/vae.py``: ``VAEResnetBlock``, the folded nearest-x2 up-sampler, the one-sided-pad stride-2
    down-sampler) on the HIP kernels against ``tests/golden/vae_blocks_ref.pt`` -- outputs of the reference's vendored copies of those
    diffusers blocks (``seine/models/resnet.py:24-207``, ``make_golden.py --vae-blocks``).  Row F1's pinnable part."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_golden as mg
    from anyv2v_amd import vae as nv
    fx = torch.load(os.path.join(ROOT, "tests", "golden", "vae_blocks_ref.pt"))
    spec = fx["spec"]
    io = mg.vae_block_inputs(spec)
    H, W = spec["hw"]
    sc = nv._Scratch()
    out = []

    def back(t, n, h, w):
        return t.float().view(n, h, w, -1).permute(0, 3, 1, 2).cpu()
    for cin, cout in spec["cases"]:
        name = f"res{cin}_{cout}"
        blk = nv.VAEResnetBlock(cin, cout, spec["groups"])
        blk.load_state_dict(io["weights"][name])
        blk = blk.to(DEV).half()
        for m in blk.modules():
            if hasattr(m, "pack"):
                m.pack()
        y = blk.run(sc, _to_tokens(io["x"][name].to(DEV).half()), H, W)
        out.append(_res(f"vae block {name} (native) vs the reference's ResnetBlock3D(temb=None) fixture", back(y, spec["n"], H, W), fx["out"][name], 3e-3))
    c = spec["sampler_c"]
    for name, stride in (("up", 1), ("down", 2)):
        smp = nv._Sampler(c, stride)
        smp.load_state_dict(io["weights"][name])
        smp = smp.to(DEV).half()
        for m in smp.modules():
            if hasattr(m, "pack"):
                m.pack()
        x = _to_tokens(io["x"][name].to(DEV).half())
        if name == "up":
            y = smp.conv.tokens(x, H, W, up=True)
            out.append(_res("vae up-sampler (native, nearest x2 folded) vs the reference's Upsample3D fixture", back(y, spec["n"], 2 * H, 2 * W), fx["out"]["up"], 3e-3))
        else:
            y = smp.conv.tokens(x, H, W, asym=True)
            out.append(_res("vae down-sampler (native, pad (0,1,0,1) stride 2) vs the reference's Downsample3D fixture (shifted-input identity)",
                            back(y, spec["n"], H // 2, W // 2), fx["out"]["down"], 3e-3))
    return out


def check_consisti2v_hooks():
    """the ConsistI2V hook family (``anyv2v_amd/consisti2v.py``) on the kernels vs the fixture the REFERENCE's
    own ``VideoLDMCrossAttnUpBlock`` + ``consisti2v/pnp_utils.py`` produced on the CPU in fp32 (``make_golden.py --consisti2v``):
    stand-ins for ``unet.up_blocks[1..3]``, un-hooked and with conv + spatial + temporal injection (t = 981) / temporal only (301)."""
    import consisti2v_spec as spec
    from anyv2v_amd import consisti2v as c2
    fx = torch.load(os.path.join(ROOT, "tests", "golden", "consisti2v_decoder_hooks.pt"))
    blocks = {i: spec.fill_weights(c2.VideoLDMCrossAttnUpBlock(**spec.block_kwargs(i))).to(DEV) for i in spec.BLOCKS}

    def call(blk, x, skips, temb, ehs):
        h = lambda t: t.to(DEV).half()
        return blk(h(x), tuple(h(s) for s in skips), h(temb), encoder_hidden_states=h(ehs)).float().cpu()
    got = spec.run_cases(blocks, c2, call)
    out = []
    for i in spec.BLOCKS:
        for case in ["nohook"] + [f"hook_t{t}" for t in spec.TS_CASES]:
            out.append(_res(f"consisti2v up_blocks[{i}] stand-in, {case} vs the reference's own block + hooks", got[f"block{i}_{case}"],
                            fx[f"block{i}_{case}"], 4e-3))
        out.append(dict(name=f"consisti2v up_blocks[{i}]: a timestep outside every schedule == un-hooked (bit-equal)", err=0.0, tol=0.0,
                        ok=bool(torch.equal(got[f"block{i}_nohook"], got[f"block{i}_hook_t101"]))))
    return out


def check_consisti2v_unet():
    """The whole ConsistI2V UNet (``anyv2v_amd/consisti2v.py:VideoLDMUNet3DConditionModel``) on the kernels vs the fixture the
    REFERENCE's own ``VideoLDMUNet3DConditionModel`` + ``consisti2v/pnp_utils.py`` produced on the CPU in fp32
    (``make_golden.py --consisti2v-unet``): toy width, every block type, first-frame concatenation, frame-stride conditioning."""
    import consisti2v_spec as spec
    from anyv2v_amd import consisti2v as c2
    fx = torch.load(os.path.join(ROOT, "tests", "golden", "consisti2v_unet.pt"))
    unet = spec.fill_weights(c2.VideoLDMUNet3DConditionModel(**spec.UNET_CFG)).to(DEV)

    def call(u, sample, t, ehs, first, stride):
        h = lambda v: v.to(DEV).half()
        return u(h(sample), t, encoder_hidden_states=h(ehs), first_frame_latents=h(first), frame_stride=stride).sample.float().cpu()
    got = spec.run_unet_cases(unet, c2, call)
    out = []
    for case in ["nohook"] + [f"hook_t{t}" for t in spec.TS_CASES]:
        out.append(_res(f"consisti2v whole UNet (toy width), {case} vs the reference's own UNet + hooks", got[f"unet_{case}"],
                        fx[f"unet_{case}"], 8e-3))
    out.append(dict(name="consisti2v whole UNet: a timestep outside every schedule == un-hooked (bit-equal)", err=0.0, tol=0.0,
                    ok=bool(torch.equal(got["unet_nohook_t101"], got["unet_hook_t101"]))))
    return out


def check_consisti2v_unet_full():
    """ConsistI2V at the released model's width (1250 M parameters, 16 frames x 32 x 32 latent pixels, [source, negative, editing]) on
    the kernels vs the fixture the REFERENCE's own ``VideoLDMUNet3DConditionModel`` + hooks produced on the CPU in fp32
    (``make_golden.py --consisti2v-unet-full``): the flash kernel with Sk = 2 HW, the whole-sequence MFMA kernel at head_dim 40 / 80 /
    160 with 16 + 8 keys, the fused feed-forward, the persistent GEMM kernels -- everything the timing tool runs."""
    import consisti2v_spec as spec
    from anyv2v_amd import consisti2v as c2
    fx = torch.load(os.path.join(ROOT, "tests", "golden", "consisti2v_unet_full.pt"))
    unet = spec.fill_weights(c2.VideoLDMUNet3DConditionModel(**spec.unet_full_cfg())).to(DEV)

    def call(u, sample, t, ehs, first, stride):
        h = lambda v: v.to(DEV).half()
        return u(h(sample), t, encoder_hidden_states=h(ehs), first_frame_latents=h(first), frame_stride=stride).sample.float().cpu()
    got = spec.run_unet_full_cases(unet, c2, call)
    out = []
    for case in ("full_nohook", "full_hook_t981"):
        out.append(_res(f"consisti2v UNet at the released width (1250 M), {case} vs the reference's own UNet + hooks (fp32 CPU)",
                        got[case], fx[case].float(), 1e-2))
    # (not bit-equal at this size: under injection the source branch's ResNet main path and attention run as launches of their own,
    # a third of the rows, which take other tile / split-K plans -- rounding-level)
    out.append(_res("consisti2v full width: the source branch with hooks on vs off", got["full_hook_t981"][:1], got["full_nohook"][:1], 5e-3))   # measured 1.95e-3 (each is 2.4-2.7e-3 from fp32)
    del unet
    torch.cuda.empty_cache()
    return out


def check_consisti2v_pipeline():
    """ConsistI2V end to end, pipeline level: ``anyv2v_amd.consisti2v_pipeline.ConditionalVideoEditingPipeline`` on the kernels --
    ``encode_vae_video``, ``invert``, ``__call__`` (reconstruction), ``sample_with_pnp`` -- vs the fixture the REFERENCE's own pipeline
    class produced on the CPU in fp32 (``make_golden.py --consisti2v-pipeline``, ``oracle/ref_consisti2v_pipeline.py``); every stage
    starts from the reference's own trajectory.  The edit row (text guidance 35) is gated against an independent fp16-storage run, not a constant."""
    import consisti2v_spec as spec
    fx = torch.load(os.path.join(ROOT, "tests", "golden", "consisti2v_pipeline.pt"))
    files = {t: fx["trajectory"][i] for i, t in enumerate(fx["inv_ts"])}
    nat = spec.native_pipeline_job(DEV, trajectory_from=files)
    out = [dict(name="consisti2v pipeline: inversion timesteps", err=0.0, tol=0.0, ok=nat["inv_ts"] == fx["inv_ts"])]
    out.append(_res("consisti2v pipeline: encode_vae_video", nat["lat0"].float().cpu(), fx["lat0"].float(), 3e-3))
    for i, t in enumerate(fx["inv_ts"]):
        out.append(_res(f"consisti2v pipeline: invert, latents written at t={t}", nat["files"][t].float().cpu(), fx["trajectory"][i].float(), 2e-2))
    out.append(_res("consisti2v pipeline: __call__ reconstruction from t_idx 1", nat["rec_lat"].float().cpu(), fx["rec_lat"].float(), 2e-2))
    # no fixed bound on the amplified row.  Text guidance 35 multiplies the difference of two branch predictions --
    # and their fp16 rounding -- by 35; the bound is 2 x what an independent fp16-storage implementation (the torch op emulation, run
    # here on the CPU on the same weights from the same trajectory) shows against the reference's fp32 output, and 3 x the recorded
    # HIP figure; HIP-vs-emulation is printed.
    emu = _emulated(lambda: spec.native_pipeline_job("cpu", trajectory_from=files))
    # (the emulation arm runs the repo's own model / pipeline code -- it is independent at KERNEL level only -- so it may
    #  tighten but never loosen the former fixed bound of 0.25, and the HIP-vs-emulation distance is capped at 1.5 x its recorded 0.19)
    out.append(_calibrated("consisti2v pipeline: sample_with_pnp (text guidance 35) vs the reference class's output; 'eager' = torch op emulation "
                           "(kernel-independent only)", nat["edit_lat"], fx["edit_lat"], emu["edit_lat"], key="consisti2v_pipeline_pnp_edit",
                           max_tol=0.25, gap_cap=0.29))
    out.append(_calibrated("consisti2v pipeline: __call__ reconstruction (calibrated)", nat["rec_lat"], fx["rec_lat"], emu["rec_lat"],
                           key="consisti2v_pipeline_reconstruction"))
    dec = torch.from_numpy(nat["pipe"].decode_latents(fx["edit_lat"].to(DEV)))
    out.append(_res("consisti2v pipeline: decode_latents of the reference's edited latents", dec, fx["edit_video"].float(), 4e-3))
    return out


def check_consisti2v_sampling():
    """ConsistI2V's samplers next to the runner stages -- ``ConditionalAnimationPipeline``, ``AutoregressiveAnimationPipeline`` (two
    chunks) and ``guidance_rescale`` + ``eta`` on the editing pipeline -- on the kernels vs the fixture the REFERENCE's own classes
    produced on the CPU in fp32 (``make_golden.py --consisti2v-sampling``); seeded noise, drawn on the host on both sides."""
    import consisti2v_spec as spec
    fx = torch.load(os.path.join(ROOT, "tests", "golden", "consisti2v_sampling.pt"))
    got = spec.native_sampling(DEV)
    tol = dict(animation=8e-3, autoregressive=8e-3, rescale_eta=2e-2)      # (3 x measured, profiles/r04_consisti2v_sampling_gpu.txt)
    return [_res(f"consisti2v sampling: {name} ({spec.sampling_cases()[name][0]})", lat.float().cpu(), fx[name].float(), tol[name])
            for name, lat in got.items()]


def check_seine_hooks():
    """the SEINE hook family (``anyv2v_amd/seine.py``) on the kernels vs the fixture the REFERENCE's own
    ``CrossAttnUpBlock3D`` + ``seine/pnp_utils.py`` produced on the CPU in fp32 (``make_golden.py --seine``): un-hooked, and with
    conv + spatial + cross + temporal injection (t = 981) / cross + temporal (501) / temporal only (301)."""
    import seine_spec as spec
    from anyv2v_amd import seine as sn
    fx = torch.load(os.path.join(ROOT, "tests", "golden", "seine_decoder_hooks.pt"))
    blocks = {i: spec.fill_weights(sn.CrossAttnUpBlock3D(**spec.block_kwargs(i)), spec.WEIGHT_SEED).to(DEV) for i in spec.BLOCKS}

    def call(blk, x, skips, temb, ehs):
        h = lambda t: t.to(DEV).half()
        return blk(h(x), tuple(h(s) for s in skips), h(temb), encoder_hidden_states=h(ehs)).float().cpu()
    got = spec.run_cases(blocks, sn, call)
    out = []
    for i in spec.BLOCKS:
        for case in ["nohook"] + [f"hook_t{t}" for t in spec.TS_CASES]:
            out.append(_res(f"seine up_blocks[{i}] stand-in, {case} vs the reference's own block + hooks", got[f"block{i}_{case}"],
                            fx[f"block{i}_{case}"], 4e-3))
        out.append(dict(name=f"seine up_blocks[{i}]: a timestep outside every schedule == un-hooked (bit-equal)", err=0.0, tol=0.0,
                        ok=bool(torch.equal(got[f"block{i}_nohook"], got[f"block{i}_hook_t101"]))))
    return out


def check_seine_unet():
    """The whole SEINE UNet (``anyv2v_amd/seine.py:UNet3DConditionModel``) on the kernels vs the fixture the REFERENCE's own
    ``UNet3DConditionModel`` + ``seine/pnp_utils.py`` produced on the CPU in fp32 (``make_golden.py --seine-unet``)."""
    import seine_spec as spec
    from anyv2v_amd import seine as sn
    fx = torch.load(os.path.join(ROOT, "tests", "golden", "seine_unet.pt"))
    unet = spec.fill_weights(sn.UNet3DConditionModel(**spec.UNET_CFG), spec.WEIGHT_SEED).to(DEV)

    def call(u, sample, t, ehs):
        return u(sample.to(DEV).half(), t, encoder_hidden_states=ehs.to(DEV).half()).sample.float().cpu()
    got = spec.run_unet_cases(unet, sn, call)
    out = []
    for case in ["nohook"] + [f"hook_t{t}" for t in spec.TS_CASES]:
        out.append(_res(f"seine whole UNet (toy width), {case} vs the reference's own UNet + hooks", got[f"unet_{case}"], fx[f"unet_{case}"], 8e-3))
    out.append(dict(name="seine whole UNet: a timestep outside every schedule == un-hooked (bit-equal)", err=0.0, tol=0.0,
                    ok=bool(torch.equal(got["unet_nohook_t101"], got["unet_hook_t101"]))))
    return out


def check_seine_pipeline():
    """SEINE end to end, runner-class level: ``anyv2v_amd.seine_pipeline`` on the kernels vs the fixture the REFERENCE's own
    ``SEINEDDIMInversionPipeline`` / ``SEINEPnPPipeline`` produced on the CPU (``make_golden.py --seine-pipeline``), DDIM and DDPM samplers
    (the DDPM noise is drawn from the CPU generator, the fixture's stream); the edit starts from the reference's own trajectory."""
    import tempfile

    import seine_spec as spec
    fx = torch.load(os.path.join(ROOT, "tests", "golden", "seine_pipeline.pt"))
    files = {t: fx["trajectory"][i] for i, t in enumerate(fx["inv_ts"])}
    out = []
    for sm in ("ddim", "ddpm"):
        with tempfile.TemporaryDirectory() as tmp:
            nat = spec.native_job(DEV, tmp, sm, trajectory_from=files)
        if sm == "ddim":
            out.append(_res("seine runners: frames -> VAE latents", nat["lat0"].float().cpu(), fx["lat0"].float(), 2e-3))
            for i, t in enumerate(fx["inv_ts"]):
                out.append(_res(f"seine runners: ddim_inversion, file at t={t}", nat["files"][t].float().cpu(), fx["trajectory"][i].float(), 1e-2))
            out.append(_res("seine runners: ddim_sample reconstruction", nat["recon_lat"].float().cpu(), fx["recon_lat"].float(), 2e-2))
        out.append(dict(name=f"seine runners: edit timesteps ({sm})", err=0.0, tol=0.0, ok=nat["edit_ts"] == fx[f"edit_ts_{sm}"]))
        with tempfile.TemporaryDirectory() as tmp2:   # (calibrated like the ConsistI2V edit row)
            emu = _emulated(lambda: spec.native_job("cpu", tmp2, sm, trajectory_from=files))
        out.append(_calibrated(f"seine runners: edit_video, {sm} sampler, cfg 4 vs the reference runner's output; 'eager' = torch op emulation "
                               "(kernel-independent only)", nat["edit_lat"], fx[f"edit_lat_{sm}"], emu["edit_lat"], key=f"seine_pipeline_edit_{sm}",
                               max_tol=5e-2, gap_cap=4.5e-2))
        dec = nat["pipe"].decode_latents(fx[f"edit_lat_{sm}"].to(DEV))
        d = int((dec.int() - fx[f"edited_frames_{sm}"].int()).abs().max())
        out.append(dict(name=f"seine runners: decode_latents of the reference's latents ({sm}), max |uint8 diff|", err=float(d), tol=1.0, ok=d <= 1))
    return out


def attention_bias_specs():
    """(heads, head_dim, frames, instantiation) of ``check_attention_bias_and_rotary_windows``."""
    return ((3, 40, 6, "small<2,6,bias>"), (8, 80, 16, "small<3,6,bias>"), (8, 160, 16, "small<5,6,bias>"), (2, 20, 5, "naive+bias"))


def check_attention_bias_and_rotary_windows():
    """``anyv2v_attention_bias_f16`` (additive score bias [heads, Sq, Sk], frame-strided sequences, qk_mod aliasing) and
    ``anyv2v_rotary_f16`` with one window per head vs PyTorch fp32."""
    out = []
    # (head_dim 40 / 80 / 160, 16 frames: SEINE's temporal attention at the released width -- the whole-sequence MFMA kernel with the
    # bias added to the score fragments; head_dim 20: the one-thread-per-query kernel)
    for (heads, D, Fr, _inst) in attention_bias_specs():
        B, HW = 3, 10
        C = heads * D
        qkv = rnd(B * Fr * HW, 3 * C, seed=D)
        bias = torch.randn(heads, Fr, Fr, device=DEV)
        o = torch.zeros(B * Fr * HW, C, dtype=torch.float16, device=DEV)
        for qk_mod in (0, B * HW // 3):
            kw = dict(batch=B * HW, heads=heads, Sq=Fr, Sk=Fr, inner=HW, q_strides=(Fr * HW, 1, HW), kv_strides=(Fr * HW, 1, HW), qk_mod=qk_mod,
                      scale=D ** -0.5, head_dim=D, bias=bias)
            ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o, **kw)
            x = qkv.float().view(B, Fr, HW, 3, heads, D).permute(3, 0, 2, 4, 1, 5)      # [3][B, HW, heads, F, D]
            q, k, v = x[0], x[1], x[2]
            if qk_mod:
                q, k = q[:1].expand_as(q), k[:1].expand_as(k)
            ref = F.scaled_dot_product_attention(q, k, v, attn_mask=bias[None, None], scale=D ** -0.5)   # [B, HW, heads, F, D]
            ref = ref.permute(0, 3, 1, 2, 4).reshape(B * Fr * HW, C)
            out.append(_res(f"attention + score bias, temporal view, {heads} x {D}, {Fr} frames, qk_mod {qk_mod}", o, ref, KTOL))
            o2 = torch.zeros_like(o)
            ops.attention(qkv[:, :C], qkv[:, C:2 * C], qkv[:, 2 * C:], o2, naive=True, **kw)
            out.append(_res(f"attention + score bias == one-thread-per-query kernel, {heads} x {D}, qk_mod {qk_mod}", o, o2.float(), 1.5e-3))
    B, Fr, HW, heads, D = 3, 6, 10, 3, 40
    C = heads * D
    xr = rnd(2 * Fr * HW, C + 16)
    got = ops.rotary(xr.clone(), 8, 32, HW, Fr, windows=heads, window_stride=D)
    pos = ((torch.arange(xr.shape[0], device=DEV) // HW) % Fr).float()
    freq = 10000.0 ** (-torch.arange(0, 32, 2, device=DEV).float() / 32)
    ang = (pos[:, None] * freq[None]).repeat_interleave(2, dim=1)
    want = xr.float().clone()
    for hh in range(heads):
        c0 = 8 + hh * D
        t = xr[:, c0:c0 + 32].float()
        rot = torch.stack([-t[:, 1::2], t[:, 0::2]], -1).reshape(t.shape)
        want[:, c0:c0 + 32] = t * ang.cos() + rot * ang.sin()
    out.append(_res("rotary, one 32-channel window per head", got, want, 2e-3))
    return out


# ------------------------------------------------------------------------------------------------ buffer edges: framed operands
# Every case below runs twice with the same flags: on plain tensors and with ALL operands inside poisoned frames (``_edge_rows``).
# The kernels read past the logical edge of an operand on purpose (clamped rows, W rows past N, key tails) and mask; the frames make
# what they read there NaN and what they may not write checkable.  Every framed operand lies inside one allocation.
def _gemm_edge(name, a0, w, ref, *, a1=None, bias=None, rowvec=None, rowvec_div=0, residual=None, act=0, M=None, ln=None, c_cols=8, **kw):
    Mout = a0.shape[0] if M is None else M
    n_out = w.shape[0] // 2 if act == ops.ACT_GEGLU else w.shape[0]
    cdt = torch.float32 if act == ops.ACT_F32OUT else torch.float16

    def run(f):
        lnf = None if ln is None else (f.inp(ln[0], flat=True), ln[1])
        return ops.gemm(f.inp(a0), f.inp(w, flat=True), a1=f.inp(a1), bias=f.inp(bias), rowvec=f.inp(rowvec), rowvec_div=rowvec_div,
                        residual=f.inp(residual), act=act, out=f.out(Mout, n_out, cdt, cols=c_cols), M=M, ln=lnf, **kw)
    return _edge_rows(name, run, ref)


def _geglu_case(M, K, inner, seed=0):
    a = rnd(M, K, seed=seed + 1)
    wfull, bfull = rnd(2 * inner, K, scale=1 / math.sqrt(K), seed=seed + 2), rnd(2 * inner, scale=0.1, seed=seed + 3)
    wp, bp = _geglu_pack(wfull, bfull, inner)
    proj = a.float() @ wfull.float().t() + bfull.float()
    return a, wp, bp, proj[:, :inner] * F.gelu(proj[:, inner:])


def _conv_edge_cases(n, ci, co, H, W, c1=0, what=("s1", "s2", "up", "asym", "two")):
    """(tag, a0, w packed, gemm kwargs, reference tokens) of the small conv geometry: stride 1 + bias + temb + residual, stride 2,
    folded nearest x2 upsample, asymmetric padding (stride 2, pad right / bottom only), two sources."""
    x, w, b = rnd(n, ci, H, W, seed=11), rnd(co, ci, 3, 3, scale=1 / math.sqrt(9 * ci), seed=12), rnd(co, seed=13)
    xt, wp = _to_tokens(x), _pack_conv(w)
    cases = []
    if "s1" in what:
        temb, res = rnd(n, co, seed=14), rnd(n * H * W, co, seed=15)
        ref = F.conv2d(x.float(), w.float(), b.float(), padding=1) + temb.float()[:, :, None, None]
        cases.append(("s1 +bias+temb+res", xt, wp, dict(bias=b, rowvec=temb, rowvec_div=H * W, residual=res, mode=ops.MODE_CONV2D,
                                                        conv=(H, W, H, W, 1, 0)), _to_tokens(ref) + res.float()))
    if "s1res" in what:   # (the persistent families take bias + residual, not temb + residual)
        res = rnd(n * H * W, co, seed=15)
        ref = F.conv2d(x.float(), w.float(), b.float(), padding=1)
        cases.append(("s1 +bias+res", xt, wp, dict(bias=b, residual=res, mode=ops.MODE_CONV2D, conv=(H, W, H, W, 1, 0)),
                      _to_tokens(ref) + res.float()))
    if "s2" in what:
        Ho, Wo = H // 2, W // 2
        cases.append(("stride 2", xt, wp, dict(bias=b, mode=ops.MODE_CONV2D, conv=(H, W, Ho, Wo, 2, 0), M=n * Ho * Wo),
                      _to_tokens(F.conv2d(x.float(), w.float(), b.float(), stride=2, padding=1))))
    if "up" in what:
        ref = F.conv2d(F.interpolate(x.float(), scale_factor=2.0, mode="nearest"), w.float(), b.float(), padding=1)
        cases.append(("upsample x2", xt, wp, dict(bias=b, mode=ops.MODE_CONV2D, conv=(H, W, 2 * H, 2 * W, 1, 1), M=n * 4 * H * W), _to_tokens(ref)))
    if "asym" in what:
        ref = F.conv2d(F.pad(x.float(), (0, 1, 0, 1)), w.float(), b.float(), stride=2)
        Ho, Wo = ref.shape[2:]
        cases.append(("asym pad, stride 2", xt, wp, dict(bias=b, mode=ops.MODE_CONV2D, conv=(H, W, Ho, Wo, 2, 0, 1), M=n * Ho * Wo), _to_tokens(ref)))
    if "two" in what:
        c1 = c1 or 128
        x1 = rnd(n, c1, H, W, seed=16)
        w2 = rnd(co, ci + c1, 3, 3, scale=1 / math.sqrt(9 * (ci + c1)), seed=17)
        ref = F.conv2d(torch.cat([x, x1], 1).float(), w2.float(), padding=1)
        cases.append(("two-source", xt, _pack_conv(w2), dict(a1=_to_tokens(x1), mode=ops.MODE_CONV2D, conv=(H, W, H, W, 1, 0)), _to_tokens(ref)))
    return cases


def _temporal_edge_case(B, Fr, HW, C, co):
    xt = rnd(B * Fr * HW, C, seed=21)
    wt, bt, rt = rnd(co, C, 3, scale=1 / math.sqrt(3 * C), seed=22), rnd(co, seed=23), rnd(B * Fr * HW, co, seed=24)
    ref = F.conv1d(xt.float().view(B, Fr, HW, C).permute(0, 2, 3, 1).reshape(B * HW, C, Fr), wt.float(), bt.float(), padding=1)
    ref = ref.view(B, HW, co, Fr).permute(0, 3, 1, 2).reshape(B * Fr * HW, co) + rt.float()
    return (f"temporal B{B} F{Fr} HW{HW} {C}->{co} +res", xt, wt.permute(0, 2, 1).reshape(co, 3 * C).contiguous(),
            dict(bias=bt, residual=rt, mode=ops.MODE_TEMPORAL, temporal=(Fr, HW)), ref)


def check_edges_gemm_tile(variants=("reg", "glds", "naive")):
    """The 128-row tile kernel (flags bit2 | bit4: no persistent kernel, no split-K), register- and LDS-DMA-staged, and the naive kernel:
    ragged M (1 / 130 / 257 rows), N % 8 = 4 (the narrowest vector epilogue), 128- / 160-column tiles plus 8, one / two K-tiles, with
    bias + rowvec + residual; two sources; GEGLU; fp32 output; one 8-byte-misaligned C view (falls back to the naive kernel)."""
    out = []
    saved, saved_glds = ops.GEMM_FLAGS, ops.USE_GLDS
    try:
        ops.GEMM_FLAGS = saved | 4 | 16
        for var in variants:
            ops.USE_GLDS = var == "glds"
            naive = var == "naive"
            for M in (1, 130, 257):
                for N in (4, 12, 136, 168, 320):
                    for K in (64, 128):
                        a, w = rnd(M, K, seed=M + N + K), rnd(N, K, scale=1 / math.sqrt(K), seed=M + N + K + 1)
                        bias, res, rv = rnd(N, seed=N), rnd(M, N, seed=M + 7 * N), rnd((M + 49) // 50, N, seed=M + 9 * N)
                        out += _gemm_edge(f"edge gemm[{var}] M{M} N{N} K{K} +bias+rowvec+res", a, w, _gemm_ref(a, w, bias, rv, 50, res),
                                          bias=bias, rowvec=rv, rowvec_div=50, residual=res, naive=naive)
            a0, a1, w = rnd(130, 128, seed=1), rnd(130, 64, seed=2), rnd(320, 192, scale=0.1, seed=3)
            out += _gemm_edge(f"edge gemm[{var}] two-source 128 + 64", a0, w, _gemm_ref(torch.cat([a0, a1], 1), w), a1=a1, naive=naive)
            a, wp, bp, ref = _geglu_case(130, 128, 128)
            out += _gemm_edge(f"edge gemm[{var}] GEGLU N256", a, wp, ref, bias=bp, act=ops.ACT_GEGLU, naive=naive)
            a, w, bias = rnd(130, 64, seed=4), rnd(12, 64, scale=0.125, seed=5), rnd(12, seed=6)
            out += _gemm_edge(f"edge gemm[{var}] fp32 out N12", a, w, _gemm_ref(a, w, bias), bias=bias, act=ops.ACT_F32OUT, naive=naive)
        ops.USE_GLDS = True
        a, w, bias, res = rnd(130, 128, seed=7), rnd(136, 128, scale=0.09, seed=8), rnd(136, seed=9), rnd(130, 136, seed=10)
        out += _gemm_edge("edge gemm: C view 8 bytes off a 16-byte boundary (naive fallback)", a, w, _gemm_ref(a, w, bias, residual=res),
                          bias=bias, residual=res, c_cols=12)
    finally:
        ops.GEMM_FLAGS, ops.USE_GLDS = saved, saved_glds
    return out


def check_edges_conv(variants=("reg", "glds", "naive")):
    """Convolutions on the small geometry (3 images of 12 x 10, 64 -> 128 channels) and the temporal conv (2 x 5 frames x 24 px) with
    residual: the taps of the first image's first row and of the last image's last row point at the frame."""
    out = []
    saved, saved_glds = ops.GEMM_FLAGS, ops.USE_GLDS
    try:
        ops.GEMM_FLAGS = saved | 4 | 16
        for var in variants:
            ops.USE_GLDS = var == "glds"
            for (tag, a, w, kw, ref) in _conv_edge_cases(3, 64, 128, 12, 10) + [_temporal_edge_case(2, 5, 24, 64, 64)]:
                out += _gemm_edge(f"edge conv3x3[{var}] {tag}" if "temporal" not in tag else f"edge conv[{var}] {tag}", a, w, ref,
                                  naive=var == "naive", **kw)
    finally:
        ops.GEMM_FLAGS, ops.USE_GLDS = saved, saved_glds
    return out


def _nk(kw, K):
    mode = kw.get("mode", ops.MODE_LINEAR)
    return (1 if mode == ops.MODE_LINEAR else (9 if mode == ops.MODE_CONV2D else 3)) * (K // 64)


def _sw_eligible(N, kw, K):
    """Host mirror of the one-wave-per-SIMD kernel's shape test for the cases below (act none; ld % 8 = 0 by construction)."""
    return N % 320 == 0 and not (kw.get("residual") is not None and kw.get("rowvec") is not None) and _nk(kw, K) >= 2


def _sk_blocks(M, N, kw, K):
    """... and of the forced stream-K form: 0 = the launch has fewer than 8 (tile, K-tile) units and stays on another kernel."""
    units = ((M + 191) // 192) * (N // 320) * _nk(kw, K)
    return (min(units // 4, 256) if units >= 8 else 0) if units < 1024 else 256


PERSISTENT_FAMILIES = (("persistent 192x320", 8), ("ping-pong 192", (1 << 17) | (1 << 19)), ("ping-pong 256", (1 << 17) | (1 << 20)),
                       ("one-wave-per-SIMD", 1 << 21), ("stream-K", 1 << 27))


def _persistent_cases():
    cases = []
    for (M, N, K) in [(197, 320, 128), (261, 320, 128), (197, 640, 192)]:
        a, w = rnd(M, K, seed=M + N), rnd(N, K, scale=1 / math.sqrt(K), seed=M + N + 1)
        bias, res = rnd(N, seed=N + 2), rnd(M, N, seed=M + 3)
        cases.append((f"M{M} N{N} K{K} +bias+res", a, w, dict(bias=bias, residual=res), _gemm_ref(a, w, bias, residual=res)))
    cases += _conv_edge_cases(3, 64, 320, 16, 16, what=("s1res",))
    cases.append(_temporal_edge_case(2, 5, 24, 64, 320))
    return cases


def check_edges_gemm_persistent():
    """The persistent 192 x 320 kernel (flags bit3), the ping-pong kernel (bit17 with bit19 / bit20), the one-wave-per-SIMD kernel (bit21) and
    its stream-K form (bit27) at row counts that are not multiples of their tiles; the stream-K rows run with the workspace NaN-filled
    and zero-filled (bit-equal: no partial tile is summed from a slot the launch did not write).  A case a kernel is not eligible for
    is skipped by name."""
    out = []
    saved, saved_glds = ops.GEMM_FLAGS, ops.USE_GLDS
    try:
        ops.USE_GLDS = True
        for fam, bits in PERSISTENT_FAMILIES:
            ops.GEMM_FLAGS = (saved & ~4) | bits
            for (tag, a, w, kw, ref) in _persistent_cases():
                name = f"edge gemm[{fam}] {tag}"
                M, N, K = kw.get("M", a.shape[0]), w.shape[0], a.shape[1]
                if bits in (1 << 21, 1 << 27) and not _sw_eligible(N, kw, K):
                    out.append(_skip_row(name, "shape not eligible for the one-wave-per-SIMD kernel"))
                    continue
                if bits == 1 << 27:
                    if _sk_blocks(M, N, kw, K) == 0:
                        out.append(_skip_row(name, "fewer than 8 (tile, K-tile) units: no stream-K form"))
                        continue
                    out += _workspace_rows(name, a, w, ref, kw)
                else:
                    out += _gemm_edge(name, a, w, ref, **kw)
    finally:
        ops.GEMM_FLAGS, ops.USE_GLDS = saved, saved_glds
    return out


def _workspace_rows(name, a, w, ref, kw):
    """Edge rows of a launch that sums fp32 partial tiles from ``ops._workspace``: the scratch NaN-filled, then zero-filled (a launch may
    only read slots it wrote itself, so the two results are bit-equal).  The workspace is scratch: nothing is restored."""
    ws = ops._workspace(DEV)
    ws.fill_(float("nan"))
    rows = _gemm_edge(name + " [workspace NaN-filled]", a, w, ref, **kw)
    ws.fill_(float("nan"))
    y_nan = ops.gemm(a, w, **kw)
    ws.zero_()
    y_zero = ops.gemm(a, w, **kw)
    torch.cuda.synchronize()
    same = bool(torch.equal(y_nan, y_zero))
    rows.append(dict(name=name + ": NaN-filled workspace == zero-filled workspace, bit for bit", err=0.0 if same else 1.0, tol=0.0, ok=same))
    rows += [r for r in _gemm_edge(name + " [workspace zero-filled]", a, w, ref, **kw)]
    return rows


def check_edges_splitk():
    """The two 8x8-level conv cases of ``check_gemm_splitk`` (M = 3072: split-K on the 128-row kernel and on the persistent kernel) with
    every operand framed and the fp32 workspace NaN- / zero-filled."""
    out = []
    saved_glds = ops.USE_GLDS
    try:
        ops.USE_GLDS = True
        H = W = 8
        for (n, ci, co, tag) in [(48, 256, 320, "split-K"), (48, 640, 1280, "persistent split-K")]:
            x, w, b = rnd(n, ci, H, W), rnd(co, ci, 3, 3, scale=1 / math.sqrt(9 * ci)), rnd(co)
            temb, res = rnd(3, co), rnd(n * H * W, co)
            kw = dict(bias=b, rowvec=temb, rowvec_div=16 * H * W, residual=res, mode=ops.MODE_CONV2D, conv=(H, W, H, W, 1, 0))
            ref = F.conv2d(x.float(), w.float(), b.float(), padding=1) + temb.float().repeat_interleave(16, 0)[:, :, None, None]
            out += _workspace_rows(f"edge conv3x3[{tag}] {ci}->{co} @8x8 M3072", _to_tokens(x), _pack_conv(w), _to_tokens(ref) + res.float(), kw)
    finally:
        ops.USE_GLDS = saved_glds
    return out


def check_edges_conv_lds_patch():
    """The LDS-patch 3x3 convolution (flags bit28) at row counts that are not multiples of its 192-row tile: the patch rows above the
    first image and below the last one come from the frame."""
    out = []
    saved, saved_glds = ops.GEMM_FLAGS, ops.USE_GLDS
    try:
        ops.USE_GLDS = True
        ops.GEMM_FLAGS = saved | (1 << 28)
        for (n, H) in [(1, 16), (3, 16), (1, 32)]:
            for (tag, a, w, kw, ref) in _conv_edge_cases(n, 64, 320, H, H, what=("s1res",)):
                out += _gemm_edge(f"edge conv3x3[LDS patch] {n} x {H}x{H} 64->320 {tag}", a, w, ref, **kw)
        out.append(_skip_row("edge conv[LDS patch] temporal", "the LDS-patch kernel takes 3x3 stride-1 convolutions only"))
    finally:
        ops.GEMM_FLAGS, ops.USE_GLDS = saved, saved_glds
    return out


def check_edges_gemm_ws():
    """The weight-stationary kernel (flags bit10): ragged strips (row guards, clamped look-ahead), K = 320 and 512, residual, GEGLU, and
    the LayerNorm fold with ``ln_c1`` framed."""
    out = []
    saved, saved_glds = ops.GEMM_FLAGS, ops.USE_GLDS
    try:
        ops.USE_GLDS = True
        ops.GEMM_FLAGS = saved | 1024
        for (M, N, K, res) in [(100, 160, 320, False), (2049, 320, 320, True), (100, 64, 512, False), (100, 512, 512, True)]:
            name = f"edge gemm[ws] M{M} N{N} K{K} res={res}"
            if K == 512 and N != 512:
                out.append(_skip_row(name, "at K = 512 the weight-stationary kernel takes N = 512 (or GEGLU) only"))
                continue
            a, w, bias = rnd(M, K, seed=M), rnd(N, K, scale=1 / math.sqrt(K), seed=N), rnd(N, seed=K)
            r = rnd(M, N, seed=M + N) if res else None
            out += _gemm_edge(name, a, w, _gemm_ref(a, w, bias, residual=r), bias=bias, residual=r)
        a, wp, bp, ref = _geglu_case(777, 320, 160)
        out += _gemm_edge("edge gemm[ws] GEGLU M777 inner160", a, wp, ref, bias=bp, act=ops.ACT_GEGLU)
        M, K, N, eps = 100, 320, 160, 1e-5
        x = (rnd(M, K, seed=31).float() * 1.5 + 2.0).half()
        gamma, beta = (1.0 + 0.3 * rnd(K, seed=32).float()).half(), (0.2 * rnd(K, seed=33).float()).half()
        w, b = rnd(N, K, scale=1 / math.sqrt(K), seed=34), rnd(N, scale=0.1, seed=35)
        ref = F.layer_norm(x.float(), (K,), gamma.float(), beta.float(), eps) @ w.float().t() + b.float()
        wq, bq, c1 = ops.ln_fold(w, b, gamma, beta)
        out += _gemm_edge("edge gemm[ws+LN] M100 K320 N160", x, wq, ref, bias=bq, ln=(c1, eps))
    finally:
        ops.GEMM_FLAGS, ops.USE_GLDS = saved, saved_glds
    return out


def check_edges_ff_fused():
    """The fused feed-forward kernel with X, W1, b1, W2, b2, R and Y framed: one strip and a ragged tail."""
    out = []
    C, H = 320, 1280
    w1, b1 = rnd(2 * H, C, scale=1 / math.sqrt(C)), rnd(2 * H, scale=0.1)
    w2, b2 = rnd(C, H, scale=1 / math.sqrt(H)), rnd(C, scale=0.1)
    w1p, b1p = _geglu_pack(w1, b1, H)
    w2s = ops.ff_pack_w2(w2)
    for M in (32, 167):
        x, r = rnd(M, C, seed=M), rnd(M, C, seed=M + 1)
        proj = x.float() @ w1.float().t() + b1.float()
        hid = (proj[:, :H] * F.gelu(proj[:, H:])).half().float()
        ref = (hid @ w2.float().t() + b2.float()).half().float() + r.float()

        def run(f):
            return ops.ff_geglu(f.inp(x), f.inp(w1p, flat=True), f.inp(b1p), f.inp(w2s, flat=True), f.inp(b2), residual=f.inp(r),
                                out=f.out(M, C))
        out += _edge_rows(f"edge ff_fused M{M} +res", run, ref)
    return out


# ---- attention
def _attn_rows_of(batch, S, inner, strides):
    outer, inner_s, seq = strides
    i = torch.arange(batch, device=DEV)
    return ((i // inner) * outer + (i % inner) * inner_s)[:, None] + torch.arange(S, device=DEV)[None] * seq   # [batch, S]


def _attn_ref(q2, k2, v2, *, batch, heads, Sq, Sk, inner, q_strides, kv_strides, kv_div=1, qk_mod=0, d=64, scale=None, causal=False,
              bias=None, only=None):
    """fp32 attention on token matrices with the entry point's addressing (include/anyv2v_hip.h): ``(rows, ref)`` -- the output rows
    of the batch elements ``only`` (default: all) and their [len(rows), heads * d] reference."""
    C = heads * d
    i = torch.arange(batch, device=DEV) if only is None else torch.tensor(only, device=DEV)
    iq = i % qk_mod if qk_mod else i
    rq, ro = _attn_rows_of(batch, Sq, inner, q_strides), _attn_rows_of(batch, Sq, inner, q_strides)
    rkv = _attn_rows_of(batch, Sk, inner, kv_strides)
    sp = lambda x, rows, S: x[rows.reshape(-1)].float().view(len(i), S, heads, d).transpose(1, 2)
    q, k, v = sp(q2, rq[iq], Sq), sp(k2, rkv[iq // kv_div], Sk), sp(v2, rkv[i // kv_div], Sk)
    scale = d ** -0.5 if scale is None else scale
    if bias is not None:
        ref = F.scaled_dot_product_attention(q, k, v, attn_mask=bias[None].float(), scale=scale)
    else:
        ref = F.scaled_dot_product_attention(q, k, v, is_causal=causal, scale=scale)
    return ro[i].reshape(-1), ref.transpose(1, 2).reshape(-1, C)


def _attn_operand(f, t):
    """A Q / K / V source matrix for the launch: plain, or inside a buffer with 16 more (poisoned) columns and poisoned frame rows."""
    if not f.framed:
        return t
    M, Wd = t.shape
    buf = torch.full((M + 128, Wd + 16), POISON16, dtype=torch.int16, device=t.device)
    view = buf.view(torch.float16)[64:64 + M, :Wd]
    view.copy_(t)
    return view


def attn_plan_words(q, k, v, o, *, batch, heads, Sq, Sk, inner=1, q_strides, kv_strides, kv_div=1, qk_mod=0, scale=0.125, head_dim=64,
                    naive=False, causal=False, bias=None, flags=0):
    """The launch ``ops.attention(q, k, v, o, ...)`` makes, as a line for tests/attention_plan_main.cpp: the entry point, the leading
    dimensions and the operands' addresses modulo 16 (their offset in an allocation, which starts 16-byte aligned), read from the tensors
    themselves -- on any device, "meta" included.  ``bias``: anything but None / False stands for a bias tensor."""
    res = lambda t: (t.storage_offset() * t.element_size()) % 16
    for t in (q, k, v, o):
        assert t.dim() == 2 and t.stride(1) == 1
    has_bias = bias is not None and bias is not False
    fl = (1 if (naive or ops.FORCE_NAIVE) else 0) | ops.ATTN_FLAGS | flags | (16 if causal else 0)
    return (f"entry={ops.attention_entry(head_dim, causal, has_bias)} head_dim={head_dim} bias={int(has_bias)} batch={batch} heads={heads} Sq={Sq} Sk={Sk} "
            f"inner={inner} q_outer={q_strides[0]} q_inner={q_strides[1]} q_seq={q_strides[2]} kv_outer={kv_strides[0]} kv_inner={kv_strides[1]} "
            f"kv_seq={kv_strides[2]} kv_div={kv_div} qk_mod={qk_mod} scale_milli={max(1, round(scale * 1000))} flags={fl} "
            f"ldq={q.stride(0)} ldk={k.stride(0)} ldv={v.stride(0)} ldo={o.stride(0)} Q={res(q)} K={res(k)} V={res(v)} O={res(o)}")


# What the planner (anyv2v_amd/csrc/attention_plan.cpp: av_attn_kernel_name) may answer for a launch that a check names by kernel:
# tests/test_attention_plan_host.py plans every named launch of this file and fails when a name and a plan disagree.
ATTN_KERNEL_INSTANTIATIONS = {
    "4-wave flash": ("flash<2,1,4>",), "short one-wave": ("short<1>", "short<3>"), "short one-wave PnP": ("short<3>",),
    "shared-softmax 4-wave": ("flash<2,3,4>",), "8-wave": ("flash<3,1,8>", "flash<3,3,8>"), "shared-softmax 8-wave": ("flash<3,3,8>",),
    "whole-sequence MFMA": ("small<2,6>", "small<3,6>", "small<4,6>", "small<5,6>", "small<2,18>", "small<3,18>", "small<4,18>"),
    "96-key loop": ("loop<2>", "loop<3>", "loop<4>", "loop<5>"),
    "bias": ("small<2,6,bias>", "small<3,6,bias>", "small<4,6,bias>", "small<5,6,bias>", "naive+bias"), "generic": ("naive",),
    "64-bit fallback": ("loop<2>",),
}


def _ae(name, kernel, instantiation, *, batch, heads, Sq, Sk, d=64, inner=1, q_strides=None, kv_strides=None, kv_div=1, qk_mod=0, causal=False,
        bias=None, naive=False, seed=0, flags=0, tol=KTOL):
    """One attention edge case: ``kernel`` as the row's tag names it, ``instantiation`` as the planner names it; ``bias`` = the seed of a bias."""
    return dict(name=name, kernel=kernel, instantiation=instantiation, batch=batch, heads=heads, Sq=Sq, Sk=Sk, d=d, inner=inner,
                q_strides=(Sq, 0, 1) if q_strides is None else q_strides, kv_strides=(Sk, 0, 1) if kv_strides is None else kv_strides,
                kv_div=kv_div, qk_mod=qk_mod, causal=causal, bias=bias, naive=naive, seed=seed, flags=flags, tol=tol)


def _attn_edge_kw(spec):
    kw = {key: spec[key] for key in ("batch", "heads", "Sq", "Sk", "inner", "q_strides", "kv_strides", "kv_div", "qk_mod")}
    d, causal = spec["d"], spec["causal"]
    extra = {} if d == 64 and not causal and spec["bias"] is None else dict(scale=d ** -0.5, head_dim=d, causal=causal)
    return kw, extra


def _attn_edge_sources(spec, device=None):
    """The source matrices of an edge case.  Self-attention shapes read Q / K / V from one fused matrix [rows, 3 C]; the others Q from
    [rows, C] and K / V from [kv rows, 2 C].  -> (Mq, mats, windows): ``windows(f)`` = the (q, k, v) column windows of the matrices as the
    operands ``f`` hold them.  On the device "meta" the matrices carry no data, the windows the same layout."""
    C = spec["heads"] * spec["d"]
    Mq = int(_xa_rows(spec["batch"], spec["Sq"], spec["inner"], spec["q_strides"]).max()) + 1
    Mk = int(_xa_rows((spec["batch"] + spec["kv_div"] - 1) // spec["kv_div"], spec["Sk"], spec["inner"], spec["kv_strides"]).max()) + 1
    seed = spec["seed"]
    mat = lambda M, W, sd: rnd(M, W, seed=sd) if device is None else torch.empty(M, W, dtype=torch.float16, device=device)
    if Mq == Mk and spec["kv_div"] == 1 and spec["q_strides"] == spec["kv_strides"]:
        mats = (mat(Mq, 3 * C, seed + 1),)
        windows = lambda f: (lambda t: (t[:, :C], t[:, C:2 * C], t[:, 2 * C:]))(_attn_operand(f, mats[0]))
    else:
        mats = (mat(Mq, C, seed + 1), mat(Mk, 2 * C, seed + 2))
        windows = lambda f: (lambda a, b: (a, b[:, :C], b[:, C:]))(_attn_operand(f, mats[0]), _attn_operand(f, mats[1]))
    return Mq, mats, windows


def _attn_edge_bias(spec):
    if spec["bias"] is None:
        return None
    return torch.randn(spec["heads"], spec["Sq"], spec["Sk"], generator=torch.Generator().manual_seed(spec["bias"])).to(DEV)


def _attn_edge(spec):
    """One attention edge case (``_ae``).  O is a framed [rows, C] window (8 guard columns each side, guard rows)."""
    C = spec["heads"] * spec["d"]
    Mq, mats, windows = _attn_edge_sources(spec)
    q2, k2, v2 = windows(_PlainOperands())
    kw, extra = _attn_edge_kw(spec)
    bias = _attn_edge_bias(spec)
    rows, ref = _attn_ref(q2, k2, v2, d=spec["d"], causal=spec["causal"], bias=bias, **kw)
    want = torch.zeros(Mq, C, device=DEV)
    want[rows] = ref

    def run(f):
        q, k, v = windows(f)
        o = f.out(Mq, C, init=torch.zeros(Mq, C, dtype=torch.float16, device=DEV))
        saved, ops.ATTN_FLAGS = ops.ATTN_FLAGS, ops.ATTN_FLAGS | spec["flags"]
        try:
            return ops.attention(q, k, v, o, naive=spec["naive"], bias=None if bias is None else f.inp(bias, flat=True), **kw, **extra)
        finally:
            ops.ATTN_FLAGS = saved
    return _edge_rows(spec["name"], run, want, spec["tol"])


def attention_edge_specs():
    """The cases of ``check_edges_attention`` / ``check_edges_attention_8wave`` / ``check_edges_attention_small``, in their order:
    -> dict(flash=[...], wave8=[...], small=[...]) of ``_ae`` specs."""
    E = dict(flash=[], wave8=[], small=[])
    for (b, h, Sq, Sk) in [(2, 2, 130, 145), (2, 1, 20, 3), (1, 1, 33, 63)]:
        E["flash"].append(_ae(f"edge attn[flash] b{b} h{h} Sq{Sq} Sk{Sk}", "4-wave flash", "flash<2,1,4>", batch=b, heads=h, Sq=Sq, Sk=Sk, seed=Sq))
    E["flash"].append(_ae("edge attn[flash] b4 h1 Sq256 Sk145 kv_div2", "4-wave flash", "flash<2,1,4>", batch=4, heads=1, Sq=256, Sk=145, kv_div=2, seed=5))
    for flag in (0, 8):
        E["flash"].append(_ae("edge attn PnP b3 h1 S130 " + ("shared-softmax kernel" if not flag else "aliasing form (flag bit3)"),
                              "shared-softmax 4-wave" if not flag else "4-wave flash", "flash<2,3,4>" if not flag else "flash<2,1,4>",
                              batch=3, heads=1, Sq=130, Sk=130, qk_mod=1, seed=6, flags=flag))
    B_, HW, h = 3, 20, 2
    for Fr in (8, 16, 40):
        for inj in (False, True):
            st = (Fr * HW, 1, HW)
            kernel, inst = ("short one-wave", "short<3>" if inj else "short<1>") if Fr <= 16 else \
                (("shared-softmax 4-wave", "flash<2,3,4>") if inj else ("4-wave flash", "flash<2,1,4>"))
            E["flash"].append(_ae(f"edge attn temporal F{Fr} inject={inj}", kernel, inst, batch=B_ * HW, heads=h, Sq=Fr, Sk=Fr, inner=HW, q_strides=st,
                                  kv_strides=st, qk_mod=HW if inj else 0, seed=Fr))
    # 8-wave (256-query) blocks: b29 h4 S2100 gives 1044 blocks; the shared-softmax form needs qk_mod x heads x 9 >= 1024 of them
    E["wave8"].append(_ae("edge attn[flash, 8-wave blocks] b29 h4 S2100", "8-wave", "flash<3,1,8>", batch=29, heads=4, Sq=2100, Sk=2100, seed=2099))
    E["wave8"].append(_ae("edge attn[shared softmax, 8-wave blocks] b87 h4 S2100 qk_mod29", "shared-softmax 8-wave", "flash<3,3,8>", batch=87, heads=4,
                          Sq=2100, Sk=2100, qk_mod=29, seed=2199))
    sm = lambda tag, kernel, inst, B, h, S, d, causal: _ae(f"edge attention[{tag}] B{B} h{h} S{S} d{d} causal={causal}", kernel, inst, batch=B, heads=h, Sq=S,
                                                           Sk=S, d=d, causal=causal, seed=S + d)
    W, L = "whole-sequence MFMA", "96-key loop"
    for (B, h, S, d, causal, inst) in [(3, 8, 24, 40, False, "small<2,6>"), (3, 16, 77, 64, True, "small<2,6>"), (2, 4, 90, 56, False, "small<2,6>"),
                                       (2, 8, 77, 160, False, "small<5,6>"),
                                       # every other instantiation, at the smallest ragged shapes and on both edges of the 96 / 288-key thresholds
                                       (2, 2, 50, 80, False, "small<3,6>"), (2, 2, 90, 128, True, "small<4,6>"), (2, 2, 97, 56, False, "small<2,18>"),
                                       (2, 3, 257, 80, False, "small<3,18>"), (2, 2, 288, 104, False, "small<4,18>")]:
        E["small"].append(sm("small mfma", W, inst, B, h, S, d, causal))
    for (B, h, S, d, causal, inst) in [(2, 3, 289, 24, False, "loop<2>"), (1, 2, 401, 56, True, "loop<2>"),
                                       (1, 2, 289, 72, False, "loop<3>"), (1, 2, 289, 128, True, "loop<4>"), (2, 2, 97, 160, False, "loop<5>")]:
        E["small"].append(sm("small loop", L, inst, B, h, S, d, causal))
    # head_dim 24 up to 288 keys: neither MFMA kernel (one 32-column group) -> one thread per query
    E["small"].append(_ae("edge attention one thread per query, B2 h3 S288 d24", "generic", "naive", batch=2, heads=3, Sq=288, Sk=288, d=24, seed=312))
    for (B, h, Sq, Sk, d, inst) in [(2, 3, 20, 24, 40, "small<2,6,bias>"), (2, 2, 33, 130, 40, "naive+bias"),
                                    # the MFMA form at exactly 96 keys on every instantiation, the generic kernel one key later
                                    (2, 2, 100, 96, 40, "small<2,6,bias>"), (2, 2, 100, 96, 80, "small<3,6,bias>"), (2, 2, 100, 96, 128, "small<4,6,bias>"),
                                    (2, 2, 100, 96, 160, "small<5,6,bias>"), (2, 2, 100, 97, 40, "naive+bias")]:
        E["small"].append(_ae(f"edge attention + score bias B{B} h{h} Sq{Sq} Sk{Sk} d{d}", "bias", inst, batch=B, heads=h, Sq=Sq, Sk=Sk, d=d, bias=Sk,
                              seed=Sk))
    B_, Fr, HW, h, d = 2, 6, 10, 2, 4
    st = (Fr * HW, 1, HW)
    E["small"].append(_ae("edge attention one thread per query, head_dim 4 (temporal layout)", "generic", "naive", batch=B_ * HW, heads=h, Sq=Fr, Sk=Fr,
                          d=d, inner=HW, q_strides=st, kv_strides=st, seed=4))
    return E


def attention_edge_plan_rows():
    """(row name, line for tests/attention_plan_main.cpp, kernel named, instantiation named) of every launch of the attention edge checks:
    the plain and the framed launch of each case (and the 8-wave cases' flag-bit2 twin), from the layout code of the launches."""
    rows = []
    for group, specs in attention_edge_specs().items():
        for spec in specs:
            Mq, _mats, windows = _attn_edge_sources(spec, device="meta")
            kw, extra = _attn_edge_kw(spec)
            for f in (_PlainOperands("meta"), _FramedOperands("meta")):
                q, k, v = windows(f)
                o = f.out(Mq, spec["heads"] * spec["d"])
                words = lambda fl: attn_plan_words(q, k, v, o, naive=spec["naive"], bias=spec["bias"], flags=fl, **kw, **extra)
                tag = f"{spec['name']} | {'framed' if f.framed else 'plain'}"
                rows.append((tag, words(spec["flags"]), spec["kernel"], spec["instantiation"]))
                if group == "wave8" and f.framed:
                    four = {"flash<3,1,8>": ("4-wave flash", "flash<2,1,4>"), "flash<3,3,8>": ("shared-softmax 4-wave", "flash<2,3,4>")}[spec["instantiation"]]
                    rows.append((tag + " | flag bit2", words(spec["flags"] | 4)) + four)
    return rows


def check_edges_attention():
    """The flash kernel (4-wave blocks): ragged query blocks and key tails, whole masked steps, shared K / V (kv_div), the PnP
    shared-softmax kernel and its aliasing form (flag bit3), the temporal layout through the short one-wave kernel (F <= 16) and the
    flash kernel (F = 40)."""
    out = []
    for spec in attention_edge_specs()["flash"]:
        out += _attn_edge(spec)
    return out


def check_edges_attention_8wave():
    """8-wave (256-query) blocks of the flash kernel, plain and shared-softmax (three V / O streams): b29 h4 S2100 gives 1044 blocks, a
    ragged last block (52 queries) and a ragged last key tile.  Framed against plain (bit-equal), framed against the 4-wave form (flag
    bit2, 1e-6), fp32 SDPA on two batch elements (every head)."""
    out = []
    for spec in attention_edge_specs()["wave8"]:
        b, h, S = spec["batch"], spec["heads"], spec["Sq"]
        C = 64 * h
        Mq, mats, windows = _attn_edge_sources(spec)
        kw, extra = _attn_edge_kw(spec)
        name = spec["name"]

        def launch(f):
            q, k, v = windows(f)
            return ops.attention(q, k, v, f.out(b * S, C), **kw, **extra)
        yp = launch(_PlainOperands())
        fr = _FramedOperands()
        yf = launch(fr)
        saved, ops.ATTN_FLAGS = ops.ATTN_FLAGS, ops.ATTN_FLAGS | 4
        try:
            y4 = launch(_FramedOperands())
        finally:
            ops.ATTN_FLAGS = saved
        torch.cuda.synchronize()
        q2, k2, v2 = windows(_PlainOperands())
        for i in (0, b - 1):
            rows, ref = _attn_ref(q2, k2, v2, only=[i], **kw)
            out.append(_res(f"{name}: framed, element {i} vs fp32 SDPA", yf[rows], ref, KTOL))
        out.append(_res(f"{name}: framed == 4-wave blocks (flag bit2), framed", yf, y4.float(), 1e-6))
        same, intact = bool(torch.equal(yf, yp)), fr.intact()
        out.append(dict(name=f"{name}: framed == plain, bit for bit", err=0.0 if same else 1.0, tol=0.0, ok=same))
        out.append(dict(name=f"{name}: frames of the outputs intact", err=0.0 if intact else 1.0, tol=0.0, ok=intact))
        del yp, yf, y4, fr, mats, windows, q2, k2, v2
    return out


def check_edges_attention_small():
    """``anyv2v_attention_small_f16``: every instantiation of the whole-sequence MFMA kernel and of the 96-key loop kernel, the
    one-thread-per-query kernel (head_dim 4; head_dim 24 at 288 keys), and the bias entry point on every MFMA instantiation (Sk <= 96)
    and on the generic kernel (Sk = 97, 130) with the fp32 bias framed."""
    out = []
    for spec in attention_edge_specs()["small"]:
        out += _attn_edge(spec)
    return out


# ---- elementwise, layout and step kernels
GRID_CAP_N = 4096 * 256 + 12345   # past the 4096-block x 256-thread grid cap of silu / add / ddim_step / guided_step: the grid-stride loop iterates
EDGE_NS = (GRID_CAP_N, 1, 7, 8, 9)


def _h(x):   # one fp16 rounding point of a kernel that computes in fp32
    return x.half().float()


def _guided_ref(e, x, coef, b_txt, b_unc, b_img, g_txt, g_img, pred, noise=None, sigma=0.0):
    """The guided step with the kernel's documented rounding points: every guidance operation in fp32 rounded to fp16, the step itself
    exact (float64)."""
    n = x.numel()
    E = e.reshape(-1, n).float()
    ee = E[b_txt]
    if b_unc >= 0:
        eu = E[b_unc]
        if b_img >= 0:
            ei = E[b_img]
            ee = _h(_h(eu + _h(g_img * _h(ei - eu))) + _h(g_txt * _h(ee - ei)))
        else:
            ee = _h(eu + _h(g_txt * _h(ee - eu)))
    sa_t, sb_t, c0, c1 = (float(torch.tensor(c, dtype=torch.float32)) for c in coef)
    ee, xx = ee.double(), x.reshape(-1).double()
    if pred == 0:
        x0, eps = sa_t * xx - sb_t * ee, sa_t * ee + sb_t * xx
    elif pred == 1:
        x0, eps = (xx - sb_t * ee) / sa_t, ee
    else:
        x0, eps = ee, (xx - sa_t * ee) / sb_t
    y = c0 * x0 + c1 * eps
    if noise is not None:
        y = y + float(torch.tensor(sigma, dtype=torch.float32)) * noise.reshape(-1).double()
    return y


GUIDANCE_FORMS = (("no guidance", dict(b_txt=1)), ("text only", dict(b_unc=0, b_txt=2, g_txt=7.5)),
                  ("image + text", dict(b_unc=2, b_img=0, b_txt=1, g_txt=7.5, g_img=1.5)))


def check_edges_elementwise():
    """silu / add / ddim_step / guided_step past the grid cap (the grid-stride loop iterates) and at 1 / 7 / 8 / 9 elements; add on operands
    2 bytes off alignment (scalar path); every guidance form x prediction type of guided_step, Y aliasing X, the noise entry point."""
    out = []
    coef = (0.8, 0.6, 0.9, math.sqrt(1 - 0.81))
    for n in EDGE_NS:
        x, y2 = rnd(n, scale=2.0, seed=n % 1000 + 1), rnd(n, seed=n % 1000 + 2)
        out += _edge_rows(f"edge silu n{n}", lambda f: ops.silu(f.inp(x), out=f.out_flat((n,))), F.silu(x.double()), 2e-3)
        out += _edge_rows(f"edge add n{n}", lambda f: ops.add(f.inp(x), f.inp(y2), out=f.out_flat((n,))), x.double() + y2.double(), 2e-3)
        sa, sb, pa, pb = coef
        ref = pa * (sa * y2.double() - sb * x.double()) + pb * (sa * x.double() + sb * y2.double())
        out += _edge_rows(f"edge ddim_step n{n}", lambda f: ops.ddim_step(f.inp(x), f.inp(y2), sa, sb, pa, pb, out=f.out_flat((n,))), ref, 3e-3)
        e = rnd(3, n, seed=n % 1000 + 3)
        gk = GUIDANCE_FORMS[2][1]
        refg = _guided_ref(e, y2, coef, gk["b_txt"], gk["b_unc"], gk["b_img"], gk["g_txt"], gk["g_img"], 0)
        out += _edge_rows(f"edge guided_step n{n} image + text, v-prediction",
                          lambda f: ops.guided_step(f.inp(e, flat=True), f.inp(y2), coef, out=f.out_flat((n,)), **gk), refg, KTOL)
    # add: every operand 2 bytes past a 16-byte boundary -> the alignment test picks the scalar path
    n = 1000
    a, b = rnd(n + 1, seed=71), rnd(n + 1, seed=72)

    def run_add(f):
        o = f.out_flat((n + 1,))
        ops.add(f.inp(a)[1:], f.inp(b)[1:], out=o[1:])
        return o[1:]
    out += _edge_rows("edge add, operands 2 bytes off a 16-byte boundary (scalar path)", run_add, a[1:].double() + b[1:].double(), 2e-3)
    n = 777
    e, x = rnd(3, n, seed=81), rnd(n, seed=82)
    nz = rnd(n, seed=83)
    for form, gk in GUIDANCE_FORMS:
        for pred in (0, 1, 2):
            args = (gk["b_txt"], gk.get("b_unc", -1), gk.get("b_img", -1), gk.get("g_txt", 1.0), gk.get("g_img", 1.0), pred)
            out += _edge_rows(f"edge guided_step {form}, prediction {pred}",
                              lambda f: ops.guided_step(f.inp(e, flat=True), f.inp(x), coef, prediction=pred, out=f.out_flat((n,)), **gk),
                              _guided_ref(e, x, coef, *args), KTOL)
            out += _edge_rows(f"edge guided_step {form}, prediction {pred}, Y aliasing X",
                              lambda f: (lambda xx: ops.guided_step(f.inp(e, flat=True), xx, coef, prediction=pred, out=xx, **gk))(f.inout(x)),
                              _guided_ref(e, x, coef, *args), KTOL)
            for sigma, tag in ((0.0, "sigma 0"), (0.3, "sigma 0.3")):
                out += _edge_rows(f"edge guided_step_noise {form}, prediction {pred}, {tag}",
                                  lambda f: ops.guided_step(f.inp(e, flat=True), f.inp(x), coef, prediction=pred, out=f.out_flat((n,)),
                                                            noise=f.inp(nz), sigma=sigma, **gk),
                                  _guided_ref(e, x, coef, *args, noise=nz, sigma=sigma), KTOL)
    # fused CFG + DDIM step without CFG (b_unc < 0), the v tokens a 4-column window of a wider matrix (ldv > C)
    Fr, H, W = 3, 4, 5
    vt, latx = rnd(3 * Fr * H * W, 4, seed=91), rnd(1, 4, Fr, H, W, seed=92)
    cf = torch.tensor(coef, dtype=torch.float32, device=DEV)
    v = vt.double().view(3, Fr, H * W, 4).permute(0, 3, 1, 2).reshape(3, 4, Fr, H, W)[1]
    c = [float(t) for t in cf]
    xx = latx.double()[0]
    ref = c[2] * (c[0] * xx - c[1] * v) + c[3] * (c[0] * v + c[1] * xx)
    out += _edge_rows("edge cfg_ddim_step without CFG (b_unc < 0), ldv > C",
                      lambda f: ops.cfg_ddim_step(f.inp(vt), -1, 1, 9.0, f.inp(cf), f.inp(latx), f.out_flat(tuple(latx.shape)))[0], ref, KTOL)
    return out


def _window_rows(name, run, window, want, exact=True, tol=0.0):
    """Edge rows of a kernel that writes a column window of a wider destination: ``run(f)`` returns (destination, its prefill); the
    window must equal ``want`` and every other column of the destination its prefill, on top of the three usual rows."""
    rows = []
    res = {}

    def run2(f):
        y, pre = run(f)
        res[f.framed] = (y, pre)
        return y
    rows += _edge_rows(name, run2, lambda yf: torch.cat([res[True][1][:, :window[0]].float(), want.float().to(DEV), res[True][1][:, window[1]:].float()], 1), tol)
    y, pre = res[True]
    keep = bool(torch.equal(y[:, :window[0]], pre[:, :window[0]]) and torch.equal(y[:, window[1]:], pre[:, window[1]:]))
    rows.append(dict(name=name + ": columns outside the destination window unchanged", err=0.0 if keep else 1.0, tol=0.0, ok=keep))
    return rows


def check_edges_layout():
    """copy_cols / gather_rows past their grid caps and on odd windows, the NCFHW <-> token layouts on a column window of a framed token
    matrix, adaptive_avgpool with non-divisible sizes."""
    out = []
    M = 8192 * 256 // 320 + 77
    for (xc, yc, C) in [(0, 0, 1), (3, 5, 13), (320, 640, 320)]:
        x, pre = rnd(M, xc + C + 3, seed=C), rnd(M, yc + C + 5, seed=C + 1)
        out += _window_rows(f"edge copy_cols M{M} x[:, {xc}:{xc + C}] -> y[:, {yc}:{yc + C}]",
                            lambda f: (ops.copy_cols(f.inp(x), xc, f.out(M, pre.shape[1], init=pre), yc, C), pre), (yc, yc + C), x[:, xc:xc + C])
    Mg = 8192 * 256 + 77                      # one 16-byte chunk per row: past the 8192-block cap
    src = rnd(300, 16, seed=7)
    idx = torch.randint(0, 300, (Mg,), generator=torch.Generator().manual_seed(8)).to(torch.int32)
    idx[:4] = torch.tensor([0, 299, 299, 0])
    idx[-3:] = torch.tensor([299, 0, 0])
    idx = idx.to(DEV)
    pre = torch.zeros(Mg, 16, dtype=torch.float16, device=DEV)
    out += _window_rows(f"edge gather_rows M{Mg} (repeated indices, first / last source row)",
                        lambda f: (ops.gather_rows(f.inp(src), 8, idx, f.out(Mg, 16, init=pre), 8, 8), pre), (8, 16), src[idx.long(), 8:16])
    B, Fr, H, W = 2, 3, 5, 6
    for C in (4, 9):
        lat = rnd(B, C, Fr, H, W, seed=C)
        pre = rnd(B * Fr * H * W, 16, seed=C + 1)
        tok_ref = lat.permute(0, 2, 3, 4, 1).reshape(-1, C)
        out += _window_rows(f"edge ncfhw_to_tokens C{C} -> tokens[:, 4:{4 + C}]",
                            lambda f: (ops.ncfhw_to_tokens(f.inp(lat), f.out(pre.shape[0], 16, init=pre), col0=4), pre), (4, 4 + C), tok_ref)
        tok = pre.clone()
        tok[:, 4:4 + C] = tok_ref
        out += _edge_rows(f"edge tokens_to_ncfhw C{C} <- tokens[:, 4:{4 + C}]",
                          lambda f: ops.tokens_to_ncfhw(f.inp(tok), B, C, Fr, H, W, col0=4, out=f.out_flat((B, C, Fr, H, W))), lat, 0.0)
    N_, C = 2, 5
    for (Hi, Wi, Ho, Wo) in [(10, 7, 4, 3), (5, 5, 8, 8), (3, 9, 1, 1)]:
        xp = rnd(N_ * Hi * Wi, C, seed=Hi * Wi)
        ref = F.adaptive_avg_pool2d(xp.double().view(N_, Hi, Wi, C).permute(0, 3, 1, 2), (Ho, Wo)).permute(0, 2, 3, 1).reshape(-1, C)
        out += _edge_rows(f"edge adaptive_avgpool {Hi}x{Wi} -> {Ho}x{Wo}",
                          lambda f: ops.adaptive_avgpool(f.inp(xp, flat=True), N_, Hi, Wi, Ho, Wo, out=f.out_flat((N_ * Ho * Wo, C))), ref, 2e-3)
    return out


def check_edges_softmax_timestep():
    """softmax_rows over 1 / 255 / 257 / 8192 columns with lds, ldp > cols (poisoned padding), logits with |scale s| up to 1e4 and one
    all-equal row, against float64 and with rows summing to 1 within 2e-3; timestep_embedding at dim 2 / 320 / 1280 for t = 0, 1, 999."""
    out = []
    for cols in (1, 255, 257, 8192):
        g = torch.Generator().manual_seed(cols)
        s = (torch.randn(4, cols, generator=g) * 3.0).to(DEV)
        s[2] = 1.25                                       # one all-equal row
        for scale, tag in ((0.044194173824159216, "scale 512^-0.5"), (1e4 / float(s.abs().max()), "|scale s| up to 1e4")):
            ref = torch.softmax(scale * s.double(), 1)
            name = f"edge softmax_rows cols {cols}, {tag}"
            got = {}

            def run(f):
                got[f.framed] = ops.softmax_rows(f.inp(s), scale, out=f.out(4, cols))
                return got[f.framed]
            out += _edge_rows(name, run, ref, KTOL)
            dev = float((got[True].double().sum(1) - 1.0).abs().max())
            out.append(dict(name=name + ": rows sum to 1", err=dev, tol=2e-3, ok=dev <= 2e-3))
    t = torch.tensor([0.0, 1.0, 999.0], device=DEV)
    for dim in (2, 320, 1280):
        half = dim // 2
        arg = t.double()[:, None] * torch.exp(-math.log(10000.0) * torch.arange(half, device=DEV).double() / half)[None]
        out += _edge_rows(f"edge timestep_embedding dim {dim}, t = 0, 1, 999",
                          lambda f: ops.timestep_embedding(f.inp(t), dim, out=f.out_flat((3, dim))), torch.cat([arg.cos(), arg.sin()], -1), 2e-3)
    return out


# ------------------------------------------------------------------------------------------------ exact data, tolerance 0
# Inputs for which the exact result is representable at every intermediate step, so the expected output is known to the last bit
# whatever the summation order.  The builders run on the CPU (tests/test_exact_host.py checks their conditions and references there);
# the checks move the operands to the GPU.  Every row: ``err`` = the number of differing elements, ``tol`` = 0.
def _count_row(name, bad):
    n = int(bad.sum())
    return dict(name=name, err=float(n), l2=0.0, tol=0.0, ok=n == 0)


def _fp16_tie(v64):
    """Where a float64 value lies exactly midway between two neighbouring fp16 values (normal range)."""
    a = v64.abs()
    _, e = torch.frexp(a)                       # a = m 2^e, m in [0.5, 1): the fp16 step at a is 2^(e - 11)
    t = torch.ldexp(a, 11 - e)
    return (t - t.floor()) == 0.5


def _xg(name, M, N, C0, *, C1=0, mode=None, geo=None, rowvec_div=0, res=False, act=None, seed=0):
    mode = ops.MODE_LINEAR if mode is None else mode
    act = ops.ACT_NONE if act is None else act
    return dict(name=name, M=M, N=N, C0=C0, C1=C1, mode=mode, geo=geo, rowvec_div=rowvec_div, res=res, act=act, seed=seed)


def _xg_conv(name, n, H, W, c0, co, kind, *, c1=0, seed=0):
    """3x3 convolution specs of ``_conv_edge_cases``' geometries: geo = (n, Hi, Wi, Ho, Wo, stride, up, asym)."""
    Ho, Wo, stride, up, asym, rvd, res = H, W, 1, 0, 0, 0, False
    if kind == "s1res":
        res = True
    elif kind == "s1temb":
        rvd = H * W
    elif kind == "s2":
        Ho, Wo, stride = H // 2, W // 2, 2
    elif kind == "up":
        Ho, Wo, up = 2 * H, 2 * W, 1
    elif kind == "asym":
        Ho, Wo, stride, asym = (H - 2) // 2 + 1, (W - 2) // 2 + 1, 2, 1     # F.pad right / bottom by 1, stride 2, no other padding
    elif kind == "two":
        c1 = c1 or 128
    else:
        raise ValueError(kind)
    return _xg(name, n * Ho * Wo, co, c0, C1=c1, mode=ops.MODE_CONV2D, geo=(n, H, W, Ho, Wo, stride, up, asym), rowvec_div=rvd, res=res,
               seed=seed)


_XG_CONV_KINDS = (("s1res", "s1 +bias+res"), ("s1temb", "s1 +bias+temb"), ("s2", "stride 2"), ("up", "upsample x2"),
                  ("asym", "asym pad, stride 2"), ("two", "two-source"))
XG_CROSS = "conv 3 x 16x16 64->320 s1 +bias+res"    # the one shape every eligible family takes: the cross-family rows


def exact_gemm_specs():
    """name -> spec of every exact-integer GEMM case (smallest shapes that reach each code path; every case has a bias, so that
    the pre-rounding values sit on the 2^-4 grid and not on the integers)."""
    specs = []
    for i, (M, N, K) in enumerate([(197, 320, 128), (261, 320, 128), (197, 640, 192)]):
        specs.append(_xg(f"M{M} N{N} K{K} +bias+res", M, N, K, res=True, seed=100 + i))
    specs.append(_xg("M130 N168 K128 +bias+rowvec+res", 130, 168, 128, rowvec_div=50, res=True, seed=110))
    specs.append(_xg("M130 N12 K128 fp32 out", 130, 12, 128, act=ops.ACT_F32OUT, seed=111))
    specs.append(_xg("M130 N256 K128 fp32 out", 130, 256, 128, act=ops.ACT_F32OUT, seed=112))
    for j, (kind, tag) in enumerate(_XG_CONV_KINDS):
        specs.append(_xg_conv(f"conv 3 x 16x16 64->320 {tag}", 3, 16, 16, 64, 320, kind, seed=120 + j))
        specs.append(_xg_conv(f"conv 3 x 12x10 64->128 {tag}", 3, 12, 10, 64, 128, kind, seed=130 + j))
    specs.append(_xg("temporal B2 F5 HW24 64->320 +bias+res", 240, 320, 64, mode=ops.MODE_TEMPORAL, geo=(2, 5, 24), res=True, seed=140))
    for j, (ci, co) in enumerate([(256, 320), (640, 1280)]):      # the two shapes of check_edges_splitk
        s = _xg_conv(f"conv 48 x 8x8 {ci}->{co} s1 +bias+temb+res", 48, 8, 8, ci, co, "s1res", seed=150 + j)
        s["rowvec_div"] = 16 * 64
        specs.append(s)
    specs.append(_xg_conv("conv 1 x 32x32 64->320 s1 +bias+res", 1, 32, 32, 64, 320, "s1res", seed=160))
    specs.append(_xg_conv("conv 1 x 64x64 64->320 s1 +bias+res", 1, 64, 64, 64, 320, "s1res", seed=161))
    specs.append(_xg("M2049 N320 K320 +bias+res", 2049, 320, 320, res=True, seed=170))
    specs.append(_xg("M100 N160 K320 +bias", 100, 160, 320, seed=171))
    specs.append(_xg("M100 N512 K512 +bias+res", 100, 512, 512, res=True, seed=172))
    out = {s["name"]: s for s in specs}
    assert len(out) == len(specs) and XG_CROSS in out
    return out


_XG_CASES = {}


def exact_gemm_case(spec):
    """Operands (CPU), the exact pre-rounding values ``v`` (float64) and the contract's expected output ``want`` of one spec:
    A, W integers in [-r, r] (r = 8 up to K = 4096, 4 above, halved until the range conditions hold), bias / rowvec multiples of 2^-4 in
    [-32, 32), residual multiples of 2^-4 in [-64, 64).  Seeded; built once per process."""
    if spec["name"] in _XG_CASES:
        return _XG_CASES[spec["name"]]
    M, N, C0, C1, mode, geo = spec["M"], spec["N"], spec["C0"], spec["C1"], spec["mode"], spec["geo"]
    ci = C0 + C1
    taps = 1 if mode == ops.MODE_LINEAR else (9 if mode == ops.MODE_CONV2D else 3)
    K = taps * ci
    rows_a = M if mode != ops.MODE_CONV2D else geo[0] * geo[1] * geo[2]
    g = torch.Generator().manual_seed(spec["seed"])
    grid16 = lambda lim, *shape: (torch.randint(-16 * lim, 16 * lim, shape, generator=g).double() / 16.0)
    bias, rowvec, res = grid16(32, N), None, None
    if spec["rowvec_div"]:
        rowvec = grid16(32, (M + spec["rowvec_div"] - 1) // spec["rowvec_div"], N)
    if spec["res"]:
        res = grid16(64, M, N)
    r = 8 if K <= 4096 else 4
    while True:
        a = torch.randint(-r, r + 1, (rows_a, ci), generator=g).double()
        if mode == ops.MODE_LINEAR:
            w = torch.randint(-r, r + 1, (N, ci), generator=g).double()
            wp, v = w, a @ w.t()
        elif mode == ops.MODE_CONV2D:
            n, H, W, Ho, Wo, stride, up, asym = geo
            w = torch.randint(-r, r + 1, (N, ci, 3, 3), generator=g).double()
            wp = _pack_conv(w)
            x = a.view(n, H, W, ci).permute(0, 3, 1, 2)
            if up:
                x = F.interpolate(x, scale_factor=2.0, mode="nearest")
            v = F.conv2d(F.pad(x, (0, 1, 0, 1)), w, stride=2) if asym else F.conv2d(x, w, stride=stride, padding=1)
            assert tuple(v.shape[2:]) == (Ho, Wo)
            v = _to_tokens(v)
        else:
            B, Fr, HW = geo
            w = torch.randint(-r, r + 1, (N, ci, 3), generator=g).double()
            wp = w.permute(0, 2, 1).reshape(N, 3 * ci).contiguous()
            v = F.conv1d(a.view(B, Fr, HW, ci).permute(0, 2, 3, 1).reshape(B * HW, ci, Fr), w, padding=1)
            v = v.view(B, HW, N, Fr).permute(0, 3, 1, 2).reshape(M, N)
        v = v + bias
        if rowvec is not None:
            v = v + rowvec[torch.arange(M) // spec["rowvec_div"]]
        # sum_k |a||w| <= K r^2: with |bias| + |rowvec| on top every partial sum in any order stays below 2^18 on the 2^-4 grid, i.e.
        # within 24 bits: exact in fp32
        abs_bound = K * r * r + float(bias.abs().max()) + (float(rowvec.abs().max()) if rowvec is not None else 0.0)
        if abs_bound < 2 ** 18 and float(v.abs().max()) <= 32768 or r == 1:
            break
        r //= 2
    h = v.half()
    case = dict(spec=spec, r=r, K=K, abs_bound=abs_bound, a0=a[:, :C0].half().contiguous(), a1=a[:, C0:].half().contiguous() if C1 else None,
                w=wp.half().contiguous(), bias=bias.half(), rowvec=None if rowvec is None else rowvec.half(),
                res=None if res is None else res.half(), v=v)
    if spec["act"] == ops.ACT_F32OUT:
        case["want"] = v.float()
    else:
        case["want"] = h if res is None else (h.double() + res).half()       # fp16(fp16(acc + bias + rowvec) + R): gemm_ref.hip
        case["single"] = None if res is None else (v + res).half()            # one rounding: NOT the contract
    _XG_CASES[spec["name"]] = case
    return case


def exact_gemm_conditions(case):
    """The measured conditions of one case (tests/test_exact_host.py asserts them)."""
    v, h = case["v"], case["v"].half()
    c = dict(abs_bound=case["abs_bound"], vmax=float(v.abs().max()), unrepresentable=float((h.double() != v).double().mean()),
             ties=int(_fp16_tie(v).sum()))
    if case.get("single") is not None:
        c["single_differs"] = float((case["single"] != case["want"]).double().mean())
    return c


def _xg_launch(case, naive=False):
    spec = case["spec"]
    if "dev" not in case:
        case["dev"] = {k: (None if case[k] is None else case[k].to(DEV)) for k in ("a0", "a1", "w", "bias", "rowvec", "res")}
        case["dev"]["want"] = case["want"].to(DEV)
    d = case["dev"]
    f32 = spec["act"] == ops.ACT_F32OUT
    out = torch.zeros(spec["M"], (spec["N"] + 7) // 8 * 8, dtype=torch.float32 if f32 else torch.float16, device=DEV)[:, :spec["N"]]
    kw = {}
    if spec["mode"] == ops.MODE_CONV2D:
        kw["conv"] = spec["geo"][1:]
    elif spec["mode"] == ops.MODE_TEMPORAL:
        kw["temporal"] = spec["geo"][1:]
    return ops.gemm(d["a0"], d["w"], a1=d["a1"], bias=d["bias"], rowvec=d["rowvec"], rowvec_div=spec["rowvec_div"], residual=d["res"],
                    act=spec["act"], out=out, mode=spec["mode"], M=spec["M"], naive=naive, **kw)


def _xg_edge_kw(spec):
    """The spec in the words ``_sw_eligible`` / ``_sk_blocks`` read."""
    return dict(mode=spec["mode"], residual=True if spec["res"] else None, rowvec=True if spec["rowvec_div"] else None)


XG_PERSISTENT_CASES = ("M197 N320 K128 +bias+res", "M261 N320 K128 +bias+res", "M197 N640 K192 +bias+res", XG_CROSS,
                       "conv 3 x 16x16 64->320 s1 +bias+temb", "temporal B2 F5 HW24 64->320 +bias+res")
XG_SPLITK_CASES = (("split-K on the 128-row kernel", "conv 48 x 8x8 256->320 s1 +bias+temb+res"),
                   ("split-K on the persistent kernel", "conv 48 x 8x8 640->1280 s1 +bias+temb+res"))
XG_LDS_PATCH_CASES = (XG_CROSS, "conv 1 x 32x32 64->320 s1 +bias+res", "conv 1 x 64x64 64->320 s1 +bias+res")
XG_WS_CASES = ("M2049 N320 K320 +bias+res", "M100 N160 K320 +bias", "M100 N512 K512 +bias+res")
XG_GROUPS = ("tile reg", "tile glds", "naive", "persistent", "split-K", "LDS patch", "weight-stationary", "cross-family")


def _xg_tile_cases(specs):
    return [n for n, s in specs.items() if n not in XG_WS_CASES and n not in XG_LDS_PATCH_CASES[1:] and not n.startswith("conv 48 x")]


def exact_gemm_launches(groups=XG_GROUPS):
    """(group, family, spec name, GEMM_FLAGS bits, USE_GLDS, naive, skip reason or None) of every launch ``check_gemm_exact`` makes; the
    cross-family launches are repeats of launches of the other groups and are not listed.  tests/test_gemm_plan_host.py pins the
    family each one names on the CPU."""
    specs = exact_gemm_specs()
    L = []
    for var in ("tile reg", "tile glds", "naive"):
        if var in groups:
            L += [(var, "naive kernel" if var == "naive" else "128-row " + var[5:], n, 4 | 16, var == "tile glds", var == "naive", None)
                  for n in _xg_tile_cases(specs)]
    if "persistent" in groups:
        for fam, bits in PERSISTENT_FAMILIES:
            for n in XG_PERSISTENT_CASES:
                s, why = specs[n], None
                if bits in (1 << 21, 1 << 27) and not _sw_eligible(s["N"], _xg_edge_kw(s), s["C0"]):
                    why = "shape not eligible for the one-wave-per-SIMD kernel"
                elif bits == 1 << 27 and _sk_blocks(s["M"], s["N"], _xg_edge_kw(s), s["C0"]) == 0:
                    why = "fewer than 8 (tile, K-tile) units: no stream-K form"
                L.append(("persistent", fam, n, bits, True, False, why))
    if "split-K" in groups:
        L += [("split-K", fam, n, 0, True, False, None) for fam, n in XG_SPLITK_CASES]
    if "LDS patch" in groups:
        L += [("LDS patch", "LDS patch", n, 1 << 28, True, False, None) for n in XG_LDS_PATCH_CASES]
    if "weight-stationary" in groups:
        L += [("weight-stationary", "ws", n, 1024, True, False, None) for n in XG_WS_CASES]
    return L


def _xg_run(case, bits, glds, naive):
    saved, saved_glds = ops.GEMM_FLAGS, ops.USE_GLDS
    try:
        ops.USE_GLDS = glds
        ops.GEMM_FLAGS = ((saved & ~4) | bits) if not bits & 4 else (saved | bits)
        return _xg_launch(case, naive=naive)
    finally:
        ops.GEMM_FLAGS, ops.USE_GLDS = saved, saved_glds


def check_gemm_exact(groups=XG_GROUPS):
    """Every GEMM family on exact-integer data against the epilogue contract of gemm_ref.hip, fp16(fp16(acc + bias + rowvec) + R), bit
    for bit: the 128-row kernel (register- and LDS-DMA-staged), the naive kernel, the five forced persistent families, both split-K forms
    (fp32 workspace NaN-filled), the LDS-patch convolution, the weight-stationary kernel; fp32 outputs equal the exact value.  Then, on
    one shape every eligible family takes, each family's output against the naive kernel's."""
    out = []
    specs = exact_gemm_specs()
    for (group, fam, n, bits, glds, naive, why) in exact_gemm_launches(groups):
        name = f"exact gemm[{fam}] {n}"
        if why is not None:
            out.append(_skip_row(name, why))
            continue
        case = exact_gemm_case(specs[n])
        if group == "split-K":
            ops._workspace(DEV).fill_(float("nan"))
        y = _xg_run(case, bits, glds, naive)
        out.append(_count_row(name + ": differing elements", y != case["dev"]["want"]))
    if "cross-family" in groups:
        case = exact_gemm_case(specs[XG_CROSS])
        y_naive = _xg_run(case, 4 | 16, True, True)
        fams = [("128-row reg", 4 | 16, False), ("128-row glds", 4 | 16, True)] + [(f, b, True) for f, b in PERSISTENT_FAMILIES] + [("LDS patch", 1 << 28, True)]
        for fam, bits, glds in fams:
            out.append(_count_row(f"exact gemm[{fam}] {XG_CROSS} == the naive kernel, bit for bit", _xg_run(case, bits, glds, False) != y_naive))
        out.append(_skip_row(f"exact gemm[split-K] {XG_CROSS} == the naive kernel", "9 K-tiles: no split-K plan takes this shape"))
        out.append(_skip_row(f"exact gemm[ws] {XG_CROSS} == the naive kernel", "the weight-stationary kernel takes Linear layers only"))
    torch.cuda.synchronize()
    return out


def exact_gemm_plan_rows():
    """(row name, descriptor line for tests/gemm_plan_main.cpp, family the check names) of every launch of ``check_gemm_exact``."""
    specs = exact_gemm_specs()
    rows = []
    for k, (group, fam, n, bits, glds, naive, why) in enumerate(exact_gemm_launches()):
        if why is not None:
            continue
        s = specs[n]
        flags = (1 if naive else 0) | (2 if glds else 0) | bits
        ld = (s["N"] + 7) // 8 * 8
        desc = f"mode={s['mode']} M={s['M']} N={s['N']} C0={s['C0']} C1={s['C1']} ldc={ld} bias=1 act={s['act']} flags={flags}"
        if s["rowvec_div"]:
            desc += f" rowvec=1 rowvec_div={s['rowvec_div']}"
        if s["res"]:
            desc += " R=1"
        if s["mode"] == ops.MODE_CONV2D:
            desc += " Hi={1} Wi={2} Ho={3} Wo={4} stride={5} up={6} asym={7}".format(*s["geo"])
        elif s["mode"] == ops.MODE_TEMPORAL:
            desc += " F={1} HW={2}".format(*s["geo"])
        rows.append((f"exact_{k:03d}", desc, fam, n))
    return rows


# ---- attention: every key, once
def _xa_rows(batch, S, inner, strides):
    outer, inner_s, seq = strides
    i = torch.arange(batch)
    return ((i // inner) * outer + (i % inner) * inner_s)[:, None] + torch.arange(S)[None] * seq   # [batch, S]


def _xa(name, kernel, instantiation, *, batch, heads, Sq, Sk, d=64, inner=1, q_strides=None, kv_strides=None, kv_div=1, qk_mod=0, causal=False,
        bias=False, naive=False, seed=0):
    return dict(name=name, kernel=kernel, instantiation=instantiation, batch=batch, heads=heads, Sq=Sq, Sk=Sk, d=d, inner=inner,
                q_strides=(Sq, 0, 1) if q_strides is None else q_strides, kv_strides=(Sk, 0, 1) if kv_strides is None else kv_strides,
                kv_div=kv_div, qk_mod=qk_mod, causal=causal, bias=bias, naive=naive, seed=seed)


XA_KERNELS = ("4-wave flash", "short one-wave", "shared-softmax 4-wave", "8-wave", "whole-sequence MFMA", "96-key loop", "bias", "generic")


def exact_attention_specs():
    """The smallest shapes that reach each kernel of attention.hip, and each of its template instantiations (dispatch:
    anyv2v_amd/csrc/attention_plan.cpp; ``instantiation`` is the planner's name of what the launch runs -- tests/test_attention_plan_host.py
    plans every spec and holds the union against the planner's own list)."""
    S = []
    t = lambda Fr, HW: dict(inner=HW, q_strides=(Fr * HW, 1, HW), kv_strides=(Fr * HW, 1, HW))   # temporal: a sequence's rows HW apart
    S.append(_xa("b2 h2 S333", "4-wave flash", "flash<2,1,4>", batch=2, heads=2, Sq=333, Sk=333, seed=1))
    S.append(_xa("cross b6 h2 Sq100 Sk145 kv_div3", "4-wave flash", "flash<2,1,4>", batch=6, heads=2, Sq=100, Sk=145, kv_div=3, seed=2))
    S.append(_xa("temporal F40 (3 x 20 px) h2", "4-wave flash", "flash<2,1,4>", batch=60, heads=2, Sq=40, Sk=40, seed=3, **t(40, 20)))
    for Fr in (16, 8):
        S.append(_xa(f"temporal F{Fr} (3 x 20 px) h2", "short one-wave", "short<1>", batch=60, heads=2, Sq=Fr, Sk=Fr, seed=4 + Fr, **t(Fr, 20)))
        S.append(_xa(f"temporal F{Fr} (3 x 20 px) h2 qk_mod (three streams)", "short one-wave", "short<3>", batch=60, heads=2, Sq=Fr, Sk=Fr, qk_mod=20,
                     seed=5 + Fr, **t(Fr, 20)))
    S.append(_xa("b3 h1 S333 qk_mod1 (three streams)", "shared-softmax 4-wave", "flash<2,3,4>", batch=3, heads=1, Sq=333, Sk=333, qk_mod=1, seed=30))
    S.append(_xa("plain b64 h4 Sq1024 Sk2100 kv_div64", "8-wave", "flash<3,1,8>", batch=64, heads=4, Sq=1024, Sk=2100, kv_div=64, seed=31))
    S.append(_xa("shared-softmax b96 h4 S2100 qk_mod32", "8-wave", "flash<3,3,8>", batch=96, heads=4, Sq=2100, Sk=2100, qk_mod=32, seed=32))
    for (B, h, Sn, d, causal, inst) in [(2, 3, 257, 80, False, "small<3,18>"), (2, 2, 77, 160, False, "small<5,6>"), (3, 8, 24, 40, False, "small<2,6>"),
                                        (3, 4, 77, 64, True, "small<2,6>"),
                                        # the other instantiations: ragged query blocks and key tails below 96 keys, both edges of 97 .. 288 keys
                                        (2, 2, 50, 80, False, "small<3,6>"), (2, 2, 90, 128, True, "small<4,6>"), (2, 2, 97, 56, False, "small<2,18>"),
                                        (2, 2, 288, 104, False, "small<4,18>")]:
        S.append(_xa(f"B{B} h{h} S{Sn} d{d} causal={causal}", "whole-sequence MFMA", inst, batch=B, heads=h, Sq=Sn, Sk=Sn, d=d, causal=causal, seed=Sn + d))
    for (B, h, Sn, d, causal, inst) in [(2, 2, 401, 40, False, "loop<2>"), (2, 2, 160, 160, False, "loop<5>"), (1, 2, 401, 56, True, "loop<2>"),
                                        # just past 288 keys (97 at head_dim 160); head_dim 24 runs the loop kernel from 289 keys on
                                        (1, 2, 289, 72, False, "loop<3>"), (1, 2, 289, 128, True, "loop<4>"), (2, 2, 97, 160, False, "loop<5>"),
                                        (2, 3, 289, 24, False, "loop<2>")]:
        S.append(_xa(f"B{B} h{h} S{Sn} d{d} causal={causal}", "96-key loop", inst, batch=B, heads=h, Sq=Sn, Sk=Sn, d=d, causal=causal, seed=Sn + d + 1))
    S.append(_xa("8 x 80, 16 frames (2 x 6 px): MFMA form", "bias", "small<3,6,bias>", batch=12, heads=8, Sq=16, Sk=16, d=80, bias=True, seed=40, **t(16, 6)))
    S.append(_xa("2 x 20, 5 frames (2 x 6 px): generic kernel", "bias", "naive+bias", batch=12, heads=2, Sq=5, Sk=5, d=20, bias=True, seed=41, **t(5, 6)))
    for d, inst in ((40, "small<2,6,bias>"), (128, "small<4,6,bias>"), (160, "small<5,6,bias>")):    # the MFMA form's last key count
        S.append(_xa(f"b2 h2 Sq100 Sk96 d{d}: MFMA form", "bias", inst, batch=2, heads=2, Sq=100, Sk=96, d=d, bias=True, seed=42 + d))
    S.append(_xa("b2 h2 Sq100 Sk97 d40: generic kernel", "bias", "naive+bias", batch=2, heads=2, Sq=100, Sk=97, d=40, bias=True, seed=43))
    S.append(_xa("naive=True b2 h2 S333", "generic", "naive", batch=2, heads=2, Sq=333, Sk=333, naive=True, seed=1))
    S.append(_xa("naive=True B3 h8 S24 d40", "generic", "naive", batch=3, heads=8, Sq=24, Sk=24, d=40, naive=True, seed=64))
    S.append(_xa("naive=True B3 h4 S77 d64 causal", "generic", "naive", batch=3, heads=4, Sq=77, Sk=77, d=64, causal=True, naive=True, seed=141))
    S.append(_xa("B2 h3 S288 d24 (one 32-column group, <= 288 keys)", "generic", "naive", batch=2, heads=3, Sq=288, Sk=288, d=24, seed=312))
    assert len({s["name"] + s["kernel"] for s in S}) == len(S) and {s["kernel"] for s in S} == set(XA_KERNELS)
    assert all(s["instantiation"] in ATTN_KERNEL_INSTANTIATIONS[s["kernel"]] for s in S)
    return S


def exact_attention_patterns(spec):
    """selection everywhere; counting without the causal mask at Sk <= 1024 (there Sk / (Sk +- 1) is no fp16 neighbour of 1 that the
    rounding of O could hide); the causal edge on the kernels with the causal flag."""
    return ("selection",) + (("causal edge",) if spec["causal"] else (("counting",) if spec["Sk"] <= 1024 else ()))


def _xa_layout(spec):
    b, kv_div = spec["batch"], spec["kv_div"]
    n_kv = (b + kv_div - 1) // kv_div
    rq = _xa_rows(b, spec["Sq"], spec["inner"], spec["q_strides"])
    rkv = _xa_rows(n_kv, spec["Sk"], spec["inner"], spec["kv_strides"])
    i = torch.arange(b)
    iq = i % spec["qk_mod"] if spec["qk_mod"] else i
    return rq, rkv, i, iq, n_kv, int(rq.max()) + 1, int(rkv.max()) + 1


def exact_attention_gain(scale):
    """The smallest power of two g with 2 g scale log2(e) >= 160."""
    return 2.0 ** math.ceil(math.log2(80.0 / (scale * math.log2(math.e))))


def _xa_keys(Sk, causal):
    if causal:     # 0, the 64-query block edges +- 1 and the 96-key block edges +- 1
        ks = {0} | {e + o for e in list(range(64, Sk + 1, 64)) + list(range(96, Sk + 1, 96)) for o in (-1, 0, 1)}
    else:          # the first and last key of every 16-key step (the 64- and 96-key tile edges are among them), and the last key
        ks = {k for t in range(0, Sk, 16) for k in (t, t + 15)} | {Sk - 1}
    return sorted(k for k in ks if 0 <= k < Sk)


def exact_attention_case(spec, pattern):
    """Operands (CPU) and the expectation of one launch: dict(q, k, v [rows, heads * d] fp16, bias or None, rows = the output rows the
    launch writes, want = their expected values [len(rows), heads * d] fp16, pi / keys = what the pattern selected)."""
    b, h, Sq, Sk, d = spec["batch"], spec["heads"], spec["Sq"], spec["Sk"], spec["d"]
    C = h * d
    rq, rkv, i, iq, n_kv, Mq, Mk = _xa_layout(spec)
    g = torch.Generator().manual_seed(spec["seed"])
    gauss = lambda *shape: torch.randn(*shape, generator=g).half()
    case = dict(spec=spec, pattern=pattern, rows=rq.reshape(-1), bias=None, scale=d ** -0.5)
    vrows = rkv[i // spec["kv_div"]]                                   # [batch, Sk]: the V rows of element i
    hh = torch.arange(h)
    if pattern == "selection":
        nbits = max(1, math.ceil(math.log2(Sk)))
        assert 2 <= nbits <= d
        v = gauss(Mk, C)
        q, k = torch.zeros(Mq, C, dtype=torch.float16), gauss(Mk, C)
        s = torch.arange(Sq)
        if spec["bias"]:   # the selection sits in the bias: q = 0, another permutation per head
            pi = ((s[None, :] + 3 * hh[:, None] + 1) % Sk)[None].expand(b, h, Sq)
            bias = torch.full((h, Sq, Sk), -200.0)
            bias.scatter_(2, pi[0][:, :, None], 0.0)
            case["bias"] = bias
        else:
            codes = torch.zeros(Sk, d)
            codes[:, :nbits] = ((torch.arange(Sk)[:, None] >> torch.arange(nbits)[None]) & 1).float() * 2 - 1
            n_q = spec["qk_mod"] if spec["qk_mod"] else b
            e = torch.arange(n_q)
            if spec["causal"]:    # a visible key: the query's own, or the one before it on every other (element, head)
                pi = (s[None, None, :] - ((e[:, None, None] + hh[None, :, None]) & 1)).clamp_min(0).expand(n_q, h, Sq)
            else:
                pi = (s[None, None, :] + (e[:, None, None] * h + hh[None, :, None]) * Sq) % Sk
            gain = exact_attention_gain(case["scale"])
            k = torch.zeros(Mk, C, dtype=torch.float16)
            k[rkv.reshape(-1)] = codes.half().repeat(1, h).repeat(n_kv, 1)
            q[rq[:n_q].reshape(-1)] = (gain * codes[pi.permute(0, 2, 1)]).reshape(n_q * Sq, C).half()     # [n_q, Sq, h, d]
            pi = pi[iq]                                                  # [batch, h, Sq]
        vsel = vrows[torch.arange(b)[:, None, None], pi]                # [batch, h, Sq]: V row of (element, head, query)
        want = v.view(Mk, h, d)[vsel.permute(0, 2, 1), hh[None, None, :]]   # [batch, Sq, h, d]
        case.update(q=q, k=k, v=v, pi=pi, want=want.reshape(b * Sq, C))
    else:
        keys = _xa_keys(Sk, pattern == "causal edge")
        assert n_kv * h * d >= len(keys), "not enough (element, head, channel) slots for the key sweep"
        key_c = torch.tensor(keys)[torch.arange(n_kv * C) % len(keys)].view(n_kv, C)       # slot (element, head, channel) -> key
        v = torch.zeros(Mk, C, dtype=torch.float16)
        v[rkv[torch.arange(n_kv)[:, None], key_c].reshape(-1), torch.arange(C).repeat(n_kv)] = float(Sk) if pattern == "counting" else 1.0
        q, k = torch.zeros(Mq, C, dtype=torch.float16), gauss(Mk, C)
        if spec["bias"]:
            case["bias"] = torch.zeros(h, Sq, Sk)
        kc = key_c[i // spec["kv_div"]]                                 # [batch, C]
        if pattern == "counting":
            want = torch.ones(b * Sq, C, dtype=torch.float16)
        else:
            s = torch.arange(Sq)
            inv = _round_once_fp16(1.0 / (s.double() + 1.0)).cpu()
            want = torch.where(kc[:, None, :] > s[None, :, None], torch.zeros((), dtype=torch.float16), inv[None, :, None]).reshape(b * Sq, C)
        case.update(q=q, k=k, v=v, keys=keys, key_c=kc, want=want)
    return case


def exact_attention_sdpa(case, only):
    """fp32 SDPA on the CPU with the entry point's addressing, for the batch elements ``only``: [len(only), Sq, heads * d]."""
    spec = case["spec"]
    h, d, Sq, Sk = spec["heads"], spec["d"], spec["Sq"], spec["Sk"]
    rq, rkv, i, iq, n_kv, Mq, Mk = _xa_layout(spec)
    only = torch.tensor(only)
    sp = lambda x, rows, S: x[rows.reshape(-1)].float().view(len(only), S, h, d).transpose(1, 2)
    q, k = sp(case["q"], rq[iq[only]], Sq), sp(case["k"], rkv[iq[only] // spec["kv_div"]], Sk)
    v = sp(case["v"], rkv[only // spec["kv_div"]], Sk)
    if case["bias"] is not None:
        o = F.scaled_dot_product_attention(q, k, v, attn_mask=case["bias"][None], scale=case["scale"])
    else:
        o = F.scaled_dot_product_attention(q, k, v, is_causal=spec["causal"], scale=case["scale"])
    return o.transpose(1, 2).reshape(len(only), Sq, h * d)


def exact_attention_bad(case, got):
    """Elementwise verdict of ``got`` (the written rows, [len(rows), C] fp16) against the expectation: selection and counting bit for
    bit; causal edge exactly 0 above the diagonal and within 1 fp16 step of 1 / (i + 1) elsewhere."""
    want = case["want"].to(got.device)
    if case["pattern"] != "causal edge":
        return got != want
    return torch.where(want == 0, got != 0, (_fp16_ulps(got, want) > 1) | (got == 0))


def _xa_operands(spec, Mq, Mk, device):
    """The (uninitialised) operands of an exact launch: (q, k, v, o)."""
    C = spec["heads"] * spec["d"]
    new = lambda M, W: torch.empty(M, W, dtype=torch.float16, device=device)
    if Mq == Mk and spec["kv_div"] == 1 and spec["q_strides"] == spec["kv_strides"]:
        t = new(Mq, 3 * C)                           # self-attention: column windows of one fused QKV matrix
        q, k, v = t[:, :C], t[:, C:2 * C], t[:, 2 * C:]
    else:
        t = new(Mk, 2 * C)                           # Q of its own, K / V column windows of one matrix
        q, k, v = new(Mq, C), t[:, :C], t[:, C:]
    return q, k, v, new(Mq, C)


def _xa_kw(spec):
    d = spec["d"]
    kw = dict(batch=spec["batch"], heads=spec["heads"], Sq=spec["Sq"], Sk=spec["Sk"], inner=spec["inner"], q_strides=spec["q_strides"],
              kv_strides=spec["kv_strides"], kv_div=spec["kv_div"], qk_mod=spec["qk_mod"], naive=spec["naive"])
    if not (d == 64 and not spec["causal"] and not spec["bias"]):
        kw.update(scale=d ** -0.5, head_dim=d, causal=spec["causal"])
    return kw


def _xa_launch(case):
    spec = case["spec"]
    q, k, v, o = _xa_operands(spec, case["q"].shape[0], case["k"].shape[0], DEV)
    q.copy_(case["q"])
    k.copy_(case["k"])
    v.copy_(case["v"])
    o.fill_(float("nan"))
    ops.attention(q, k, v, o, bias=None if case["bias"] is None else case["bias"].to(DEV), **_xa_kw(spec))
    return o[case["rows"].to(DEV)]


def exact_attention_plan_rows():
    """(row name, line for tests/attention_plan_main.cpp, kernel named, instantiation named) of every launch of ``check_attention_exact``."""
    rows = []
    for spec in exact_attention_specs():
        Mq, Mk = _xa_layout(spec)[5:7]
        q, k, v, o = _xa_operands(spec, Mq, Mk, "meta")
        rows.append((f"exact | {spec['kernel']}: {spec['name']}", attn_plan_words(q, k, v, o, bias=spec["bias"], **_xa_kw(spec)), spec["kernel"],
                     spec["instantiation"]))
    return rows


def check_attention_exact(kernels=XA_KERNELS):
    """Every kernel of attention.hip on three exact patterns.  Selection: a one-hot softmax (keys = the +-1 codes of their index,
    query i = a power-of-two gain x the code of pi(i), so every other score sits >= 160 binary orders below; on the bias kernels the
    selection is in the bias) -- O[i] = V[pi(i)] bit for bit, every key a target.  Counting: q = 0, V[key_c, c] = Sk -- every output
    exactly 1.0 (each key read once and counted once in the denominator).  Causal edge: q = 0, V[key_c, c] = 1 -- exactly 0 iff
    key_c > i, else 1 / (i + 1) to 1 fp16 step.  No kernel needs a last-bit allowance on the first two: P is exactly 0 or 1 in fp16, l is
    exactly 1 (selection; the flash kernels' l = exp2 of a rounding residual < 2^-13 leaves V x (1 / l) inside V's rounding interval)
    or Sk (counting), and Sk x fl(1 / Sk) rounds to 1."""
    out = []
    for spec in exact_attention_specs():
        if spec["kernel"] not in kernels:
            continue
        for pattern in exact_attention_patterns(spec):
            case = exact_attention_case(spec, pattern)
            got = _xa_launch(case)
            what = "differing elements" if pattern != "causal edge" else "elements off (0 above the diagonal, 1 / (i + 1) +- 1 ulp below)"
            out.append(_count_row(f"exact attention[{spec['kernel']}] {spec['name']}, {pattern}: {what}", exact_attention_bad(case, got)))
    torch.cuda.synchronize()
    return out


EDGE_CHECKS = [check_edges_gemm_tile, check_edges_conv, check_edges_gemm_persistent, check_edges_splitk, check_edges_conv_lds_patch,
               check_edges_gemm_ws, check_edges_ff_fused, check_edges_attention, check_edges_attention_8wave, check_edges_attention_small,
               check_edges_elementwise, check_edges_layout, check_edges_softmax_timestep]

ALL_KERNEL_CHECKS = [check_selftest, check_gemm, check_gemm_big, check_gemm_ws, check_gemm_ws_ln, check_gemm_splitk, check_conv, check_norms, check_attention,
                     check_attention_small_mfma, check_attention_bias_and_rotary_windows, check_gelu_all_inputs, check_silu_all_inputs,
                     check_timestep_embedding_all_timesteps, check_elementwise,
                     check_full_size_properties, check_vae_kernels] + EDGE_CHECKS + [check_gemm_exact, check_attention_exact]


def check_frame_parallel(Fr=4, hw=16, tol=4e-3):
    """Frame-parallel clip (``anyv2v_amd.parallel.FrameParallel``): called on every rank of an
    initialised process group; the sharded forward must reproduce this rank's own unsharded forward (same kernels, same
    weights; only the order of the fp32 additions inside the 5-D GroupNorm statistics differs), with and without the
    PnP hooks and the shared stem, and leave the pipeline untouched."""
    import types
    from anyv2v_amd import pnp_utils
    from anyv2v_amd.parallel import FrameParallel
    from oracle import pnp_oracle
    out = []
    fp = FrameParallel()
    native, oracle, ocfg = build_pair("mini", 1234)
    otol = 8e-3   # mini model, HIP fp16 (or the CPU emulation) vs the fp32 CPU oracle: 3 x the measured 2.0-2.4e-3 (round 4)
    for B in (1, 3):
        inp = config1_inputs(ocfg, B, Fr, hw)
        if B == 3:  # the edit loop's batch: slots 1 and 2 share latent and image latents (shared stem allowed)
            inp["sample"][2] = inp["sample"][1]
            inp["image_latents"][2] = inp["image_latents"][1]
        smp = inp["sample"].half().to(DEV)
        kw = dict(fps=inp["fps"].to(DEV), image_latents=inp["image_latents"].half().to(DEV),
                  image_embeddings=inp["image_embeddings"].half().to(DEV),
                  encoder_hidden_states=inp["encoder_hidden_states"].half().to(DEV))
        cases = [("no hooks", 981, False)]
        if B == 3:
            ts = [981 - 20 * i for i in range(50)]
            pipe = types.SimpleNamespace(unet=native)
            pnp_utils.register_conv_injection(pipe, ts[:10])
            pnp_utils.register_spatial_attention_pnp(pipe, ts[:25])
            pnp_utils.register_temp_attention_pnp(pipe, ts[:40])
            pnp_oracle.register_conv_injection(oracle, ts[:10])
            pnp_oracle.register_spatial_attention_pnp(oracle, ts[:25])
            pnp_oracle.register_temp_attention_pnp(oracle, ts[:40])
            cases = [("PnP all sites", 981, False), ("PnP temporal only + shared stem", 301, True), ("PnP off", 1, True)]
        for name, t, shared in cases:
            if B == 3:
                pnp_utils.register_time(pipe, t)
                pnp_oracle.register_time(oracle, t)
            with torch.no_grad():  # the checker: fp32 CPU oracle on the same fp16-rounded inputs (not only "vs itself")
                v_or = oracle(smp.float().cpu(), t, fps=inp["fps"], image_latents=inp["image_latents"].half().float(),
                              image_embeddings=inp["image_embeddings"].half().float(),
                              encoder_hidden_states=inp["encoder_hidden_states"].half().float())[0]
            res = []
            for use_fp in (None, fp):
                native.set_frame_parallel(use_fp)
                native.forward_tokens(smp, t, kw["fps"], kw["image_latents"], kw["image_embeddings"], kw["encoder_hidden_states"])
                native._ctx.shared_stem = shared
                res.append(native(smp, t, **kw)[0].float().cpu())
            out.append(_res(f"frame-parallel x{fp.world} rank {fp.rank}: B{B} {name} vs unsharded", res[1], res[0], tol))
            out.append(_res(f"frame-parallel x{fp.world} rank {fp.rank}: B{B} {name} vs the fp32 CPU oracle", res[1], v_or, otol))
        if B == 3:
            pnp_oracle.clear_hooks(oracle)
    # the pipeline loops on top (unchanged code: every rank steps the full, replicated latents): 4-step inversion, then
    # a 4-step PnP edit with schedules that end early (so the 2-branch steps are covered too)
    from anyv2v_amd.pipeline import I2VGenXLPipeline
    from anyv2v_amd.schedulers import DDIMInverseScheduler, DDIMScheduler
    inp = config1_inputs(ocfg, 3, Fr, hw)
    h = lambda x: x.half().to(DEV)
    lat0, ehs, ie, il = h(inp["sample"][:1]), h(inp["encoder_hidden_states"]), h(inp["image_embeddings"]), h(inp["image_latents"])
    n_steps, finals = 4, []
    for use_fp in (None, fp):
        native.set_frame_parallel(use_fp)
        pipe = I2VGenXLPipeline(unet=native, scheduler=DDIMInverseScheduler())
        pipe._device = torch.device(DEV)
        traj = pipe.invert(prompt_embeds=ehs[:1], image_embeddings=ie[:1], image_latents=il[:1], height=hw * 8, width=hw * 8,
                           num_frames=Fr, num_inference_steps=n_steps, guidance_scale=1.0, target_fps=8, latents=lat0,
                           return_trajectory=True)
        T = max(traj.keys())
        sched = DDIMScheduler()
        sched.set_timesteps(n_steps)
        pnp_utils.register_conv_injection(pipe, sched.timesteps[:1])
        pnp_utils.register_spatial_attention_pnp(pipe, sched.timesteps[:2])
        pnp_utils.register_temp_attention_pnp(pipe, sched.timesteps[:3])
        pipe.register_modules(scheduler=sched)
        res = pipe.sample_with_pnp(prompt_embeds=ehs[2:3], negative_prompt_embeds=ehs[1:2], image_embeddings=ie[2:3],
                                   image_latents=il[2:3], height=hw * 8, width=hw * 8, num_frames=Fr,
                                   num_inference_steps=n_steps, guidance_scale=9.0, target_fps=8, latents=traj[T].clone(),
                                   output_type="latent", ddim_init_latents_t_idx=0, ddim_inv_latents_path=traj,
                                   ddim_inv_prompt_embeds=ehs[:1], ddim_inv_image_embeddings=ie[:1],
                                   ddim_inv_image_latents=il[:1]).frames
        finals.append((traj[T].float().cpu(), res.float().cpu()))
        pnp_utils.clear_time(pipe)
    out.append(_res(f"frame-parallel rank {fp.rank}: pipeline.invert {n_steps} steps vs unsharded", finals[1][0], finals[0][0], 6e-3))   # measured 1.5e-3
    out.append(_res(f"frame-parallel rank {fp.rank}: pipeline.sample_with_pnp {n_steps} steps vs unsharded", finals[1][1],
                    finals[0][1], 4e-2))
    native.set_frame_parallel(None)
    out.append({"name": f"frame-parallel rank {fp.rank}: all-to-all payload > 0", "err": 0.0 if fp.bytes_moved > 0 else 1.0,
                "tol": 0.5, "ok": fp.bytes_moved > 0})
    return out


# ------------------------------------------------------------------------------------------------ far operands: offsets past 2^32 bytes
# A small logical operand inside one large allocation, its rows so far apart that the last row starts 2^32 bytes or more behind the
# pointer the kernel gets, and that pointer FAR_LEAD bytes into the allocation.  An offset a kernel truncates to 32 bits -- signed or
# unsigned, counted in elements or in bytes -- then lies between the pointer - 4 GiB and the true offset, i.e. inside the allocation:
# a truncating kernel reads or writes a wrong row (a failing row of the check), it does not fault.  With power-of-two strides every
# such image falls on the start of another row of the operand or, for the negative ones, in front of it; the helper writes those
# places ("decoys") with other random data, so a wrong read is wrong deterministically and a wrong store is seen.  The geometry is
# plain integers (numpy): tests/test_far_operands_host.py checks every case on the CPU.  Memory is ``torch.empty`` and never filled;
# only the operand's rows and the decoys are written.
FAR_LEAD = 4 << 30
FAR_CAP = 10 << 30
FAR_MIN_FREE = 12 << 30
FAR_KINDS = ("unsigned elements", "signed elements", "unsigned bytes", "signed bytes")


def far_geometry(name, offsets, cols, item=2, **extra):
    """``offsets``: element offsets of the operand's row starts from the pointer handed to the kernel, in logical row order."""
    import numpy as np
    offs = np.asarray(offsets, dtype=np.int64).reshape(-1)
    return dict(name=name, offsets=offs, cols=int(cols), item=int(item), lead=FAR_LEAD, **extra)


def far_images(geo):
    """The four 32-bit images of every row offset, as element offsets: {kind: int64 array}."""
    o, it = geo["offsets"], geo["item"]
    u = lambda v: v & 0xFFFFFFFF
    s = lambda v: ((v + (1 << 31)) & 0xFFFFFFFF) - (1 << 31)
    return {"unsigned elements": u(o), "signed elements": s(o), "unsigned bytes": u(o * it) // it, "signed bytes": s(o * it) // it}


def far_decoys(geo):
    """Images that are not themselves a row start (sorted, unique)."""
    import numpy as np
    return np.setdiff1d(np.unique(np.concatenate(list(far_images(geo).values()))), geo["offsets"])


def far_span_bytes(geo):
    return geo["lead"] + (int(geo["offsets"].max()) + geo["cols"]) * geo["item"]


def far_ld(rows, item=2):
    """The power-of-two row stride (elements) that puts row ``rows - 1`` at or past 2^32 bytes."""
    ld = 1
    while (rows - 1) * ld * item < (1 << 32):
        ld *= 2
    return ld


def far_matrix_geometry(name, M, cols, item=2):
    ld = far_ld(M, item)
    assert ld < (1 << 31) and cols <= ld
    import numpy as np
    return far_geometry(name, np.arange(M, dtype=np.int64) * ld, cols, item, ld=ld, rows=M)


def far_skip_reason():
    free = torch.cuda.mem_get_info()[0]
    return None if free >= FAR_MIN_FREE else f"{free / 2 ** 30:.1f} GiB of device memory free, the far cases need 12"


FAR_PEAK = {}   # case name -> peak bytes allocated (torch) while it ran


class _FarBuffer:
    """The allocation behind one far operand."""

    def __init__(self, geo, dtype, seed=0):
        item = torch.empty(0, dtype=dtype).element_size()
        assert item == geo["item"] and far_span_bytes(geo) <= FAR_CAP
        self.geo, self.cols = geo, geo["cols"]
        self.flat = torch.empty((far_span_bytes(geo) // item + 7) // 8 * 8, dtype=dtype, device=DEV)
        self.base = geo["lead"] // item
        ar = torch.arange(self.cols, device=DEV)
        self.ix = ((torch.from_numpy(geo["offsets"]).to(DEV) + self.base)[:, None] + ar[None]).reshape(-1)
        dec = far_decoys(geo)
        self.dix = ((torch.from_numpy(dec).to(DEV) + self.base)[:, None] + ar[None]).reshape(-1)
        g = torch.Generator().manual_seed(977 + seed)
        self.dvals = (torch.randn(len(dec) * self.cols, generator=g) * 3.0 + 40.0).to(dtype).to(DEV)   # no operand holds such values
        if len(dec):
            self.flat[self.dix] = self.dvals

    def write(self, t):
        assert t.numel() == self.ix.numel()
        self.flat[self.ix] = t.reshape(-1).to(self.flat.dtype)
        # the indexed store above, checked through plain slices (whose offsets the host computes) on the first and the last row
        for r in (0, len(self.geo["offsets"]) - 1):
            o = self.base + int(self.geo["offsets"][r])
            bits = torch.int16 if self.flat.element_size() == 2 else torch.int32
            assert torch.equal(self.flat[o:o + self.cols].view(bits), t.reshape(-1, self.cols)[r].to(self.flat.dtype).contiguous().view(bits))

    def read(self):
        return self.flat[self.ix].view(-1, self.cols)

    def decoys_intact(self):
        return bool(torch.equal(self.flat[self.dix], self.dvals)) if self.dix.numel() else True

    def view(self, shape, strides):
        return torch.as_strided(self.flat, shape, strides, self.base)


def _poison(shape, dtype):
    if dtype == torch.float32:
        return torch.full(shape, POISON32, dtype=torch.int32, device=DEV).view(torch.float32)
    return torch.full(shape, POISON16, dtype=torch.int16, device=DEV).view(torch.float16)


class _FarOperands:
    """Hands a launch its matrices: plain tensors, except the one called ``which``, which lies in a ``_FarBuffer`` with
    ``far_matrix_geometry`` (a power-of-two leading dimension).  ``out`` matrices start as the poison pattern."""

    def __init__(self, which=None):
        self.which, self.buf, self.is_out = which, None, False

    def mat(self, name, t, out=False, inplace=False):
        if t is None:
            return None
        shape, dtype = tuple(t.shape), t.dtype
        init = _poison(shape, dtype) if out and not inplace else t
        if name != self.which:
            return init.clone() if out else t
        geo = far_matrix_geometry(name, shape[0], shape[1], t.element_size())
        self.buf, self.is_out = _FarBuffer(geo, dtype, seed=shape[0]), out
        self.buf.write(init)
        return self.buf.view(shape, (geo["ld"], 1))

    def result(self, y):
        return self.buf.read() if (self.buf is not None and self.is_out) else y

    def intact(self):
        return self.buf is None or self.buf.decoys_intact()

    def release(self):
        self.buf = None


def _same_row(name, a, b, also=True):
    same = bool(torch.equal(a.view(torch.int16 if a.element_size() == 2 else torch.int32), b.view(torch.int16 if b.element_size() == 2 else torch.int32)))
    bad = 0.0 if same else float((a != b).sum())
    return dict(name=name, err=bad if also else max(bad, 1.0), tol=0.0, ok=same and also)


def _far_case_rows(name, run, fars, ref, tol=KTOL, other_family=()):
    """The rows of one kernel case: the plain ("near") launch against ``ref`` at ``tol``, then one launch per operand in ``fars`` with
    that operand far: far result == near result bit for bit and the decoys of the far operand untouched.  For an operand in
    ``other_family`` the far layout legitimately runs another kernel: that row compares with ``ref`` at ``tol`` instead."""
    why = far_skip_reason()
    if why is not None:
        return [_skip_row(f"{name}: near and {len(fars)} far launches", why)]
    f0 = _FarOperands(None)
    y_near = f0.result(run(f0))
    torch.cuda.synchronize()
    want = ref(y_near) if callable(ref) else ref
    rows = [_res(f"{name}: near vs reference", y_near, want, tol)]
    for which in fars:
        torch.cuda.reset_peak_memory_stats()
        f = _FarOperands(which)
        y = f.result(run(f))
        torch.cuda.synchronize()
        assert f.buf is not None, f"{name}: no operand called {which}"
        if which in other_family:
            r = _res(f"{name}: {which} far (another kernel: 64-bit fallback) vs reference", y, want, tol)
            r["ok"] = r["ok"] and f.intact()
            rows.append(r)
        else:
            rows.append(_same_row(f"{name}: {which} far == near, bit for bit, decoys untouched", y.contiguous(), y_near.contiguous(), f.intact()))
        FAR_PEAK[f"{name}: {which} far"] = torch.cuda.max_memory_allocated()
        f.release()
        del f, y
        torch.cuda.empty_cache()
    return rows


def far_skipped(rows):
    n = sum(1 for r in rows if r.get("skipped"))
    print(f"far operands: {n} of {len(rows)} rows skipped")
    return n


# ---- GEMM families
# (family, GEMM_FLAGS bits, LDS-DMA staging, naive, case).  Row counts M with (M - 1) between 2^k and 1.5 x 2^k, so that the far
# matrix stays inside FAR_CAP with a power-of-two leading dimension.
FAR_GEMM_FAMILIES = (("128-row reg", 4 | 16, False, False), ("128-row glds", 4 | 16, True, False), ("naive", 4 | 16, True, True),
                     ("persistent 192x320", 8, True, False), ("ping-pong 192", (1 << 17) | (1 << 19), True, False),
                     ("ping-pong 256", (1 << 17) | (1 << 20), True, False), ("one-wave-per-SIMD", 1 << 21, True, False),
                     ("stream-K", 1 << 27, True, False), ("LDS patch", 1 << 28, True, False), ("weight-stationary", 1024, True, False),
                     ("weight-stationary + LayerNorm", 1024, True, False), ("split-K", 0, True, False))


def far_gemm_specs(family):
    """[(case name, descriptor words for the planner, operands made far in turn)] of one family; ``check_far_gemm`` builds the data."""
    if family in ("128-row reg", "128-row glds", "naive"):
        return [("M130 N136 K128 +bias+rowvec/50+res", dict(mode=0, M=130, N=136, C0=128, rowvec_div=50, R=1, bias=1), ("A0", "C", "R", "rowvec")),
                ("two-source M130 N320 K128+64", dict(mode=0, M=130, N=320, C0=128, C1=64), ("A1",)),
                ("conv3x3 3 x 12x10 64->128 +bias+temb+res", dict(mode=1, M=360, N=128, C0=64, Hi=12, Wi=10, Ho=12, Wo=10, stride=1, rowvec_div=120, R=1, bias=1), ("A0",)),
                ("temporal B2 F5 HW17 64->64 +bias+res", dict(mode=2, M=170, N=64, C0=64, F=5, HW=17, R=1, bias=1), ("A0",))]
    if family in ("persistent 192x320", "ping-pong 192", "ping-pong 256", "one-wave-per-SIMD", "stream-K"):
        return [("M261 N640 K192 +bias+res", dict(mode=0, M=261, N=640, C0=192, R=1, bias=1), ("A0", "C", "R")),
                ("two-source M261 N640 K128+64 +bias+rowvec/100", dict(mode=0, M=261, N=640, C0=128, C1=64, rowvec_div=100, bias=1), ("A1", "rowvec"))]
    if family == "LDS patch":
        return [("conv3x3 5 x 16x16 64->320 +bias+res", dict(mode=1, M=1280, N=320, C0=64, Hi=16, Wi=16, Ho=16, Wo=16, stride=1, R=1, bias=1), ("A0", "C", "R")),
                ("conv3x3 5 x 16x16 64+64->320 +bias+temb", dict(mode=1, M=1280, N=320, C0=64, C1=64, Hi=16, Wi=16, Ho=16, Wo=16, stride=1, rowvec_div=512, bias=1),
                 ("A1", "rowvec"))]
    if family == "weight-stationary":
        return [("M130 N320 K320 +bias+res", dict(mode=0, M=130, N=320, C0=320, R=1, bias=1), ("A0", "C", "R"))]
    if family == "weight-stationary + LayerNorm":
        return [("M130 N160 K320 LayerNorm fold", dict(mode=0, M=130, N=160, C0=320, bias=1, ln=1), ("A0", "C"))]
    if family == "split-K":
        return [("conv3x3 40 x 8x8 256->320 +bias+temb+res M2560", dict(mode=1, M=2560, N=320, C0=256, Hi=8, Wi=8, Ho=8, Wo=8, stride=1, rowvec_div=1024, R=1, bias=1),
                 ("A0", "C", "R", "rowvec")),
                ("conv3x3 40 x 8x8 128+128->320 +bias+temb+res M2560", dict(mode=1, M=2560, N=320, C0=128, C1=128, Hi=8, Wi=8, Ho=8, Wo=8, stride=1, rowvec_div=1024,
                                                                            R=1, bias=1), ("A1",))]
    raise KeyError(family)


def far_gemm_operand_rows(words, which):
    """(rows, cols) of operand ``which`` of the launch ``words`` describes (A of a convolution has the INPUT rows: stride 1 here)."""
    M, N = words["M"], words["N"]
    return {"A0": (M, words["C0"]), "A1": (M, words.get("C1", 0)), "C": (M, N), "R": (M, N),
            "rowvec": ((M + words.get("rowvec_div", 1) - 1) // words.get("rowvec_div", 1), N)}[which]


def far_gemm_plan_rows():
    """(row name, descriptor line for tests/gemm_plan_main.cpp) of every near and far GEMM launch, in pairs: the planner must give
    both the same family (tests/test_far_operands_host.py)."""
    rows = []
    field = {"A0": "lda0", "A1": "lda1", "C": "ldc", "R": "ldr", "rowvec": "ldrv"}
    for fam, bits, glds, naive in FAR_GEMM_FAMILIES:
        for cname, words, fars in far_gemm_specs(fam):
            flags = (1 if naive else 0) | (2 if glds else 0) | bits
            base = " ".join(f"{k}={v}" for k, v in words.items() if k not in ("rowvec_div",)) + f" flags={flags}"
            if "rowvec_div" in words:
                base += f" rowvec=1 rowvec_div={words['rowvec_div']}"
            rows.append((f"{fam} | {cname} | near", base))
            for which in fars:
                r, _c = far_gemm_operand_rows(words, which)
                rows.append((f"{fam} | {cname} | {which} far", base + f" {field[which]}={far_ld(r)}"))
    return rows


def _far_gemm_data(words):
    M, N, C0, C1, mode = words["M"], words["N"], words["C0"], words.get("C1", 0), words["mode"]
    taps = {0: 1, 1: 9, 2: 3}[mode]
    K = taps * (C0 + C1)
    a0, a1 = rnd(M, C0, seed=M + 1), (rnd(M, C1, seed=M + 2) if C1 else None)
    w = rnd(N, K, scale=1 / math.sqrt(K), seed=N + 3)
    bias = rnd(N, seed=N + 4) if words.get("bias") else None
    div = words.get("rowvec_div", 0)
    rv = rnd((M + div - 1) // div, N, seed=N + 5) if div else None
    res = rnd(M, N, seed=M + 6) if words.get("R") else None
    kw = {}
    A = (a0 if a1 is None else torch.cat([a0, a1], 1)).double()
    if mode == 0:
        acc = A @ w.double().t()
    elif mode == 1:
        H, W_ = words["Hi"], words["Wi"]
        n = M // (H * W_)
        x = A.view(n, H, W_, C0 + C1).permute(0, 3, 1, 2)
        wk = w.double().view(N, 9, C0 + C1).permute(0, 2, 1).reshape(N, C0 + C1, 3, 3)
        acc = F.conv2d(x, wk, padding=1).permute(0, 2, 3, 1).reshape(M, N)
        kw = dict(mode=ops.MODE_CONV2D, conv=(H, W_, H, W_, 1, 0))
    else:
        Fr, HW = words["F"], words["HW"]
        B = M // (Fr * HW)
        x = A.view(B, Fr, HW, C0).permute(0, 2, 3, 1).reshape(B * HW, C0, Fr)
        wk = w.double().view(N, 3, C0).permute(0, 2, 1)
        acc = F.conv1d(x, wk, padding=1).view(B, HW, N, Fr).permute(0, 3, 1, 2).reshape(M, N)
        kw = dict(mode=ops.MODE_TEMPORAL, temporal=(Fr, HW))
    ln = None
    if words.get("ln"):
        gamma, beta = (1.0 + 0.3 * rnd(C0, seed=32).float()).half(), (0.2 * rnd(C0, seed=33).float()).half()
        a0 = (a0.float() * 1.5 + 2.0).half()
        acc = F.layer_norm(a0.double(), (C0,), gamma.double(), beta.double(), 1e-5) @ w.double().t()
        w, bias_f, c1 = ops.ln_fold(w, bias, gamma, beta)
        acc = acc + bias.double()
        bias, ln = bias_f, (c1, 1e-5)
    elif bias is not None:
        acc = acc + bias.double()
    if rv is not None:
        acc = acc + rv.double().repeat_interleave(div, 0)[:M]
    if res is not None:
        acc = acc + res.double()
    return dict(a0=a0, a1=a1, w=w, bias=bias, rv=rv, div=div, res=res, ln=ln, kw=kw, ref=acc)


def check_far_gemm(family):
    """One GEMM family with A0 / A1 / C / R / rowvec far in turn (``far_gemm_specs``); the stream-K and split-K workspace NaN-filled."""
    fam, bits, glds, naive = next(f for f in FAR_GEMM_FAMILIES if f[0] == family)
    out = []
    saved, saved_glds = ops.GEMM_FLAGS, ops.USE_GLDS
    try:
        ops.USE_GLDS = glds
        ops.GEMM_FLAGS = ((saved & ~4) | bits) if not bits & 4 else (saved | bits)
        for cname, words, fars in far_gemm_specs(fam):
            d = _far_gemm_data(words)
            M, N = words["M"], words["N"]

            def run(f, d=d, M=M, N=N):
                if fam in ("stream-K", "split-K"):
                    ops._workspace(DEV).fill_(float("nan"))
                return ops.gemm(f.mat("A0", d["a0"]), d["w"], a1=f.mat("A1", d["a1"]), bias=d["bias"], rowvec=f.mat("rowvec", d["rv"]),
                                rowvec_div=d["div"], residual=f.mat("R", d["res"]), out=f.mat("C", torch.empty(M, N, dtype=torch.float16, device=DEV), out=True),
                                naive=naive, ln=d["ln"], **d["kw"])
            out += _far_case_rows(f"far gemm[{fam}] {cname}", run, fars, d["ref"])
    finally:
        ops.GEMM_FLAGS, ops.USE_GLDS = saved, saved_glds
    return out


def check_far_ff_fused():
    """``ff_geglu`` with X, R and Y far (M = 161: one strip and a ragged tail)."""
    C, H, M = 320, 1280, 161
    w1, b1 = rnd(2 * H, C, scale=1 / math.sqrt(C)), rnd(2 * H, scale=0.1)
    w2, b2 = rnd(C, H, scale=1 / math.sqrt(H)), rnd(C, scale=0.1)
    w1p, b1p = _geglu_pack(w1, b1, H)
    w2s = ops.ff_pack_w2(w2)
    x, r = rnd(M, C, seed=M), rnd(M, C, seed=M + 1)
    proj = x.double() @ w1.double().t() + b1.double()
    hid = (proj[:, :H] * F.gelu(proj[:, H:])).half().double()
    ref = (hid @ w2.double().t() + b2.double()).half().double() + r.double()

    def run(f):
        return ops.ff_geglu(f.mat("X", x), w1p, b1p, w2s, b2, residual=f.mat("R", r), out=f.mat("Y", torch.empty(M, C, dtype=torch.float16, device=DEV), out=True))
    return _far_case_rows(f"far ff_fused M{M} +res", run, ("X", "R", "Y"), ref)


# ---- attention
FAR_ATTN_SEQ_ROWS = 512      # far through a sequence stride: batch element i, position s at row i + 512 s
FAR_ATTN_OUTER_ROWS = 4096   # far through the outer (batch) stride: row 4096 i + s


FLASH_LIMIT_LD = ((1 << 31) - 1 - 64) // 63 // 8 * 8     # 34 087 040: the largest kv_seq * ld, a multiple of 8, that fits


def flash_tile_offsets_fit(kv_seq, ldk, ldv):
    """Host mirror of the entry point's test: the largest K / V byte offset inside a 64-key tile fits 32 bits."""
    return kv_seq >= 0 and (63 * kv_seq * max(ldk, ldv) + 64) * 2 < (1 << 32)


def _fa(name, kernel, fars, *, batch, heads, Sq, Sk, d=64, qk_mod=0, causal=False, bias=False, naive=False, flags=0, only=None):
    return dict(name=name, kernel=kernel, fars=fars, batch=batch, heads=heads, Sq=Sq, Sk=Sk, d=d, qk_mod=qk_mod, causal=causal, bias=bias,
                naive=naive, flags=flags, only=only)


def far_attention_specs():
    """Every attention case: ``fars`` = (operand, "seq" | "outer") pairs made far in turn.  Sk = 40: one ragged tile; Sk = 88: a full and
    a ragged tile (K / V far through kv_seq below the flash kernels' limit: 104 keys at a power-of-two stride of 2^25 elements would
    span 6.4 GiB behind the 4 GiB lead); Sk = 104 with Q / O far.  Far K / V through kv_seq at Sk = 40 exceeds the limit (2^26
    elements per key) and takes the 64-bit fallback."""
    S = "seq"
    return [
        _fa("flash 4-wave b3 h2 Sq130 Sk40", "4-wave flash", (("Q", S), ("K", S), ("V", S), ("O", S), ("K", "outer"), ("Q", "outer")), batch=3, heads=2, Sq=130, Sk=40),
        _fa("flash 4-wave b1 h1 Sq130 Sk70 at the limit of the 32-bit tile offsets", "4-wave flash", (("K", "limit"), ("K", "limit+8"), ("V", "limit"), ("V", "limit+8")),
            batch=1, heads=1, Sq=130, Sk=70),
        _fa("flash 4-wave b2 h2 Sq130 Sk88", "4-wave flash", (("K", S), ("V", S)), batch=2, heads=2, Sq=130, Sk=88),
        _fa("flash 4-wave b2 h2 Sq130 Sk104", "4-wave flash", (("Q", S), ("O", S)), batch=2, heads=2, Sq=130, Sk=104),
        _fa("flash 8-wave b264 h1 Sq1024 Sk2100", "8-wave", (("K", S), ("V", "outer")), batch=264, heads=1, Sq=1024, Sk=2100, only=(0, 263)),
        _fa("PnP shared-softmax 4-wave b3 h2 S130", "shared-softmax 4-wave", (("K", S), ("V", S), ("O", S), ("V", "outer")), batch=3, heads=2, Sq=130, Sk=130, qk_mod=1),
        _fa("PnP shared-softmax 4-wave b3 h2 Sq130 Sk40", "shared-softmax 4-wave", (("K", S), ("V", S)), batch=3, heads=2, Sq=130, Sk=40, qk_mod=1),
        _fa("PnP shared-softmax 8-wave b129 h3 Sq2048 Sk2100", "shared-softmax 8-wave", (("V", S), ("K", "outer")), batch=129, heads=3, Sq=2048, Sk=2100,
            qk_mod=43, only=(0, 43, 128)),
        _fa("short one-wave b5 h2 S12", "short one-wave", (("Q", S), ("K", S), ("V", S), ("O", S), ("V", "outer")), batch=5, heads=2, Sq=12, Sk=12),
        _fa("short one-wave PnP b6 h2 S12", "short one-wave PnP", (("K", S), ("V", S), ("O", S), ("K", "outer")), batch=6, heads=2, Sq=12, Sk=12, qk_mod=2),
        _fa("whole-sequence MFMA b3 h2 S40 d80", "whole-sequence MFMA", (("Q", S), ("K", S), ("V", S), ("O", S), ("K", "outer")), batch=3, heads=2, Sq=40, Sk=40, d=80),
        _fa("whole-sequence MFMA causal b3 h2 S40 d64", "whole-sequence MFMA", (("K", S), ("V", S)), batch=3, heads=2, Sq=40, Sk=40, causal=True),
        _fa("96-key loop b3 h2 S330 d80", "96-key loop", (("K", S), ("V", S), ("O", S), ("K", "outer")), batch=3, heads=2, Sq=330, Sk=330, d=80),
        _fa("96-key loop causal b2 h1 S330 d64", "96-key loop", (("K", S), ("Q", S)), batch=2, heads=1, Sq=330, Sk=330, causal=True),
        _fa("score bias b3 h2 Sq20 Sk40 d40", "bias", (("K", S), ("V", S), ("O", "outer")), batch=3, heads=2, Sq=20, Sk=40, d=40, bias=True),
        _fa("score bias (generic kernel) b2 h2 Sq33 Sk130 d40", "bias", (("K", S),), batch=2, heads=2, Sq=33, Sk=130, d=40, bias=True),
        _fa("generic kernel b3 h2 Sq33 Sk40", "generic", (("Q", S), ("K", S), ("V", S), ("O", S), ("K", "outer")), batch=3, heads=2, Sq=33, Sk=40, naive=True),
    ]


def far_attention_layout(spec, which, via):
    """The far launch of ``spec`` with ``which`` far through ``via``: the pair that shares strides with ``which`` (Q / O, K / V) lies on
    the sparse row pattern; ``which`` gets the power-of-two leading dimension that puts its last row at or past 2^32 bytes.
    -> dict(strides of the pair, ld of ``which``, S, nb, geometry)."""
    import numpy as np
    pair_q = which in ("Q", "O")
    S = spec["Sq"] if pair_q else spec["Sk"]
    nb = spec["batch"]
    if via.startswith("limit"):
        # one key per row, the leading dimension at the last value the flash kernels' 32-bit tile offsets hold (kv_seq * ld = 34 087 040
        # elements, a multiple of 8) and 8 elements past it: the entry point's test, pinned on both sides of its edge
        assert not pair_q and nb == 1
        strides = (S, 0, 1)
        ld = FLASH_LIMIT_LD + (8 if via.endswith("+8") else 0)
    elif via == "seq":
        assert nb <= FAR_ATTN_SEQ_ROWS
        strides = (1, 0, FAR_ATTN_SEQ_ROWS)
        ld = far_ld(S) // FAR_ATTN_SEQ_ROWS            # (S - 1) * seq * ld >= 2^31 elements
    else:
        assert S <= FAR_ATTN_OUTER_ROWS and nb >= 3
        strides = (FAR_ATTN_OUTER_ROWS, 0, 1)
        ld = far_ld(nb) // FAR_ATTN_OUTER_ROWS
    C = spec["heads"] * spec["d"]
    assert ld >= C and ld % 8 == 0
    i, s = np.arange(nb, dtype=np.int64)[:, None], np.arange(S, dtype=np.int64)[None]
    rows = (i * strides[0] + s * strides[2]).reshape(-1)
    geo = far_geometry(f"{spec['name']}: {which} far via {via}", rows * ld, C, 2, **({} if via.startswith("limit") else dict(ld=ld)))
    fallback = spec["kernel"] in ("4-wave flash", "8-wave", "shared-softmax 4-wave", "shared-softmax 8-wave") and not pair_q and \
        not flash_tile_offsets_fit(strides[2], ld, C)
    return dict(strides=strides, ld=ld, S=S, nb=nb, rows=rows, geo=geo, pair_q=pair_q, fallback=fallback)


def _far_attn_case(spec):
    why = far_skip_reason()
    name = f"far attention[{spec['kernel']}] {spec['name']}"
    if why is not None:
        return [_skip_row(f"{name}: near and {len(spec['fars'])} far launches", why)]
    b, h, Sq, Sk, d = spec["batch"], spec["heads"], spec["Sq"], spec["Sk"], spec["d"]
    C = h * d
    seed = Sq + Sk + d
    data = dict(Q=rnd(b * Sq, C, seed=seed + 1), K=rnd(b * Sk, C, seed=seed + 2), V=rnd(b * Sk, C, seed=seed + 3))
    bias = torch.randn(h, Sq, Sk, generator=torch.Generator().manual_seed(Sk)).to(DEV) if spec["bias"] else None
    kw = dict(batch=b, heads=h, Sq=Sq, Sk=Sk, inner=1, qk_mod=spec["qk_mod"])
    extra = {} if d == 64 and not spec["causal"] and bias is None else dict(scale=d ** -0.5, head_dim=d, causal=spec["causal"])
    near = dict(q_strides=(Sq, 0, 1), kv_strides=(Sk, 0, 1))
    saved, ops.ATTN_FLAGS = ops.ATTN_FLAGS, ops.ATTN_FLAGS | spec["flags"]
    try:
        o = _poison((b * Sq, C), torch.float16)
        y_near = ops.attention(data["Q"], data["K"], data["V"], o, naive=spec["naive"], bias=bias, **kw, **near, **extra)
        torch.cuda.synchronize()
        rows_ref, ref = _attn_ref(data["Q"], data["K"], data["V"], d=d, causal=spec["causal"], bias=bias, only=spec["only"], **kw, **near)
        out = [_res(f"{name}: near vs reference", y_near[rows_ref], ref, KTOL)]
        for which, via in spec["fars"]:
            torch.cuda.reset_peak_memory_stats()
            L = far_attention_layout(spec, which, via)
            idx = torch.from_numpy(L["rows"]).to(DEV)
            n_rows = int(L["rows"].max()) + 1
            ops_t, buf = {}, None
            for nm in ("Q", "O") if L["pair_q"] else ("K", "V"):
                src = _poison((b * Sq, C), torch.float16) if nm == "O" else data[nm]
                if nm == which:
                    buf = _FarBuffer(L["geo"], torch.float16, seed=seed)
                    buf.write(src)
                    ops_t[nm] = buf.view((n_rows, C), (L["ld"], 1))
                else:
                    m = torch.empty(n_rows, C, dtype=torch.float16, device=DEV)
                    m[idx] = src
                    ops_t[nm] = m
            for nm in ("K", "V") if L["pair_q"] else ("Q", "O"):
                ops_t[nm] = _poison((b * Sq, C), torch.float16) if nm == "O" else data[nm]
            st = dict(near)
            st["q_strides" if L["pair_q"] else "kv_strides"] = L["strides"]
            ops.attention(ops_t["Q"], ops_t["K"], ops_t["V"], ops_t["O"], naive=spec["naive"], bias=bias, **kw, **st, **extra)
            torch.cuda.synchronize()
            y = buf.read() if which == "O" else (ops_t["O"][idx] if L["pair_q"] else ops_t["O"])
            tag = f"{name}: {which} far via {via}"
            if L["fallback"]:
                r = _res(f"{tag} (beyond the flash kernels' limit: 64-bit fallback) vs reference", y[rows_ref], ref, KTOL)
                r["ok"] = r["ok"] and buf.decoys_intact()
                out.append(r)
            else:
                out.append(_same_row(f"{tag} == near, bit for bit, decoys untouched", y.contiguous(), y_near, buf.decoys_intact()))
            FAR_PEAK[tag] = torch.cuda.max_memory_allocated()
            del buf, ops_t, y, idx
            torch.cuda.empty_cache()
    finally:
        ops.ATTN_FLAGS = saved
    return out


def check_far_attention(kernel):
    out = []
    for spec in far_attention_specs():
        if spec["kernel"] == kernel or (kernel == "short one-wave" and spec["kernel"] == "short one-wave PnP"):
            out += _far_attn_case(spec)
    return out


def check_attention_negative_kv_seq():
    """kv_seq = -1 (K / V handed over at their last key, walked backwards): the flash kernels' unsigned tile offsets cannot hold it, the
    entry point takes the 64-bit kernels.  softmax(Q K^T) V does not depend on the order of the keys: the reference is the plain one."""
    b, h, Sq, Sk = 2, 2, 130, 70
    C = 64 * h
    q, k, v = rnd(b * Sq, C, seed=1), rnd(b * Sk, C, seed=2), rnd(b * Sk, C, seed=3)
    kw = dict(batch=b, heads=h, Sq=Sq, Sk=Sk, inner=1, q_strides=(Sq, 0, 1))
    rows, ref = _attn_ref(q, k, v, kv_strides=(Sk, 0, 1), **kw)
    o = _poison((b * Sq, C), torch.float16)
    ops.attention(q, k[Sk - 1:], v[Sk - 1:], o, kv_strides=(Sk, 0, -1), **kw)
    torch.cuda.synchronize()
    return [_res(f"attention b{b} h{h} Sq{Sq} Sk{Sk}, kv_seq = -1 (64-bit fallback) vs reference", o[rows], ref, KTOL)]


def check_attention_wide_exit_to_generic():
    """The exit of ``anyv2v_attention_f16`` that leaves the flash kernels for the one-thread-per-query kernel: a layout their 32-bit tile
    offsets cannot hold (kv_seq = -1) with more batch elements than the loop kernel's grid takes (65536 > 65535).  Two queries and two keys
    per element; flag bit1 keeps the short one-wave kernel, which comes first at <= 16 positions, out of the way."""
    b, h, Sq, Sk = WIDE_GENERIC_SHAPE
    C = 64 * h
    q, k, v = rnd(b * Sq, C, seed=11), rnd(b * Sk, C, seed=12), rnd(b * Sk, C, seed=13)
    kw = dict(batch=b, heads=h, Sq=Sq, Sk=Sk, inner=1, q_strides=(Sq, 0, 1))
    rows, ref = _attn_ref(q, k, v, kv_strides=(Sk, 0, 1), **kw)
    o = _poison((b * Sq, C), torch.float16)
    saved, ops.ATTN_FLAGS = ops.ATTN_FLAGS, ops.ATTN_FLAGS | 2
    try:
        ops.attention(q, k[Sk - 1:], v[Sk - 1:], o, kv_strides=(Sk, 0, -1), **kw)
    finally:
        ops.ATTN_FLAGS = saved
    torch.cuda.synchronize()
    return [_res(f"attention b{b} h{h} Sq{Sq} Sk{Sk}, kv_seq = -1, batch > 65535 (generic kernel) vs reference", o[rows], ref, KTOL)]


WIDE_GENERIC_SHAPE = (65536, 1, 2, 2)   # batch, heads, Sq, Sk


def forced_rescale_8wave_specs():
    """The smallest 8-wave shapes of ``exact_attention_specs`` with spiked keys (second tile, middle, ragged last tile), as in
    ``check_attention_forced_rescale``: (name, instantiation, launch shape, spiked keys, gain, batch elements compared)."""
    return (("plain b64 h4 Sq1024 Sk2100 kv_div64", "flash<3,1,8>", dict(batch=64, heads=4, Sq=1024, Sk=2100, kv_div=64, qk_mod=0), [70, 1029, 2099], 6.0, (0, 63)),
            ("shared-softmax b96 h4 S2100 qk_mod32", "flash<3,3,8>", dict(batch=96, heads=4, Sq=2100, Sk=2100, kv_div=1, qk_mod=32), [70, 1029, 2099], 6.0, (0, 95)))


def _rescale8_strides(shape):
    return dict(inner=1, q_strides=(shape["Sq"], 0, 1), kv_strides=(shape["Sk"], 0, 1))


def check_attention_forced_rescale_8wave():
    """``check_attention_forced_rescale`` on the 8-wave instantiations of the flash kernel: keys whose score for one query row dwarfs the
    rest force the textbook path (true maximum, rescale of O and l, re-exponentiation) after the first step.  Reference: fp32 SDPA on the
    same fp16 inputs, two batch elements (every head)."""
    out = []
    for name, inst, shape, keys, gain, only in forced_rescale_8wave_specs():
        b, h, Sq, Sk = shape["batch"], shape["heads"], shape["Sq"], shape["Sk"]
        C = 64 * h
        n_kv = b // shape["kv_div"]
        g = torch.Generator(device=DEV).manual_seed(Sq + Sk)
        new = lambda M, W: torch.randn(M, W, device=DEV, generator=g).half()
        if Sq == Sk and shape["kv_div"] == 1:
            t = new(b * Sq, 3 * C)
            q, k, v = t[:, :C], t[:, C:2 * C], t[:, 2 * C:]
        else:
            t = new(n_kv * Sk, 2 * C)
            q, k, v = new(b * Sq, C), t[:, :C], t[:, C:]
        qv, kvw = q.view(b, Sq, h, 64), k.view(n_kv, Sk, h, 64)
        for n, key in enumerate(keys):      # in turn for the compared elements: a key of the K the element reads follows one of the query rows it reads
            src = only[n % len(only)] % shape["qk_mod"] if shape["qk_mod"] else only[n % len(only)]
            kvw[src // shape["kv_div"], key] = (gain * qv[src, (7 + 13 * n) % Sq].float()).half()
        o = torch.zeros(b * Sq, C, dtype=torch.float16, device=DEV)
        kw = dict(shape, **_rescale8_strides(shape))
        ops.attention(q, k, v, o, **kw)
        rows, ref = _attn_ref(q, k, v, only=list(only), **kw)
        out.append(_res(f"attn[{inst}] forced rescale: spikes at keys {keys}, {name}, elements {only} vs fp32 SDPA", o[rows], ref, KTOL))
        del t, q, k, v, o, ref
    return out


def named_attention_plan_rows():
    """(row name, line for tests/attention_plan_main.cpp, kernel named, instantiation named or None) of the launches that the random-data
    checks name by kernel: ``check_attention_small_mfma``, ``check_attention_forced_rescale`` (and its 8-wave twin),
    ``check_attention_bias_and_rotary_windows``, the kernel-naming rows of ``check_attention``, ``check_attention_negative_kv_seq`` and
    ``check_attention_wide_exit_to_generic``.  The operands are the column windows those checks cut, on the device "meta"."""
    rows = []
    new = lambda M, W: torch.empty(M, W, dtype=torch.float16, device="meta")

    def fused(Mq, C):
        t = new(Mq, 3 * C)
        return t[:, :C], t[:, C:2 * C], t[:, 2 * C:], new(Mq, C)

    def q_kv(Mq, Mk, C):
        t = new(Mk, 2 * C)
        return new(Mq, C), t[:, :C], t[:, C:], new(Mq, C)

    def add(name, kernel, inst, tensors, **kw):
        rows.append((name, attn_plan_words(*tensors, **kw), kernel, inst))
    sp = lambda S, Sk=None: dict(inner=1, q_strides=(S, 0, 1), kv_strides=(S if Sk is None else Sk, 0, 1))
    for (B, h, S, d, causal, kernel) in attention_small_mfma_specs():
        add(f"small mfma | B{B} h{h} S{S} d{d} causal={causal}", kernel, None, fused(B * S, h * d), batch=B, heads=h, Sq=S, Sk=S, scale=d ** -0.5,
            head_dim=d, causal=causal, **sp(S))
    Bc, Fr, HW, h, d = 2, 16, 48, 8, 40          # its temporal layout row: 16 queries x 24 keys
    add("small mfma | temporal layout 8 x 40", "whole-sequence MFMA", "small<2,6>", q_kv(Bc * Fr * HW, Bc * HW * (Fr + 8), h * d), batch=Bc * HW, heads=h,
        Sq=Fr, Sk=Fr + 8, inner=HW, q_strides=(Fr * HW, 1, HW), kv_strides=(HW * (Fr + 8), Fr + 8, 1), scale=d ** -0.5, head_dim=d)
    for name, S, Sk, _build in forced_rescale_specs():
        add(f"forced rescale | flash: {name}", "4-wave flash", "flash<2,1,4>", q_kv(2 * S, 2 * Sk, 128), batch=2, heads=2, Sq=S, Sk=Sk, **sp(S, Sk))
        if S == Sk:
            add(f"forced rescale | shared softmax: {name}", "shared-softmax 4-wave", "flash<2,3,4>", fused(3 * S, 128), batch=3, heads=2, Sq=S, Sk=S,
                qk_mod=1, **sp(S))
    for name, inst, shape, _keys, _gain, _only in forced_rescale_8wave_specs():
        b, Sq, Sk, C = shape["batch"], shape["Sq"], shape["Sk"], 64 * shape["heads"]
        tensors = fused(b * Sq, C) if Sq == Sk and shape["kv_div"] == 1 else q_kv(b * Sq, b // shape["kv_div"] * Sk, C)
        add(f"forced rescale 8-wave | {name}", "8-wave", inst, tensors, **shape, **_rescale8_strides(shape))
    for (heads, D, Fr, inst) in attention_bias_specs():
        B, HW = 3, 10
        for qk_mod in (0, B * HW // 3):
            add(f"score bias | {heads} x {D}, {Fr} frames, qk_mod {qk_mod}", "bias", inst, fused(B * Fr * HW, heads * D), batch=B * HW, heads=heads, Sq=Fr,
                Sk=Fr, inner=HW, q_strides=(Fr * HW, 1, HW), kv_strides=(Fr * HW, 1, HW), qk_mod=qk_mod, scale=D ** -0.5, head_dim=D, bias=True)
    for (b, h, S) in ATTN_PNP_SHARED_SHAPES:
        for flag, kernel, inst in ((0, "shared-softmax 4-wave", "flash<2,3,4>"), (8, "4-wave flash", "flash<2,1,4>")):
            add(f"check_attention | PnP shared-softmax b{b} h{h} S{S} flags {flag}", kernel, inst, fused(b * S, 64 * h), batch=b, heads=h, Sq=S, Sk=S,
                qk_mod=b // 3, flags=flag, **sp(S))
    for key, qk, plans in (("shared-softmax", True, ((0, "shared-softmax 8-wave", "flash<3,3,8>"), (8, "8-wave", "flash<3,1,8>"))),
                           ("shared-softmax, ragged", True, ((0, "shared-softmax 8-wave", "flash<3,3,8>"), (8, "8-wave", "flash<3,1,8>"))),
                           ("plain", False, ((0, "8-wave", "flash<3,1,8>"), (4, "4-wave flash", "flash<2,1,4>")))):
        b, h, S = ATTN_8WAVE_SHAPES[key]
        for flag, kernel, inst in plans:
            add(f"check_attention | 8-wave blocks, {key} b{b} h{h} S{S} flags {flag}", kernel, inst, fused(b * S, 64 * h), batch=b, heads=h, Sq=S, Sk=S,
                qk_mod=b // 3 if qk else 0, flags=flag, **sp(S))
    for (b, h, S, Sk, kv_div, qk_mod) in ATTN_FLASH_KV_LOOP_SHAPES:
        add(f"check_attention | attn[flash] b{b} h{h} S{S} Sk{Sk} kv_div{kv_div} qk_mod{qk_mod}", "4-wave flash", "flash<2,1,4>",
            q_kv(b * S, (b // kv_div) * Sk, 64 * h), batch=b, heads=h, Sq=S, Sk=Sk, kv_div=kv_div, qk_mod=qk_mod, **sp(S, Sk))
    # kv_seq = -1: K / V handed over at their last key (row Sk - 1 of a [b Sk, C] matrix)
    b, h, Sq, Sk = 2, 2, 130, 70
    last = lambda Mk, C: new(Mk, C)[Sk - 1:]
    add("negative kv_seq | b2 h2 Sq130 Sk70", "64-bit fallback", "loop<2>", (new(b * Sq, 64 * h), last(b * Sk, 64 * h), last(b * Sk, 64 * h), new(b * Sq, 64 * h)),
        batch=b, heads=h, Sq=Sq, Sk=Sk, inner=1, q_strides=(Sq, 0, 1), kv_strides=(Sk, 0, -1))
    b, h, Sq, Sk = WIDE_GENERIC_SHAPE
    for flag, kernel, inst in ((2, "generic", "naive"), (0, "short one-wave", "short<1>")):     # without bit1 the short kernel takes two positions first
        add(f"wide exit to the generic kernel | b{b} h{h} Sq{Sq} Sk{Sk} flags {flag}", kernel, inst,
            (new(b * Sq, 64 * h), last(b * Sk, 64 * h), last(b * Sk, 64 * h), new(b * Sq, 64 * h)), batch=b, heads=h, Sq=Sq, Sk=Sk, inner=1,
            q_strides=(Sq, 0, 1), kv_strides=(Sk, 0, -1), flags=flag)
    return rows


def far_attention_plan_rows():
    """(row name, line for tests/attention_plan_main.cpp, kernel named, instantiation named or None, fallback) of every launch of
    ``check_far_attention``: the near launch of each spec and each far one, with the leading dimension and strides ``far_attention_layout``
    gives the far operand (a far buffer's pointer lies a multiple of 16 bytes into its allocation)."""
    rows = []
    for spec in far_attention_specs():
        b, h, Sq, Sk, d = spec["batch"], spec["heads"], spec["Sq"], spec["Sk"], spec["d"]
        C = h * d
        kw = dict(batch=b, heads=h, Sq=Sq, Sk=Sk, inner=1, qk_mod=spec["qk_mod"], naive=spec["naive"], bias=spec["bias"], flags=spec["flags"])
        if not (d == 64 and not spec["causal"] and not spec["bias"]):
            kw.update(scale=d ** -0.5, head_dim=d, causal=spec["causal"])
        near = dict(q_strides=(Sq, 0, 1), kv_strides=(Sk, 0, 1))
        mat = lambda M, ld=C: torch.empty_strided((M, C), (ld, 1), dtype=torch.float16, device="meta")
        base = f"far | {spec['kernel']}: {spec['name']}"
        rows.append((base + " | near", attn_plan_words(mat(b * Sq), mat(b * Sk), mat(b * Sk), mat(b * Sq), **kw, **near), spec["kernel"], None, False))
        for which, via in spec["fars"]:
            L = far_attention_layout(spec, which, via)
            assert L["geo"]["lead"] % 16 == 0
            n_rows = int(L["rows"].max()) + 1
            t = dict(Q=mat(b * Sq), K=mat(b * Sk), V=mat(b * Sk), O=mat(b * Sq))
            for nm in ("Q", "O") if L["pair_q"] else ("K", "V"):
                t[nm] = mat(n_rows, L["ld"] if nm == which else C)
            st = dict(near)
            st["q_strides" if L["pair_q"] else "kv_strides"] = L["strides"]
            rows.append((f"{base} | {which} far via {via}", attn_plan_words(t["Q"], t["K"], t["V"], t["O"], **kw, **st),
                         "64-bit fallback" if L["fallback"] else spec["kernel"], None, L["fallback"]))
    return rows


FAR_ATTN_KERNELS = ("4-wave flash", "8-wave", "shared-softmax 4-wave", "shared-softmax 8-wave", "short one-wave", "whole-sequence MFMA", "96-key loop",
                    "bias", "generic")


# ---- layout and elementwise kernels with a leading dimension
FAR_LAYOUT_M = 161     # rows of the far matrices below: (M - 1) * 2^24 elements = 5 GiB of fp16
FAR_LAYOUT_CASES = ("copy_cols", "gather_rows", "rotary", "ncfhw_to_tokens", "tokens_to_ncfhw", "softmax_rows", "cfg_ddim_step", "freeu", "tile_blend")
FAR_FREEU = (2, 9, 9, 16, 8)            # n_img, H, W, C_hidden, C_skip: 162 rows
FAR_TILE_ROWS = 1281                    # rows of the far tile matrix (the stitch of 2 images of 14 x 20 needs 936: the last tile lies at its end)


def far_layout_geometries():
    """(name, rows, cols, item) of every far matrix the layout cases make (``far_matrix_geometry``)."""
    M = FAR_LAYOUT_M
    return [("copy_cols x", M, 24, 2), ("copy_cols y", M, 32, 2), ("gather_rows x", M, 16, 2), ("gather_rows y", M, 16, 2), ("rotary x", M, 64, 2),
            ("ncfhw_to_tokens y", 2 * 3 * 30, 16, 2), ("tokens_to_ncfhw x", 2 * 3 * 30, 16, 2), ("softmax_rows s", 5, 257, 4), ("softmax_rows p", 5, 257, 2),
            ("cfg_ddim_step v", 3 * 3 * 20, 8, 2), ("freeu hidden", 162, 16, 2), ("freeu hidden'", 162, 16, 2), ("freeu skip", 162, 8, 2),
            ("freeu skip'", 162, 8, 2), ("tile_blend tiles", FAR_TILE_ROWS, 8, 2)]


def check_far_layout(case):
    M = FAR_LAYOUT_M
    if case == "copy_cols":
        x, pre = rnd(M, 24, seed=1), rnd(M, 32, seed=2)
        want = pre.clone()
        want[:, 5:18] = x[:, 3:16]
        return _far_case_rows("far copy_cols x[:, 3:16] -> y[:, 5:18]", lambda f: ops.copy_cols(f.mat("x", x), 3, f.mat("y", pre, out=True, inplace=True), 5, 13),
                              ("x", "y"), want.double(), 0.0)
    if case == "gather_rows":
        src, pre = rnd(M, 16, seed=3), rnd(M, 16, seed=4)
        idx = torch.randint(0, M, (M,), generator=torch.Generator().manual_seed(5)).to(torch.int32)
        idx[:3] = torch.tensor([M - 1, 0, M - 1])      # the far row is named first and last
        idx[-1] = M - 1
        idx = idx.to(DEV)
        want = pre.clone()
        want[:, 8:16] = src[idx.long(), 8:16]
        return _far_case_rows("far gather_rows", lambda f: ops.gather_rows(f.mat("x", src), 8, idx, f.mat("y", pre, out=True, inplace=True), 8, 8),
                              ("x", "y"), want.double(), 0.0)
    if case == "rotary":
        x = rnd(M, 64, seed=6)
        rot, n_pos, rpp, theta = 32, 7, 5, 10000.0
        pos = ((torch.arange(M, device=DEV) // rpp) % n_pos).double()
        ang = pos[:, None] * theta ** (-torch.arange(0, rot, 2, device=DEV).double() / rot)[None]
        xr = x.double().clone()
        a, b = xr[:, 8:8 + rot:2].clone(), xr[:, 9:9 + rot:2].clone()
        xr[:, 8:8 + rot:2], xr[:, 9:9 + rot:2] = a * ang.cos() - b * ang.sin(), a * ang.sin() + b * ang.cos()
        return _far_case_rows("far rotary cols 8..40", lambda f: ops.rotary(f.mat("x", x, out=True, inplace=True), 8, rot, rpp, n_pos, theta), ("x",), xr, KTOL)
    if case in ("ncfhw_to_tokens", "tokens_to_ncfhw"):
        B, C, Fr, H, W = 2, 9, 3, 5, 6
        lat, pre = rnd(B, C, Fr, H, W, seed=7), rnd(B * Fr * H * W, 16, seed=8)
        tok = pre.clone()
        tok[:, 4:4 + C] = lat.permute(0, 2, 3, 4, 1).reshape(-1, C)
        if case == "ncfhw_to_tokens":
            return _far_case_rows("far ncfhw_to_tokens -> tokens[:, 4:13]", lambda f: ops.ncfhw_to_tokens(lat, f.mat("y", pre, out=True, inplace=True), col0=4),
                                  ("y",), tok.double(), 0.0)
        return _far_case_rows("far tokens_to_ncfhw <- tokens[:, 4:13]",
                              lambda f: ops.tokens_to_ncfhw(f.mat("x", tok), B, C, Fr, H, W, col0=4).reshape(B * C, -1), ("x",), lat.double().reshape(B * C, -1), 0.0)
    if case == "softmax_rows":
        s = (torch.randn(5, 257, generator=torch.Generator().manual_seed(9)) * 3.0).to(DEV)
        sc = 0.044194173824159216
        return _far_case_rows("far softmax_rows 5 x 257", lambda f: ops.softmax_rows(f.mat("s", s), sc, out=f.mat("p", torch.empty(5, 257, dtype=torch.float16, device=DEV), out=True)),
                              ("s", "p"), torch.softmax(sc * s.double(), 1), KTOL)
    if case == "cfg_ddim_step":
        Fr, H, W, C = 3, 4, 5, 4
        vt, latx = rnd(3 * Fr * H * W, 8, seed=10), rnd(1, C, Fr, H, W, seed=11)
        cf = torch.tensor((0.8, 0.6, 0.9, math.sqrt(1 - 0.81)), dtype=torch.float32, device=DEV)
        c = [float(t) for t in cf]
        vv = vt[:, :C].double().view(3, Fr, H * W, C).permute(0, 3, 1, 2).reshape(3, C, Fr, H, W)
        v = _h(vv[0].float() + _h(7.5 * _h(vv[2].float() - vv[0].float()))).double()   # the kernel's fp16 CFG rounding points
        xx = latx.double()[0]
        ref = c[2] * (c[0] * xx - c[1] * v) + c[3] * (c[0] * v + c[1] * xx)
        return _far_case_rows("far cfg_ddim_step b_unc 0, b_cond 2 (the last branch's rows are the far ones)",
                              lambda f: ops.cfg_ddim_step(f.mat("v", vt), 0, 2, 7.5, cf, latx, torch.empty_like(latx))[0].reshape(C, -1), ("v",), ref.reshape(C, -1), KTOL)
    if case == "freeu":
        import freeu_spec
        n_img, H, W, Ch, Cs = FAR_FREEU
        rows, b_, s_ = n_img * H * W, 1.2, 0.9
        g = torch.Generator().manual_seed(77)
        hidden, skip = (1.5 * torch.randn(rows, Ch, generator=g) + 2).half(), (1.5 * torch.randn(rows, Cs, generator=g) + 2).half()
        ref_h, ref_s = freeu_spec.freeu_tokens_reference(hidden, skip, n_img, H, W, b_, s_, dtype=torch.float64)
        hd, sd = hidden.to(DEV), skip.to(DEV)

        def run(f):
            ho, so = ops.freeu(f.mat("hidden", hd), f.mat("skip", sd), n_img, H, W, b_, s_,
                               out=(f.mat("hidden'", torch.empty(rows, Ch, dtype=torch.float16, device=DEV), out=True),
                                    f.mat("skip'", torch.empty(rows, Cs, dtype=torch.float16, device=DEV), out=True)))
            if f.which == "hidden'":
                ho = f.buf.read()
            if f.which == "skip'":
                so = f.buf.read()
            f.is_out = False      # both outputs are returned, joined: the far one is already read back
            return torch.cat([ho, so], 1)
        return _far_case_rows(f"far freeu {n_img} x {H}x{W} C{Ch} / C{Cs}", run, ("hidden", "skip", "hidden'", "skip'"),
                              torch.cat([ref_h.double(), ref_s.double()], 1), KTOL)
    if case == "tile_blend":
        import vae_tiling_spec as vts
        from anyv2v_amd.vae_tiling import AxisPlan, StitchPlan
        p, size, n_img, C = vts.DEC, (14, 20), 2, 8
        plan = StitchPlan(AxisPlan(size[0], **p), AxisPlan(size[1], **p))
        g = torch.Generator().manual_seed(14020)
        tiles = [[torch.randn(n_img, C, th, tw, generator=g).half() for tw in plan.ax.sizes] for th in plan.ay.sizes]
        want = vts.stitch([[t.double() for t in r] for r in tiles], p["e"], p["limit"], crop=(plan.H, plan.W))
        bases, rows = [], 0
        for th in plan.ay.sizes:
            bases.append([])
            for tw in plan.ax.sizes:
                bases[-1].append(rows)
                rows += n_img * th * tw
        assert rows <= FAR_TILE_ROWS
        bases[-1][-1] = FAR_TILE_ROWS - n_img * plan.ay.sizes[-1] * plan.ax.sizes[-1]     # the last tile ends on the matrix's last row
        raw = torch.full((FAR_TILE_ROWS, 8), float("nan"), dtype=torch.float16)
        for ty, r in enumerate(tiles):
            for tx, t in enumerate(r):
                m = t.shape[0] * t.shape[2] * t.shape[3]
                raw[bases[ty][tx]:bases[ty][tx] + m, :C] = t.permute(0, 2, 3, 1).reshape(m, C)
        raw = raw.to(DEV)
        # one rounding of an fp64 sum: within one fp16 ulp of the exact value, i.e. 2^-10 of it
        return _far_case_rows("far tile_blend 2 x 14x20 C8 (tile_rows 1281)", lambda f: ops.tile_blend(f.mat("tiles", raw), C, plan, bases, n_img).reshape(n_img * C, -1),
                              ("tiles",), want.reshape(n_img * C, -1), 2.0 ** -10)
    raise KeyError(case)


# ---- norms: no leading dimension in the ABI, so the source itself is 4 GiB (M * C just past 2^31 elements) and so is the output
FAR_NORM_ENTRIES = ("groupnorm", "groupnorm pivot entry points", "groupnorm_from_stats", "layernorm")
FAR_NORM_SHAPE = (2, 13 << 18, 320, 32)     # statistics groups, rows per group (13 reference chunks of 2^18 rows), C, G: M * C = 2^31 + 33 554 432


def check_far_norm(entry):
    """One norm entry point on a real [M, 320] source of 2^31 + 2^25 elements: the first and the last 2048 rows and every 4099th row
    against float64 (statistics summed in float64 over the whole source, in chunks) at KTOL.  The rows past 2^31 elements hold their
    own random data, so a 32-bit row offset reads, or writes, a wrong row."""
    nsg, rpg, C, G = FAR_NORM_SHAPE
    M, cg, eps = nsg * rpg, C // G, 1e-5
    name = f"far {entry} M{M} C{C} (2^31 + {M * C - (1 << 31)} elements)"
    why = far_skip_reason()
    if why is not None:
        return [_skip_row(name, why)]
    assert M * C > 1 << 31
    torch.cuda.reset_peak_memory_stats()
    x = torch.empty(M, C, dtype=torch.float16, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(47)
    step = 1 << 19
    for r in range(0, M, step):
        x[r:r + step].normal_(0.5, 1.0, generator=g)
    ga, be = _affine(C, 31)
    idx = torch.cat([torch.arange(2048), torch.arange(2048, M - 2048, 4099), torch.arange(M - 2048, M)]).to(DEV)
    xs = x[idx].double()
    if entry == "layernorm":
        y = ops.layernorm(x, ga, be, eps)
        ref = _ln_ref64(xs, ga, be, eps)
    else:
        s1 = torch.zeros(nsg, G, dtype=torch.float64, device=DEV)
        s2 = torch.zeros(nsg, G, dtype=torch.float64, device=DEV)
        chunk = 1 << 18
        assert rpg % chunk == 0
        for r in range(0, M, chunk):
            xc = x[r:r + chunk].double().view(chunk, G, cg)
            s1[r // rpg] += xc.sum((0, 2))
            s2[r // rpg] += xc.square_().sum((0, 2))
        mean = s1 / (rpg * cg)
        rstd = torch.rsqrt(s2 / (rpg * cg) - mean * mean + eps)      # float64: the cancellation costs 1e-16 x (1 + mean^2 / var)
        sg = idx // rpg
        yn = ((xs.view(-1, G, cg) - mean[sg][:, :, None]) * rstd[sg][:, :, None]).view(-1, C) * ga.double() + be.double()
        ref = yn * torch.sigmoid(yn)
        if entry == "groupnorm_from_stats":
            need = ops.gn_stats_floats(M, rpg, G)
            stats = torch.zeros(need, dtype=torch.float32, device=DEV)
            rec = stats[:3 * (M // 16) * G].view(M // 16, G, 3)
            for r in range(0, M, chunk):     # the records a producing GEMM writes: (K, sum(x - K), sum((x - K)^2)) per (16 rows, channel group)
                xc = x[r:r + chunk].float().view(chunk // 16, 16, G, cg)
                K = xc[:, 0, :, 0].clone()
                dlt = xc - K[:, None, :, None]
                out = rec[r // 16:(r + chunk) // 16]
                out[:, :, 0], out[:, :, 1], out[:, :, 2] = K, dlt.sum((1, 3)), dlt.square().sum((1, 3))
            y = ops.groupnorm_from_stats(x, ga, be, stats, rpg, groups=G, eps=eps, silu=True)
        else:
            stats = torch.zeros(ops.gn_scratch_floats(M, rpg, G), dtype=torch.float32, device=DEV)
            shard = (1, lambda t: None) if entry == "groupnorm pivot entry points" else None
            y = ops.groupnorm(x, ga, be, stats, rpg, groups=G, eps=eps, silu=True, shard=shard)
    torch.cuda.synchronize()
    rows = [_res(f"{name}: first / last 2048 rows and every 4099th row vs float64", y[idx], ref, KTOL)]
    FAR_PEAK[name] = torch.cuda.max_memory_allocated()
    del x, y
    torch.cuda.empty_cache()
    return rows


# ---- flat kernels: the only cases that move 4 GiB per operand
FAR_FLAT_N = (1 << 31) + 8 * 1024 + 3


def check_far_flat(which):
    """``silu`` / ``add`` on n = 2^31 + 8 x 1024 + 3 elements: the first and the last 2^20 elements and a strided sample against float64
    (2e-3, the elementwise edge check's bound), the whole output against torch's own elementwise result in chunks."""
    name = f"far {which} n = 2^31 + 8195"
    why = far_skip_reason()
    if why is not None:
        return [_skip_row(name, why)]
    n, ch = FAR_FLAT_N, 1 << 26    # chunked compares: the temporaries stay far below the two 4 GiB operands
    torch.cuda.reset_peak_memory_stats()
    x = torch.empty(n, dtype=torch.float16, device=DEV)
    g = torch.Generator(device=DEV).manual_seed(31)
    for o in range(0, n, 1 << 28):
        x[o:o + (1 << 28)].normal_(0.0, 2.0, generator=g)
    if which == "silu":
        y = ops.silu(x)
        f64 = lambda sl: F.silu(x[sl].double())
        native = lambda sl: F.silu(x[sl].float()).half()
    else:
        b = x    # both addends are the one 4 GiB buffer: the case stays inside FAR_CAP
        y = ops.add(x, b)
        f64 = lambda sl: x[sl].double() + b[sl].double()
        native = lambda sl: x[sl] + b[sl]
    torch.cuda.synchronize()
    rows = []
    for tag, sl in (("first 2^20", slice(0, 1 << 20)), ("last 2^20", slice(n - (1 << 20), n)), ("every 4099th", slice(0, n, 4099))):
        rows.append(_res(f"{name}: {tag} elements vs float64", y[sl], f64(sl), 2e-3))
    bad = 0
    for o in range(0, n, ch):
        sl = slice(o, min(o + ch, n))
        bad += int((y[sl] != native(sl)).sum())
    if which == "add":
        rows.append(dict(name=f"{name}: whole output == torch's fp16 add, differing elements", err=float(bad), tol=0.0, ok=bad == 0))
    else:   # silu in fp32 rounded once: torch's own kernel may round the last bit differently; the count is reported, the bound is 1 ulp
        ulp = 0
        for o in range(0, n, ch):
            sl = slice(o, min(o + ch, n))
            ulp = max(ulp, int((_fp16_key(y[sl]) - _fp16_key(native(sl))).abs().max()))
        rows.append(dict(name=f"{name}: whole output vs torch's fp32 silu rounded to fp16, max ulps ({bad} elements differ)", err=float(ulp), tol=1.0, ok=ulp <= 1))
    FAR_PEAK[name] = torch.cuda.max_memory_allocated()
    del x, y
    torch.cuda.empty_cache()
    return rows


# ------------------------------------------------------------------------------------------------ a branch subset under the batch hint
# The invariant the source-feature cache and the two-branch replay engine rest on (ops.batch_hint): a launch on the last B - 1 of a
# step's B branches, planned under batch_hint(B, B - 1), computes for its rows the BITS the launch on all B branches computes for them.
# Cases: tests/batch_subset_spec.py (tests/test_batch_subset_host.py proves on the CPU that the hint is decisive for the `sharp` ones).
# Rows of a case: the full launch against the reference of that kernel's existing check (KTOL: two equally wrong results do not pass);
# hinted subset == the full launch's rows, bit for bit; and, informational, whether the subset WITHOUT the hint happens to coincide.
def _bs_tail(full, r):
    """The rows of the full launch's result (or record slice) that the subset launch stands for."""
    return full[r:]


def _bs_same(name, got, want):
    same = bool(got.shape == want.shape and torch.equal(got, want))
    err = 0.0
    if not same:
        err = float((got.float() - want.float()).abs().nan_to_num(nan=float("inf")).max()) if got.shape == want.shape else float("inf")
        err = err or 1.0   # (-0.0 against 0.0, or NaN payloads: different bits, no distance)
    return dict(name=name, err=err, l2=0.0, tol=0.0, ok=same)


def _bs_info(name, got, want):
    same = bool(got.shape == want.shape and torch.equal(got, want))
    return dict(name=f"{name}: [info] subset WITHOUT the hint == full rows: {'yes (bits coincide)' if same else 'no (the hint is decisive)'}",
                err=0.0, l2=0.0, tol=0.0, ok=True, informational=True, coincides=same)


def _bs_rows(name, full, ref, tol, r, launch_subset, B, also=(), hint_free=False):
    """``launch_subset()`` -> the subset's result (a tensor, or a tuple of tensors compared one by one with ``full``'s); ``r``: the first
    row of the subset in each of them.  ``ref`` None: the caller adds the reference row.  ``hint_free``: the kernel's planner does not
    read the hint, so the subset launched WITHOUT it must be bit-equal as well (a row, not a remark)."""
    full = full if isinstance(full, tuple) else (full,)
    with ops.batch_hint(B, B - 1):
        sub = launch_subset()
    plain = launch_subset()
    torch.cuda.synchronize()
    sub, plain = (sub if isinstance(sub, tuple) else (sub,)), (plain if isinstance(plain, tuple) else (plain,))
    rows = [] if ref is None else [_res(f"{name}: full launch vs reference", full[0], ref, tol)]
    for i, (f, s, p) in enumerate(zip(full, sub, plain)):
        what = "output" if i == 0 else f"records / statistics {i}"
        want = _bs_tail(f, r[i] if isinstance(r, tuple) else r)
        rows.append(_bs_same(f"{name}: subset under batch_hint({B}, {B - 1}) == full rows, bit for bit ({what})", s, want))
        if hint_free:
            rows.append(_bs_same(f"{name}: subset WITHOUT the hint == full rows, bit for bit ({what})", p, want))
        else:
            rows.append(_bs_info(f"{name} ({what})", p, want))
    return rows + list(also)


def _bs_gemm_case(s, seed):
    """(a0, w, kwargs of ops.gemm, fp32 reference) of one GEMM case of batch_subset_spec on T = B r rows."""
    B, r, N, C0, C1, mode, act = s["B"], s["r"], s["N"], s["C0"], s["C1"], s["mode"], s["act"]
    T, K = B * r, C0 + C1
    if act == ops.ACT_GEGLU:
        a, wp, bp, ref = _geglu_case(T, K, N // 2, seed=seed)
        return a, wp, dict(bias=bp, act=act), ref
    if s["ln"]:
        x = (rnd(T, K, seed=seed).float() * 1.5 + 2.0).half()
        gamma, beta = (1.0 + 0.3 * rnd(K, seed=seed + 1).float()).half(), (0.2 * rnd(K, seed=seed + 2).float()).half()
        w, b = rnd(N, K, scale=1 / math.sqrt(K), seed=seed + 3), rnd(N, scale=0.1, seed=seed + 4)
        wq, bq, c1 = ops.ln_fold(w, b, gamma, beta)
        return x, wq, dict(bias=bq, ln=(c1, 1e-5)), F.layer_norm(x.float(), (K,), gamma.float(), beta.float(), 1e-5) @ w.float().t() + b.float()
    a = rnd(T, K, seed=seed)
    kw = dict(mode=mode)
    if mode == ops.MODE_LINEAR:
        w = rnd(N, K, scale=1 / math.sqrt(K), seed=seed + 1)
        y = a.float() @ w.float().t()
    elif mode == ops.MODE_CONV2D:
        H, W = s["geo"]
        w4 = rnd(N, K, 3, 3, scale=1 / math.sqrt(9 * K), seed=seed + 1)
        w = _pack_conv(w4)
        y = _to_tokens(F.conv2d(a.float().view(T // (H * W), H, W, K).permute(0, 3, 1, 2), w4.float(), padding=1))
        kw["conv"] = (H, W, H, W, 1, 0)
    else:
        Fr, HW = s["geo"]
        n = T // (Fr * HW)
        wt = rnd(N, K, 3, scale=1 / math.sqrt(3 * K), seed=seed + 1)
        w = wt.permute(0, 2, 1).reshape(N, 3 * K).contiguous()
        y = F.conv1d(a.float().view(n, Fr, HW, K).permute(0, 2, 3, 1).reshape(n * HW, K, Fr), wt.float(), padding=1)
        y = y.view(n, HW, N, Fr).permute(0, 3, 1, 2).reshape(T, N)
        kw["temporal"] = (Fr, HW)
    if "bias" in s["epi"]:
        kw["bias"] = rnd(N, seed=seed + 2)
        y = y + kw["bias"].float()
    if "rowvec" in s["epi"]:
        kw["rowvec"], kw["rowvec_div"] = rnd(B, N, seed=seed + 3), r
        y = y + kw["rowvec"].float().repeat_interleave(r, 0)
    if act:
        kw["act"] = act
        y = F.silu(y) if act == ops.ACT_SILU else F.gelu(y)
    if "res" in s["epi"]:
        kw["residual"] = rnd(T, N, seed=seed + 4)
        y = y + kw["residual"].float()
    a0, a1 = (a[:, :C0].contiguous(), a[:, C0:].contiguous()) if C1 else (a, None)
    if a1 is not None:
        kw["a1"] = a1
    return a0, w, kw, y


def _bs_gemm_subset_kw(kw, r):
    k2 = dict(kw)
    for key in ("residual", "a1"):
        if k2.get(key) is not None:
            k2[key] = k2[key][r:].contiguous()
    if k2.get("rowvec") is not None:
        k2["rowvec"] = k2["rowvec"][1:].contiguous()
    return k2


def check_subset_gemm(line):
    """Every GEMM case of one table line of batch_subset_spec.GEMM_SPECS ("ln / ff" adds the fused feed-forward kernel)."""
    import batch_subset_spec as bss
    out = []
    saved, saved_glds = ops.GEMM_FLAGS, ops.USE_GLDS
    try:
        ops.USE_GLDS = True
        for idx, s in enumerate(bss.GEMM_SPECS):
            if s["line"] != line:
                continue
            name = f"subset gemm[{s['line']}] {s['name']} r{s['r']} x {s['B']} N{s['N']} K{s['C0'] + s['C1']}"
            if s["gpu_skip"]:
                out.append(_skip_row(name, s["gpu_skip"]))
                continue
            ops.GEMM_FLAGS = ((saved & ~4) | s["flags"]) if s["flags"] else saved
            a0, w, kw, ref = _bs_gemm_case(s, 1000 + 10 * idx)
            r = s["r"]
            full = ops.gemm(a0, w, **kw)
            a0s, kws = a0[r:].contiguous(), _bs_gemm_subset_kw(kw, r)
            out += _bs_rows(name, full, ref, KTOL, r, lambda: ops.gemm(a0s, w, **kws), s["B"])
            del a0, w, kw, ref, full, a0s, kws
        ops.GEMM_FLAGS = saved
        if line == "ln / ff":
            C, H = 320, 1280
            B, r = bss.FF_SPEC["B"], bss.FF_SPEC["r"]
            w1, b1 = rnd(2 * H, C, scale=1 / math.sqrt(C)), rnd(2 * H, scale=0.1)
            w2, b2 = rnd(C, H, scale=1 / math.sqrt(H)), rnd(C, scale=0.1)
            w1p, b1p = _geglu_pack(w1, b1, H)
            w2s = ops.ff_pack_w2(w2)
            x, res = rnd(B * r, C, seed=501), rnd(B * r, C, seed=502)
            proj = x.float() @ w1.float().t() + b1.float()
            hid = (proj[:, :H] * F.gelu(proj[:, H:])).half().float()
            ref = (hid @ w2.float().t() + b2.float()).half().float() + res.float()
            full = ops.ff_geglu(x, w1p, b1p, w2s, b2, residual=res)
            xs, rs = x[r:].contiguous(), res[r:].contiguous()
            out += _bs_rows(f"subset {bss.FF_SPEC['name']} r{r} x {B}", full, ref, KTOL, r, lambda: ops.ff_geglu(xs, w1p, b1p, w2s, b2, residual=rs), B)
    finally:
        ops.GEMM_FLAGS, ops.USE_GLDS = saved, saved_glds
    return out


def _bs_norm_data(s, seed):
    import batch_subset_spec as bss
    C, nsg = s["C0"] + s["C1"], s["per_branch"] * s["B"]
    x = _offset_data(nsg, s["rpg"], C, 32, bss.NORM_OFFSET_SIGMA, seed=seed)
    x0, x1 = (x[:, :s["C0"]].contiguous(), x[:, s["C0"]:].contiguous()) if s["C1"] else (x, None)
    return x0, x1, _affine(C, seed + 1)


def check_subset_groupnorm():
    """``ops.groupnorm`` in one call: the chunk size follows the hinted group count (x0 only and x0 + x1, SiLU on and off, the (2, 1)
    stem pair), on data 50 sigma off zero."""
    import batch_subset_spec as bss
    out = []
    for i, s in enumerate(bss.NORM_SPECS):
        x0, x1, (ga, be) = _bs_norm_data(s, 700 + 10 * i)
        r = s["per_branch"] * s["rpg"]
        full = _gn_run(x0, x1, ga, be, s["rpg"], 32, 1e-5, s["silu"])
        ref = _gn_ref64(x0, x1, ga, be, s["rpg"], 32, 1e-5, s["silu"])
        x0s, x1s = x0[r:].contiguous(), None if x1 is None else x1[r:].contiguous()
        out += _bs_rows(f"subset {s['name']} rows/group {s['rpg']} x {s['per_branch'] * s['B']} silu={s['silu']}", full, ref, KTOL, r,
                        lambda: _gn_run(x0s, x1s, ga, be, s["rpg"], 32, 1e-5, s["silu"]), s["B"])
        del x0, x1, full, ref, x0s, x1s
    return out


def check_subset_groupnorm_two_phase_and_records():
    """The two-phase entry points (pivot, partial sums about the pivot, apply; ``ops.groupnorm(shard=(1, ...))``): output, partial sums
    [nsg][nchunks][G][2] and pivots [nsg][G] of the subset are the full launch's slices.  ``groupnorm_from_stats`` on the records of the
    GEMM that produced its input: GEMM output, records [M / 16][G][3] and the normalised output likewise (the fold of 257 records per
    group into runs of 2 does not depend on the first row)."""
    import batch_subset_spec as bss
    from anyv2v_amd import _lib
    lib = _lib.load()
    out = []
    s = bss.NORM_TWO_PHASE
    G, rpg, B, C = 32, s["rpg"], s["B"], s["C0"] + s["C1"]
    x0, x1, (ga, be) = _bs_norm_data(s, 800)
    r = s["per_branch"] * rpg

    def two_phase(x0_, x1_):
        M = x0_.shape[0]
        n, npiv = int(lib.anyv2v_groupnorm_partial_floats(M, rpg, G, C)), (M // rpg) * G
        stats = torch.zeros(ops.gn_scratch_floats(M, rpg, G), dtype=torch.float32, device=DEV)
        y = ops.groupnorm(x0_, ga, be, stats, rpg, x1=x1_, groups=G, eps=1e-5, silu=s["silu"], shard=(1, lambda t: None))
        return y, stats[:n].view(M // rpg, -1).clone(), stats[n:n + npiv].view(M // rpg, G).clone()
    full = two_phase(x0, x1)
    ref = _gn_ref64(x0, x1, ga, be, rpg, G, 1e-5, s["silu"])
    x0s, x1s = x0[r:].contiguous(), None if x1 is None else x1[r:].contiguous()
    out += _bs_rows(f"subset two-phase {s['name']} rows/group {rpg} x {s['per_branch'] * B}", full, ref, KTOL, (r, s["per_branch"], s["per_branch"]),
                    lambda: two_phase(x0s, x1s), B)
    del x0, x1, full, ref, x0s, x1s
    # records of a producing GEMM
    s = bss.NORM_RECORDS
    rpg, B, C, K = s["rpg"], s["B"], s["C"], s["K"]
    r = s["per_branch"] * rpg
    T = B * r
    a, w, bias = rnd(T, K, seed=811), rnd(C, K, scale=1 / math.sqrt(K), seed=812), (rnd(C, seed=813).float() + 3.0).half()
    ga, be = _affine(C, 814)

    def chain(a_):
        M = a_.shape[0]
        assert ops.gemm_gn_stats_floats(a_, w, rows_per_group=rpg, groups=G, bias=bias) == 3 * (M // 16) * G, "the producer's plan emits no records"
        rec = torch.zeros(ops.gn_stats_floats(M, rpg, G), dtype=torch.float32, device=DEV)
        c = ops.gemm(a_, w, bias=bias, gn=(rec, rpg, G))
        y = ops.groupnorm_from_stats(c, ga, be, rec, rpg, groups=G, silu=True)
        return y, c, rec[:3 * (M // 16) * G].view(M // 16, 3 * G).clone()
    full = chain(a)
    ref = _gn_ref64(full[1], None, ga, be, rpg, G, 1e-5, True)
    a_s = a[r:].contiguous()
    out += _bs_rows(f"subset {s['name']} rows/group {rpg} x {B}", full, ref, KTOL, (r, r, r // 16), lambda: chain(a_s), B,
                    also=[_res(f"subset {s['name']}: the producing GEMM vs torch", full[1], _gemm_ref(a, w, bias), KTOL)])
    return out


def _bs_attn_layout(s, batch, Sq, Sk):
    """(q rows, kv rows, inner, q strides, kv strides) of ``batch`` elements."""
    if s["layout"] == "temporal":
        HW = s["HW"]
        st = (Sq * HW, 1, HW)
        return batch // HW * Sq * HW, batch // HW * Sk * HW, HW, st, st
    return batch * Sq, (batch // s.get("kv_div", 1)) * Sk, 1, (Sq, 0, 1), (Sk, 0, 1)


def check_subset_attention():
    """``ops.attention`` on the last two of three branches' batch elements, with and without the hint (the attention planner does not
    read it): plain flash with a ragged last query tile, cross-attention with kv_div, the one-wave temporal kernel at a unit offset
    that is no multiple of the 4 units of a block, the 96-key loop and whole-sequence kernels, 8-wave blocks against 4-wave blocks."""
    import batch_subset_spec as bss
    out = []
    for i, s in enumerate(bss.ATTN_SPECS):
        b, h, Sq, Sk, d, sub = s["batch"], s["heads"], s["Sq"], s["Sk"], s["d"], s["sub"]
        C = h * d
        Mq, Mk, inner, qst, kst = _bs_attn_layout(s, b, Sq, Sk)
        fused = s["kv_div"] == 1 and Sq == Sk
        if fused:
            m = rnd(Mq, 3 * C, seed=900 + i)
            q2, k2, v2 = m[:, :C], m[:, C:2 * C], m[:, 2 * C:]
        else:
            q2, kv = rnd(Mq, C, seed=900 + i), rnd(Mk, 2 * C, seed=950 + i)
            k2, v2 = kv[:, :C], kv[:, C:]
        extra = {} if d == 64 else dict(scale=d ** -0.5, head_dim=d)
        kw = dict(heads=h, Sq=Sq, Sk=Sk, inner=inner, q_strides=qst, kv_strides=kst, kv_div=s["kv_div"])
        full = ops.attention(q2, k2, v2, torch.zeros(Mq, C, dtype=torch.float16, device=DEV), batch=b, **kw, **extra)
        only = None if b * h * Sq * Sk <= (1 << 26) else [0, sub, b - 1]
        rows, ref = _attn_ref(q2, k2, v2, batch=b, d=d, only=only, **kw)
        rq, rk = _bs_attn_layout(s, sub, Sq, Sk)[:2]
        if fused:
            ms = m[rq:].contiguous()
            qs, ks, vs = ms[:, :C], ms[:, C:2 * C], ms[:, 2 * C:]
        else:
            qs, kvs = q2[rq:].contiguous(), kv[rk:].contiguous()
            ks, vs = kvs[:, :C], kvs[:, C:]
        name = f"subset attention[{s['full']} -> {s['subset']}] {s['name']}"
        out.append(_res(f"{name}: full launch vs fp32 SDPA", full[rows], ref, KTOL))
        out += _bs_rows(name, full, None, KTOL, rq, lambda: ops.attention(qs, ks, vs, torch.zeros(Mq - rq, C, dtype=torch.float16, device=DEV),
                                                                         batch=b - sub, **kw, **extra), 3, hint_free=True)
        del full, ref
    return out


def check_subset_attention_pnp():
    """The PnP launch of a replayed site (unet.py: HipAttnProcessor.run, ``src_io = ("replay", buf)``): [negative, editing] with Q, K
    read from the cached source rows [Ts, 2 C], V from the two-branch matrix, ``qk_mod = batch / 2`` -- against branches 1 and 2 of the
    three-branch shared-softmax launch (``qk_mod = batch / 3``).  Flash form and the <= 16-frame one-wave form."""
    import batch_subset_spec as bss
    out = []
    for i, s in enumerate(bss.ATTN_PNP_SPECS):
        e, h, S = s["per_branch"], s["heads"], s["S"]
        C = 64 * h
        M3, _mk, inner, st, _ = _bs_attn_layout(s, 3 * e, S, S)
        Ts = M3 // 3
        qkv3 = rnd(M3, 3 * C, seed=980 + i)
        kw = dict(heads=h, Sq=S, Sk=S, inner=inner, q_strides=st, kv_strides=st)
        full = ops.attention(qkv3[:, :C], qkv3[:, C:2 * C], qkv3[:, 2 * C:], torch.zeros(M3, C, dtype=torch.float16, device=DEV), batch=3 * e, qk_mod=e, **kw)
        rows, ref = _attn_ref(qkv3[:, :C], qkv3[:, C:2 * C], qkv3[:, 2 * C:], batch=3 * e, qk_mod=e, **kw)
        src_qk = qkv3[:Ts, :2 * C].contiguous()
        qkv2 = torch.full((2 * Ts, 3 * C), float("nan"), dtype=torch.float16, device=DEV)   # (Q, K columns of the two branches: never projected, never read)
        qkv2[:, 2 * C:] = qkv3[Ts:, 2 * C:]

        def replay():
            return ops.attention(src_qk[:, :C], src_qk[:, C:], qkv2[:, 2 * C:], torch.zeros(2 * Ts, C, dtype=torch.float16, device=DEV), batch=2 * e,
                                 qk_mod=e, **kw)
        name = f"subset attention[{s['full']} -> {s['subset']}] {s['name']}"
        out.append(_res(f"{name}: three-branch launch vs fp32 SDPA", full[rows], ref, KTOL))
        out += _bs_rows(name, full, None, KTOL, Ts, replay, 3, hint_free=True)
    return out


def check_subset_step_kernels():
    """The step kernels that take branch indices: the three-branch Vtok with (b_unc, b_cond) = (1, 2) against Vtok[1:] with (0, 1) --
    cfg_ddim_step, guidance_stats (its records), cfg_ddim_step_ex with rescale and noise, guided_step."""
    import batch_subset_spec as bss
    import sampler_options_spec as sos
    from anyv2v_amd.schedulers import DDIMScheduler
    out = []
    sp = bss.STEP_SPEC
    C, Fr, H, W, ld, G = sp["C"], sp["F"], sp["H"], sp["W"], sp["ld"], sp["guidance"]
    n1 = Fr * H * W
    vt = (rnd(3 * n1, ld, seed=1201).float() + 0.25).half()
    lat, noise = rnd(1, C, Fr, H, W, seed=1202), rnd(1, C, Fr, H, W, seed=1203)
    vts = vt[n1:].contiguous()
    coef = torch.tensor([0.8, 0.6, 0.9, math.sqrt(1 - 0.81)], dtype=torch.float32, device=DEV)
    c = [float(t) for t in coef]
    vv = vt[:, :C].double().view(3, Fr, H * W, C).permute(0, 3, 1, 2).reshape(3, C, Fr, H, W)
    v = _h(vv[1].float() + _h(G * _h(vv[2].float() - vv[1].float()))).double()   # the kernel's fp16 CFG rounding points
    xx = lat.double()[0]
    ref = (c[2] * (c[0] * xx - c[1] * v) + c[3] * (c[0] * v + c[1] * xx))[None]
    full = ops.cfg_ddim_step(vt, 1, 2, G, coef, lat, torch.empty_like(lat))
    out += _bs_rows("subset cfg_ddim_step (1, 2) -> (0, 1)", full, ref, KTOL, 0, lambda: ops.cfg_ddim_step(vts, 0, 1, G, coef, lat, torch.empty_like(lat)), 3)
    sch = DDIMScheduler()
    sch.set_timesteps(50)
    row = sch.coefficient_table([501], "cpu", eta=0.5, phi=0.7, n=lat.numel())[0]
    drow = row.to(DEV)
    ref = sos.fused_step(vt.cpu(), 1, 2, G, [float(t) for t in row], lat.cpu(), noise.cpu(), 0)

    def ex(v_, bu, bc):
        stats = ops.guidance_stats(v_, bu, bc, G, lat.shape)
        y = ops.cfg_ddim_step_ex(v_, bu, bc, G, drow, lat, torch.empty_like(lat), prediction=0, stats=stats, phi=0.7, noise=noise)
        return y, stats.clone()
    out += _bs_rows("subset guidance_stats + cfg_ddim_step_ex (1, 2) -> (0, 1)", ex(vt, 1, 2), ref, KTOL, (0, 0), lambda: ex(vts, 0, 1), 3)
    n = 4096 * 256 + 777   # past the grid cap: the grid-stride loop iterates
    e, x = rnd(3, n, seed=1204), rnd(n, seed=1205)
    es = e[1:].contiguous()
    cf = (0.8, 0.6, 0.9, math.sqrt(1 - 0.81))
    for pred in (0, 1, 2):
        full = ops.guided_step(e, x, cf, b_unc=1, b_txt=2, g_txt=G, prediction=pred)
        out += _bs_rows(f"subset guided_step prediction {pred} (1, 2) -> (0, 1)", full, _guided_ref(e, x, cf, 2, 1, -1, G, 1.0, pred), KTOL, 0,
                        lambda: ops.guided_step(es, x, cf, b_unc=0, b_txt=1, g_txt=G, prediction=pred), 3)
    return out


def check_subset_layernorm_softmax():
    """``layernorm`` and ``softmax_rows``: rows [T / 3, T) at an offset that is no multiple of the rows a block takes."""
    import batch_subset_spec as bss
    out = []
    r, C = bss.LAYERNORM_SPEC["r"], bss.LAYERNORM_SPEC["C"]
    x = (rnd(3 * r, C, seed=1301).float() * 1.5 + 2.0).half()
    ga, be = _affine(C, 1302)
    xs = x[r:].contiguous()
    out += _bs_rows(f"subset layernorm r{r} x 3 C{C}", ops.layernorm(x, ga, be), _ln_ref64(x, ga, be, 1e-5), KTOL, r, lambda: ops.layernorm(xs, ga, be), 3)
    r, cols = bss.SOFTMAX_SPEC["r"], bss.SOFTMAX_SPEC["cols"]
    s = (rnd(3 * r, cols, seed=1303).float() * 8.0).contiguous()
    ss = s[r:].contiguous()
    out += _bs_rows(f"subset softmax_rows r{r} x 3 cols{cols}", ops.softmax_rows(s, 0.125), torch.softmax(0.125 * s.double(), 1), KTOL, r,
                    lambda: ops.softmax_rows(ss, 0.125), 3)
    return out


def check_subset_hint_restored():
    """After every ``with ops.batch_hint(...)`` above, a plain launch plans as un-hinted again: batch_subset_spec.HINT_PROBE is a
    launch whose plan splits K on its own rows (no GroupNorm records) and emits records under batch_hint(3, 2) (the three-branch
    launch does not split)."""
    import batch_subset_spec as bss
    p = bss.HINT_PROBE
    a, w = torch.empty(p["M"], p["K"], dtype=torch.float16, device=DEV), torch.empty(p["N"], p["K"], dtype=torch.float16, device=DEV)
    q = lambda: ops.gemm_gn_stats_floats(a, w, rows_per_group=p["M"], groups=32)
    plain = q()
    with ops.batch_hint(3, 2):
        hinted = q()
    after = q()
    ok = plain == after == 0 and hinted == 3 * (p["M"] // 16) * 32 and ops._HINT == [1, 1]
    return [dict(name=f"batch hint restored: records query plain {plain}, under batch_hint(3, 2) {hinted}, after {after}", err=0.0 if ok else 1.0, l2=0.0, tol=0.0, ok=ok)]
