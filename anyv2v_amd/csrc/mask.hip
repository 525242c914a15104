// Masked PnP editing: the source clip is kept outside an edit mask, bit for bit (latent blending of Blended Latent Diffusion, arXiv
// 2206.02779, and of diffusers' inpaint loop `latents = (1 - mask) * init_latents_proper + mask * latents`, with the inverted latent of
// the source in the place of the re-noised one).  Nothing in the reference does this; include/anyv2v_hip.h holds the definition.
//   mask_pool_kernel     mean over each 8 x 8 pixel block of the pixel mask -> latent resolution
//   mask_grow_kernel     maximum over the (2 r + 1)^2 window, positions outside the image ignored
//   mask_feather_kernel  separable Gaussian with replicate padding, evaluated per output (runs once per clip: <= 49^2 taps x F h w)
//   masked_blend_kernel  out = m == 0 ? src : m == 1 ? x : fp16(fmaf(m, x - src, src)), the mask broadcast over channels (and frames)
// Values are dropped by a select, never by a multiply: outside the mask the output carries the source's bits even where x is Inf / NaN.
// No atomics; every output element is written exactly once by one thread.
#include "common.h"

#include <math.h>

#define MK_THREADS 256
#define MK_MAX_GROW ANYV2V_MASK_MAX_GROW
#define MK_MAX_R ANYV2V_MASK_MAX_RADIUS

struct MaskTaps {
    float t[2 * MK_MAX_R + 1];
};

// a stage's result goes to the fp32 workspace, or -- the last stage that runs -- through the one rounding to fp16 into the latent mask
__device__ __forceinline__ void mask_store(float v, int i, float* __restrict__ outf, half_t* __restrict__ outh) {
    if (outh != nullptr)
        outh[i] = (half_t)v;
    else
        outf[i] = v;
}

// Sum of the 64 values in units of 2^-24 (the smallest fp16 subnormal; values clamped to [0, 1], NaN counts as 0): an exact integer
// <= 2^30.  Its conversion to fp32 is the ONE rounding of this stage, so the pooled value is the correctly rounded mean whatever the
// order of the additions (a binary mask gives k / 64 exactly).
__global__ __launch_bounds__(MK_THREADS) void mask_pool_kernel(const half_t* __restrict__ mask, int n, int h, int w, float* __restrict__ outf,
                                                               half_t* __restrict__ outh) {
    const int i = blockIdx.x * MK_THREADS + threadIdx.x;
    if (i >= n) return;
    const int x = i % w, y = (i / w) % h, f = i / (w * h);
    const half_t* src = mask + ((long long)f * h * 8 + (long long)y * 8) * (w * 8) + x * 8;
    uint32_t sum = 0;
    for (int r = 0; r < 8; ++r) {
        const half_t* row = src + (long long)r * (w * 8);
#pragma unroll
        for (int c = 0; c < 8; ++c) {
            const float v = fminf(fmaxf((float)row[c], 0.0f), 1.0f);
            sum += (uint32_t)(v * 16777216.0f);
        }
    }
    mask_store((float)sum * 9.31322574615478515625e-10f /* 2^-30 */, i, outf, outh);
}

__global__ __launch_bounds__(MK_THREADS) void mask_grow_kernel(const float* __restrict__ in, int n, int h, int w, int r, float* __restrict__ outf,
                                                               half_t* __restrict__ outh) {
    const int i = blockIdx.x * MK_THREADS + threadIdx.x;
    if (i >= n) return;
    const int x = i % w, y = (i / w) % h, f = i / (w * h);
    const float* plane = in + (long long)f * h * w;
    const int y0 = max(y - r, 0), y1 = min(y + r, h - 1), x0 = max(x - r, 0), x1 = min(x + r, w - 1);
    float m = 0.0f;   // (the pooled values are >= 0)
    for (int yy = y0; yy <= y1; ++yy)
        for (int xx = x0; xx <= x1; ++xx) m = fmaxf(m, plane[yy * w + xx]);
    mask_store(m, i, outf, outh);
}

// out[y, x] = sum_j t[j] (sum_i t[i] in[clamp(y + j), clamp(x + i)]): rows first, each in tap order, in fp32
__global__ __launch_bounds__(MK_THREADS) void mask_feather_kernel(const float* __restrict__ in, int n, int h, int w, int R, MaskTaps taps,
                                                                  float* __restrict__ outf, half_t* __restrict__ outh) {
    const int i = blockIdx.x * MK_THREADS + threadIdx.x;
    if (i >= n) return;
    const int x = i % w, y = (i / w) % h, f = i / (w * h);
    const float* plane = in + (long long)f * h * w;
    float acc = 0.0f;
    for (int j = -R; j <= R; ++j) {
        const float* row = plane + min(max(y + j, 0), h - 1) * w;
        float racc = 0.0f;
        for (int k = -R; k <= R; ++k) racc = fmaf(taps.t[k + R], row[min(max(x + k, 0), w - 1)], racc);
        acc = fmaf(taps.t[j + R], racc, acc);
    }
    mask_store(acc, i, outf, outh);
}

__device__ __forceinline__ half_t blend_one(half_t x, half_t s, half_t m) {
    const float mf = (float)m;
    // the fp32 fma, THEN the fp16 rounding: left alone, hipcc fuses the fma and the conversion into v_fma_mixlo_f16, which rounds the
    // exact result once -- another fp16 value wherever the fp32 rounding lands on an fp16 tie (as in freeu.hip)
    float y = __builtin_fmaf(mf, (float)x - (float)s, (float)s);
    asm("" : "+v"(y));
    const half_t b = (half_t)y;
    return mf == 0.0f ? s : (mf == 1.0f ? x : b);
}

// VEC: 8 elements (16 bytes) per thread along w -- HW % 8 == 0 keeps a vector inside one (channel, frame) plane and its mask aligned
template <bool VEC>
__global__ __launch_bounds__(MK_THREADS) void masked_blend_kernel(const half_t* x, const half_t* __restrict__ src, const half_t* __restrict__ mask,
                                                                  int mask_frames, half_t* out, int n, int F, int HW) {
    const int per = VEC ? 8 : 1;
    const long long i = ((long long)blockIdx.x * MK_THREADS + threadIdx.x) * per;
    if (i >= n) return;
    const int plane = (int)(i / HW), p = (int)(i - (long long)plane * HW);   // plane = c * F + f
    const int mi = (mask_frames == 1 ? 0 : plane % F) * HW + p;
    if (VEC) {
        const h8 xv = *(const h8*)(x + i), sv = *(const h8*)(src + i), mv = *(const h8*)(mask + mi);
        h8 y;
#pragma unroll
        for (int e = 0; e < 8; ++e) y[e] = blend_one(xv[e], sv[e], mv[e]);
        *(h8*)(out + i) = y;
    } else {
        out[i] = blend_one(x[i], src[i], mask[mi]);
    }
}

extern "C" int anyv2v_latent_mask_f16(const void* mask, int32_t mask_frames, int32_t H, int32_t W, int32_t grow, const float* taps,
                                      int32_t R, float* workspace, void* out, void* stream) {
    AV_CHECK(mask && workspace && out, "latent_mask: null pointer");
    AV_CHECK(mask_frames >= 1 && H >= 8 && W >= 8 && H % 8 == 0 && W % 8 == 0,
             "latent_mask: mask_frames = %d, H = %d, W = %d: at least one frame, H and W positive multiples of 8", mask_frames, H, W);
    AV_CHECK(grow >= 0 && grow <= MK_MAX_GROW, "latent_mask: grow = %d must lie in [0, %d]", grow, MK_MAX_GROW);
    AV_CHECK(R >= 0 && R <= MK_MAX_R, "latent_mask: R = %d must lie in [0, %d]", R, MK_MAX_R);
    AV_CHECK(R == 0 || taps, "latent_mask: null pointer (R > 0 needs the 2 R + 1 taps)");
    AV_CHECK((long long)mask_frames * H * W < (1ll << 31), "latent_mask: mask_frames * H * W must fit an int");
    MaskTaps tp;
    for (int i = 0; i < 2 * MK_MAX_R + 1; ++i) tp.t[i] = 0.0f;
    for (int i = 0; i < 2 * R + 1 && R > 0; ++i) {
        AV_CHECK(isfinite(taps[i]) && taps[i] >= 0.0f && taps[i] <= 1.0f, "latent_mask: tap %d is not a weight in [0, 1]", i);
        tp.t[i] = taps[i];
    }
    const int h = H / 8, w = W / 8, n = mask_frames * h * w;
    const dim3 grid((unsigned)((n + MK_THREADS - 1) / MK_THREADS)), block(MK_THREADS);
    hipStream_t st = (hipStream_t)stream;
    float* a = workspace;
    float* b = workspace + n;
    half_t* o = (half_t*)out;
    const bool g = grow > 0, f = R > 0;
    hipLaunchKernelGGL(mask_pool_kernel, grid, block, 0, st, (const half_t*)mask, n, h, w, a, (g || f) ? (half_t*)nullptr : o);
    if (g) hipLaunchKernelGGL(mask_grow_kernel, grid, block, 0, st, (const float*)a, n, h, w, grow, b, f ? (half_t*)nullptr : o);
    if (f) hipLaunchKernelGGL(mask_feather_kernel, grid, block, 0, st, (const float*)(g ? b : a), n, h, w, R, tp, g ? a : b, o);
    return av_launch_status("latent_mask");
}

extern "C" int anyv2v_masked_blend_f16(const void* x, const void* src, const void* mask, int32_t mask_frames, void* out, int32_t C,
                                       int32_t F, int32_t HW, void* stream) {
    AV_CHECK(x && src && mask && out, "masked_blend: null pointer");
    AV_CHECK(C > 0 && F > 0 && HW > 0, "masked_blend: bad arguments (C = %d, F = %d, HW = %d)", C, F, HW);
    AV_CHECK(mask_frames == 1 || mask_frames == F, "masked_blend: mask_frames = %d must be 1 or F = %d", mask_frames, F);
    AV_CHECK((long long)C * F * HW < (1ll << 31), "masked_blend: C * F * HW must fit an int");
    AV_CHECK(src != out && mask != out, "masked_blend: out may alias x only");
    const int n = C * F * HW;
    const bool vec = HW % 8 == 0 && av_aligned16(x) && av_aligned16(src) && av_aligned16(mask) && av_aligned16(out);
    const int threads = vec ? n / 8 : n;
    const dim3 grid((unsigned)((threads + MK_THREADS - 1) / MK_THREADS)), block(MK_THREADS);
    if (vec)
        hipLaunchKernelGGL(masked_blend_kernel<true>, grid, block, 0, (hipStream_t)stream, (const half_t*)x, (const half_t*)src,
                           (const half_t*)mask, mask_frames, (half_t*)out, n, F, HW);
    else
        hipLaunchKernelGGL(masked_blend_kernel<false>, grid, block, 0, (hipStream_t)stream, (const half_t*)x, (const half_t*)src,
                           (const half_t*)mask, mask_frames, (half_t*)out, n, F, HW);
    return av_launch_status("masked_blend");
}
