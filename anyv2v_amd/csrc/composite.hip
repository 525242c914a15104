// Pixel-space composite behind the VAE decode of a masked PnP edit: outside the edit region the frames written are the SOURCE's bytes, not
// decode(encode(source)) (the pixel-space finish of Blended Latent Diffusion, arXiv 2206.02779; diffusers' `apply_overlay` of the inpaint
// pipelines).  Nothing in the reference does this; include/anyv2v_hip.h holds the definition.
//   alpha_row_dist_kernel     per latent row and pixel column: the distance, along the row, to the nearest latent cell with mask > 0
//   alpha_dilate_kernel       column pass over the latent rows in reach: code 2 = core (grown by grow_px), 1 = wide (grow_px + R), 0
//   alpha_row_feather_kernel  Gaussian along x of (code >= 1), replicate padding, tap order, fp32 fmaf; the row through an LDS tile
//   alpha_col_feather_kernel  Gaussian along y of the row sums, eight outputs of one column per thread; alpha = core ? 1 : min(a, 1)
//   composite_stats_kernel    exact 64-bit integer sums over the kept pixels (alpha == 0), one record per block of a fixed grid
//   composite_kernel          out = alpha == 0 ? source : alpha == 1 ? edit : rint(fmaf(alpha, edit - source, source)), in bytes
// Dilation and feather are separable two-pass kernels: O(grow_px + R) per output, not its square (mask.hip evaluates full windows, which
// is right for a <= 64 x 64 latent grid and not for 16 x 512 x 512 pixels).  Values are dropped by a select, never by a multiply: a kept
// pixel carries the source's byte whatever the decode holds there.  No atomics; every output element is written exactly once by one thread.
#include "common.h"

#include <math.h>

#define CP_THREADS 256
#define CP_MAX_GROW ANYV2V_COMPOSITE_MAX_GROW
#define CP_MAX_R ANYV2V_COMPOSITE_MAX_RADIUS
#define CP_BLOCKS ANYV2V_COMPOSITE_STATS_BLOCKS
#define CP_RECORD ANYV2V_COMPOSITE_STATS_RECORD
#define CP_YB 8           // outputs of one column per thread in the column feather (H = 8 h: the chunks are whole)
#define CP_FAR (1 << 20)  // "no cell of this row in reach"

struct AlphaTaps {
    float t[2 * CP_MAX_R + 1];
};

// distance from pixel p to the 8 pixels [8 c, 8 c + 7] of latent cell c along one axis
__device__ __forceinline__ int cell_dist(int p, int c) { return max(0, max(8 * c - p, p - 8 * c - 7)); }

__global__ __launch_bounds__(CP_THREADS) void alpha_row_dist_kernel(const half_t* __restrict__ lm, int n, int w, int reach,
                                                                    float* __restrict__ dist) {
    const int i = blockIdx.x * CP_THREADS + threadIdx.x;   // over [Fm h, W]
    if (i >= n) return;
    const int W = 8 * w, x = i % W, row = i / W;
    const half_t* cells = lm + (long long)row * w;
    const int c0 = max(x - reach, 0) >> 3, c1 = min((x + reach) >> 3, w - 1);
    int d = CP_FAR;
    for (int c = c0; c <= c1; ++c)
        if ((float)cells[c] > 0.0f) d = min(d, cell_dist(x, c));
    dist[i] = (float)d;
}

// FINAL (R == 0): the hard mask goes straight to alpha; else the code to the workspace
template <bool FINAL>
__global__ __launch_bounds__(CP_THREADS) void alpha_dilate_kernel(const float* __restrict__ dist, int n, int h, int w, int grow, int reach,
                                                                  float* __restrict__ out) {
    const int i = blockIdx.x * CP_THREADS + threadIdx.x;   // over [Fm, H, W]
    if (i >= n) return;
    const int W = 8 * w, H = 8 * h, x = i % W, y = (i / W) % H, f = i / (W * H);
    const float* col = dist + (long long)f * h * W + x;
    const int r0 = max(y - reach, 0) >> 3, r1 = min((y + reach) >> 3, h - 1);
    bool core = false, wide = false;
    for (int r = r0; r <= r1; ++r) {
        const float d = col[(long long)r * W];
        const int dv = cell_dist(y, r);
        core = core || (dv <= grow && d <= (float)grow);
        wide = wide || (dv <= reach && d <= (float)reach);
    }
    out[i] = FINAL ? (core ? 1.0f : 0.0f) : (core ? 2.0f : (wide ? 1.0f : 0.0f));
}

__global__ __launch_bounds__(CP_THREADS) void alpha_row_feather_kernel(const float* __restrict__ code, int W, int tiles, int R, AlphaTaps taps,
                                                                       float* __restrict__ out) {
    __shared__ float tile[CP_THREADS + 2 * CP_MAX_R];
    const int row = blockIdx.x / tiles, x0 = (blockIdx.x % tiles) * CP_THREADS;
    const float* src = code + (long long)row * W;
    for (int i = threadIdx.x; i < CP_THREADS + 2 * R; i += CP_THREADS)
        tile[i] = src[min(max(x0 - R + i, 0), W - 1)] >= 1.0f ? 1.0f : 0.0f;   // wide (the core lies inside it)
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= W) return;
    float acc = 0.0f;
    for (int k = 0; k <= 2 * R; ++k) acc = fmaf(taps.t[k], tile[threadIdx.x + k], acc);
    out[(long long)row * W + x] = acc;
}

// Output y0 + k takes tap j from row y0 + k + j - R: with s = k + j the row is y0 + s - R for every k, so one load serves up to eight
// outputs, and for each output j still ascends with s -- the sum runs in tap order.
__global__ __launch_bounds__(CP_THREADS) void alpha_col_feather_kernel(const float* __restrict__ rows, const float* __restrict__ code, int n,
                                                                       int H, int W, int R, AlphaTaps taps, float* __restrict__ alpha) {
    const int i = blockIdx.x * CP_THREADS + threadIdx.x;   // over [Fm, H / 8, W]
    if (i >= n) return;
    const int x = i % W, y0 = (i / W) % (H / CP_YB) * CP_YB, f = i / (W * (H / CP_YB));
    const long long base = (long long)f * H * W + x;
    float acc[CP_YB];
#pragma unroll
    for (int k = 0; k < CP_YB; ++k) acc[k] = 0.0f;
    for (int s = 0; s < CP_YB + 2 * R; ++s) {
        const float v = rows[base + (long long)min(max(y0 - R + s, 0), H - 1) * W];
#pragma unroll
        for (int k = 0; k < CP_YB; ++k) {
            const int j = s - k;
            if (j >= 0 && j <= 2 * R) acc[k] = fmaf(taps.t[j], v, acc[k]);
        }
    }
#pragma unroll
    for (int k = 0; k < CP_YB; ++k) {
        const long long o = base + (long long)(y0 + k) * W;
        alpha[o] = code[o] >= 2.0f ? 1.0f : fminf(acc[k], 1.0f);
    }
}

// The level `vae.to_pil` forms from an fp16 value: ((v + 1.0) * 127.5).round().clamp(0, 255) on an fp16 tensor -- the sum rounded to fp16,
// the product rounded to fp16, round-half-even, the clamp; NaN gives 0 (what the conversion to uint8 makes of it), +-Inf 255 / 0.  Each
// fp32 operation is exact or correctly rounded and is THEN rounded to fp16 (innocuous double rounding: 24 >= 2 * 11 + 2); the empty asm
// statements keep hipcc from contracting the steps.
__device__ __forceinline__ float pil_level(half_t v) {
    float a = (float)v + 1.0f;
    asm("" : "+v"(a));
    float b = (float)(half_t)a * 127.5f;
    asm("" : "+v"(b));
    const float r = rintf((float)(half_t)b);
    return fminf(fmaxf(r, 0.0f), 255.0f);   // (fmaxf drops the NaN: 0)
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// record of a block: for channel c the five sums at [5 c .. 5 c + 4] = count, sum e, sum e^2, sum s, sum s^2; [15] = 0.  Integer sums:
// the same whatever the order.
__global__ __launch_bounds__(CP_THREADS) void composite_stats_kernel(const half_t* __restrict__ video, const uint8_t* __restrict__ src,
                                                                     const float* __restrict__ alpha, int mask_frames, int F, int HW,
                                                                     long long* __restrict__ rec) {
    __shared__ unsigned long long red[CP_THREADS / WAVE][CP_RECORD];
    unsigned long long acc[15];
#pragma unroll
    for (int k = 0; k < 15; ++k) acc[k] = 0;
    const int n = F * HW;
    for (int p = blockIdx.x * CP_THREADS + threadIdx.x; p < n; p += CP_BLOCKS * CP_THREADS) {
        const int f = p / HW, hw = p - f * HW;
        if (alpha[mask_frames == 1 ? hw : p] != 0.0f) continue;
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const unsigned long long e = (unsigned long long)pil_level(video[((long long)c * F + f) * HW + hw]);
            const unsigned long long s = src[3ll * p + c];
            acc[5 * c] += 1;
            acc[5 * c + 1] += e;
            acc[5 * c + 2] += e * e;
            acc[5 * c + 3] += s;
            acc[5 * c + 4] += s * s;
        }
    }
#pragma unroll
    for (int k = 0; k < 15; ++k) {
        const unsigned long long t = wave_sum_u64(acc[k]);
        if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE][k] = t;
    }
    __syncthreads();
    if (threadIdx.x < CP_RECORD) {
        unsigned long long t = 0;
        if (threadIdx.x < 15)
            for (int i = 0; i < CP_THREADS / WAVE; ++i) t += red[i][threadIdx.x];
        rec[blockIdx.x * CP_RECORD + threadIdx.x] = (long long)t;
    }
}

// match: e' = clamp(fmaf(gain, e, bias), 0, 255) stands in for e; one rint at the end.  The fp32 fma, THEN rint (as blend_one in mask.hip).
__device__ __forceinline__ uint8_t composite_one(half_t v, uint8_t sb, float a, bool match, float gain, float bias) {
    const float s = (float)sb;
    float e = pil_level(v);
    if (match) e = fminf(fmaxf(fmaf(gain, e, bias), 0.0f), 255.0f);
    float y = __builtin_fmaf(a, e - s, s);
    asm("" : "+v"(y));
    const float b = fminf(fmaxf(rintf(y), 0.0f), 255.0f);   // (between s and e already; the clamp only keeps a NaN alpha off the conversion)
    return (uint8_t)(a == 0.0f ? s : (a == 1.0f ? rintf(e) : b));
}

// VEC: 4 pixels per thread -- three 8-byte loads of the video, one 16-byte load of alpha, the 12 source / output bytes as three dwords
// (HW % 4 == 0 keeps the four inside one frame and every access aligned).  Scalar: one pixel per thread.
template <bool VEC>
__global__ __launch_bounds__(CP_THREADS) void composite_kernel(const half_t* __restrict__ video, const uint8_t* __restrict__ src,
                                                               const float* __restrict__ alpha, int mask_frames,
                                                               const long long* __restrict__ rec, uint8_t* __restrict__ out, int F, int HW) {
    __shared__ long long sums[CP_RECORD];
    __shared__ float gb[6];
    const bool match = rec != nullptr;
    if (match) {   // every block folds the records itself, in record order, and forms the same gain and bias
        if (threadIdx.x < 15) {
            long long t = 0;
            for (int b = 0; b < CP_BLOCKS; ++b) t += rec[b * CP_RECORD + threadIdx.x];
            sums[threadIdx.x] = t;
        }
        __syncthreads();
        if (threadIdx.x < 3) {
            const long long* q = sums + 5 * threadIdx.x;
            const double cnt = (double)q[0];
            double gain = 1.0, bias = 0.0;
            if (q[0] >= 64) {
                const double me = (double)q[1] / cnt, ms = (double)q[3] / cnt;
                const double ve = fmax((double)q[2] / cnt - me * me, 0.0), vs = fmax((double)q[4] / cnt - ms * ms, 0.0);
                if (ve > 0.0) {
                    gain = fmin(fmax(sqrt(vs) / sqrt(ve), 0.5), 2.0);
                    bias = ms - gain * me;
                }
            }
            gb[threadIdx.x] = (float)gain;
            gb[3 + threadIdx.x] = (float)bias;
        }
        __syncthreads();
    }
    const int per = VEC ? 4 : 1;
    const long long p = ((long long)blockIdx.x * CP_THREADS + threadIdx.x) * per;
    if (p >= (long long)F * HW) return;
    const int f = (int)(p / HW), hw = (int)(p - (long long)f * HW);
    const long long ai = mask_frames == 1 ? hw : p;
    if (VEC) {
        const f4 av = *(const f4*)(alpha + ai);
        const uint32_t* s4 = (const uint32_t*)(src + 3 * p);
        const uint32_t sw[3] = {s4[0], s4[1], s4[2]};
        uint32_t ow[3] = {0u, 0u, 0u};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const h4 vv = *(const h4*)(video + ((long long)c * F + f) * HW + hw);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const int byte = 3 * k + c;
                const uint8_t sb = (uint8_t)(sw[byte >> 2] >> (8 * (byte & 3)));
                const uint8_t o = composite_one(vv[k], sb, av[k], match, match ? gb[c] : 1.0f, match ? gb[3 + c] : 0.0f);
                ow[byte >> 2] |= (uint32_t)o << (8 * (byte & 3));
            }
        }
        uint32_t* o4 = (uint32_t*)(out + 3 * p);
        o4[0] = ow[0];
        o4[1] = ow[1];
        o4[2] = ow[2];
    } else {
        const float a = alpha[ai];
#pragma unroll
        for (int c = 0; c < 3; ++c)
            out[3 * p + c] = composite_one(video[((long long)c * F + f) * HW + hw], src[3 * p + c], a, match, match ? gb[c] : 1.0f,
                                           match ? gb[3 + c] : 0.0f);
    }
}

extern "C" int anyv2v_pixel_alpha_f16(const void* latent_mask, int32_t mask_frames, int32_t h, int32_t w, int32_t grow_px, const float* taps,
                                      int32_t R, float* workspace, float* alpha, void* stream) {
    AV_CHECK(latent_mask && workspace && alpha, "pixel_alpha: null pointer");
    AV_CHECK(mask_frames >= 1 && h >= 1 && w >= 1, "pixel_alpha: mask_frames = %d, h = %d, w = %d: all at least 1", mask_frames, h, w);
    AV_CHECK(grow_px >= 0 && grow_px <= CP_MAX_GROW, "pixel_alpha: grow_px = %d must lie in [0, %d]", grow_px, CP_MAX_GROW);
    AV_CHECK(R >= 0 && R <= CP_MAX_R, "pixel_alpha: R = %d must lie in [0, %d]", R, CP_MAX_R);
    AV_CHECK(R == 0 || taps, "pixel_alpha: null pointer (R > 0 needs the 2 R + 1 taps)");
    AV_CHECK((long long)mask_frames * h * w < (1ll << 25), "pixel_alpha: 64 * mask_frames * h * w (the alpha plane) must fit an int");
    AV_CHECK((const void*)workspace != (const void*)alpha, "pixel_alpha: the workspace may not be the output");
    AlphaTaps tp;
    for (int i = 0; i < 2 * CP_MAX_R + 1; ++i) tp.t[i] = 0.0f;
    for (int i = 0; i < 2 * R + 1 && R > 0; ++i) {
        AV_CHECK(isfinite(taps[i]) && taps[i] >= 0.0f && taps[i] <= 1.0f, "pixel_alpha: tap %d is not a weight in [0, 1]", i);
        tp.t[i] = taps[i];
    }
    const int H = 8 * h, W = 8 * w, n = mask_frames * H * W, nd = mask_frames * h * W;
    const dim3 block(CP_THREADS), grid_n((unsigned)((n + CP_THREADS - 1) / CP_THREADS));
    hipStream_t st = (hipStream_t)stream;
    float* code = workspace;        // [Fm, H, W]
    float* rows = workspace + n;    // [Fm, H, W]; before the feather its head holds the row distances [Fm, h, W]
    hipLaunchKernelGGL(alpha_row_dist_kernel, dim3((unsigned)((nd + CP_THREADS - 1) / CP_THREADS)), block, 0, st, (const half_t*)latent_mask, nd,
                       w, grow_px + R, rows);
    if (R == 0) {
        hipLaunchKernelGGL(alpha_dilate_kernel<true>, grid_n, block, 0, st, (const float*)rows, n, h, w, grow_px, grow_px, alpha);
        return av_launch_status("pixel_alpha");
    }
    hipLaunchKernelGGL(alpha_dilate_kernel<false>, grid_n, block, 0, st, (const float*)rows, n, h, w, grow_px, grow_px + R, code);
    const int tiles = (W + CP_THREADS - 1) / CP_THREADS;
    hipLaunchKernelGGL(alpha_row_feather_kernel, dim3((unsigned)(mask_frames * H * tiles)), block, 0, st, (const float*)code, W, tiles, R, tp, rows);
    const int nc = n / CP_YB;
    hipLaunchKernelGGL(alpha_col_feather_kernel, dim3((unsigned)((nc + CP_THREADS - 1) / CP_THREADS)), block, 0, st, (const float*)rows,
                       (const float*)code, nc, H, W, R, tp, alpha);
    return av_launch_status("pixel_alpha");
}

static int composite_shape_ok(const char* what, int32_t mask_frames, int32_t F, int32_t H, int32_t W) {
    AV_CHECK(F > 0 && H > 0 && W > 0, "%s: bad arguments (F = %d, H = %d, W = %d)", what, F, H, W);
    AV_CHECK(mask_frames == 1 || mask_frames == F, "%s: mask_frames = %d must be 1 or F = %d", what, mask_frames, F);
    AV_CHECK(3ll * F * H * W < (1ll << 31), "%s: 3 * F * H * W must fit an int", what);
    return ANYV2V_OK;
}

extern "C" int anyv2v_composite_stats_u8(const void* video, const void* source, const float* alpha, int32_t mask_frames, int32_t F, int32_t H,
                                         int32_t W, int64_t* records, void* stream) {
    AV_CHECK(video && source && alpha && records, "composite_stats: null pointer");
    if (int rc = composite_shape_ok("composite_stats", mask_frames, F, H, W)) return rc;
    AV_CHECK((((uintptr_t)records) & 7) == 0, "composite_stats: records must be 8-byte aligned");
    hipLaunchKernelGGL(composite_stats_kernel, dim3(CP_BLOCKS), dim3(CP_THREADS), 0, (hipStream_t)stream, (const half_t*)video,
                       (const uint8_t*)source, alpha, mask_frames, F, H * W, (long long*)records);
    return av_launch_status("composite_stats");
}

extern "C" int anyv2v_composite_u8(const void* video, const void* source, const float* alpha, int32_t mask_frames, const int64_t* records,
                                   void* out, int32_t F, int32_t H, int32_t W, void* stream) {
    AV_CHECK(video && source && alpha && out, "composite: null pointer");
    if (int rc = composite_shape_ok("composite", mask_frames, F, H, W)) return rc;
    AV_CHECK(out != source && out != video && out != (const void*)alpha && out != (const void*)records, "composite: out may not alias an input");
    AV_CHECK((((uintptr_t)records) & 7) == 0, "composite: records must be 8-byte aligned");
    const int HW = H * W;
    const long long n = (long long)F * HW;
    const bool vec = HW % 4 == 0 && (((uintptr_t)video) & 7) == 0 && av_aligned16(alpha) && (((uintptr_t)source) & 3) == 0 && (((uintptr_t)out) & 3) == 0;
    const long long threads = vec ? n / 4 : n;
    const dim3 grid((unsigned)((threads + CP_THREADS - 1) / CP_THREADS)), block(CP_THREADS);
    if (vec)
        hipLaunchKernelGGL(composite_kernel<true>, grid, block, 0, (hipStream_t)stream, (const half_t*)video, (const uint8_t*)source, alpha,
                           mask_frames, (const long long*)records, (uint8_t*)out, F, HW);
    else
        hipLaunchKernelGGL(composite_kernel<false>, grid, block, 0, (hipStream_t)stream, (const half_t*)video, (const uint8_t*)source, alpha,
                           mask_frames, (const long long*)records, (uint8_t*)out, F, HW);
    return av_launch_status("composite");
}
