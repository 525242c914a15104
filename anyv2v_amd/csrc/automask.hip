// Automatic edit masks for the masked PnP edit (DiffEdit, Couairon et al., arXiv 2210.11427; diffusers'
// StableDiffusionDiffEditPipeline.generate_mask): where do the UNet's predictions under the source and under the edit conditioning
// differ?  Nothing in the reference does this; include/anyv2v_hip.h holds the definition.
//   diff_map_accum_kernel   acc[p] (+)= sum_c |V_tgt[p, c] - V_src[p, c]| from the UNet's token-layout output, one thread per pixel
//   diff_map_sum_kernel     partial sums of acc, one record per block of a fixed grid
//   diff_map_finish_kernel  folds the records in fp64, in record order, into the clip mean; map = fp16(clamp(ratio acc / mean, 0, 1)),
//                           mask = map > threshold, written at the pixel size (each latent pixel over its 8 x 8 block)
// No atomics and a fixed grid for the mean: the records, their fold and therefore map and mask are bit-reproducible.  Every output element
// is written exactly once by one thread; the padding columns C .. ldv - 1 of V are never read.
#include "common.h"

#include <math.h>

#define DM_BLOCKS ANYV2V_DIFF_MAP_BLOCKS
#define DM_THREADS ANYV2V_DIFF_MAP_THREADS

// first_dev != nullptr: the flag is read from the device (one captured graph serves the first map and the following ones)
__global__ __launch_bounds__(DM_THREADS) void diff_map_accum_kernel(const half_t* __restrict__ V, int ldv, int C, int npix, float* acc,
                                                                    int first, const int32_t* __restrict__ first_dev) {
    const int p = blockIdx.x * DM_THREADS + threadIdx.x;
    if (p >= npix) return;
    const half_t* ps = V + (long long)p * ldv;
    const half_t* pt = V + ((long long)npix + p) * ldv;
    float s = 0.0f;
    for (int c = 0; c < C; ++c) s += fabsf((float)pt[c] - (float)ps[c]);   // exact difference of two fp16 values; channels in order
    const bool overwrite = first_dev != nullptr ? (first_dev[0] != 0) : (first != 0);
    acc[p] = overwrite ? s : acc[p] + s;
}

__global__ __launch_bounds__(DM_THREADS) void diff_map_sum_kernel(const float* __restrict__ acc, int npix, float* __restrict__ rec) {
    __shared__ float red[DM_THREADS / WAVE];
    float s = 0.0f;
    for (int p = blockIdx.x * DM_THREADS + threadIdx.x; p < npix; p += DM_BLOCKS * DM_THREADS) s += acc[p];
    s = wave_sum(s);
    if ((threadIdx.x & (WAVE - 1)) == 0) red[threadIdx.x / WAVE] = s;
    __syncthreads();
    if (threadIdx.x == 0) {
        float t = 0.0f;
        for (int i = 0; i < DM_THREADS / WAVE; ++i) t += red[i];   // wave order: fixed
        rec[blockIdx.x] = t;
    }
}

__device__ __forceinline__ half_t diff_map_value(float a, float scale) {
    return (half_t)fminf(fmaxf(a * scale, 0.0f), 1.0f);   // (a NaN product comes out as 0; scale is 0 when the mean is 0)
}

// VEC: 8 latent pixels of one row per thread -- two 16-byte loads of acc, one 16-byte store of the map, four 16-byte stores per pixel row
// of the mask (w % 8 == 0 keeps the eight inside one row).  Scalar: one latent pixel per thread, byte stores.
template <bool VEC>
__global__ __launch_bounds__(DM_THREADS) void diff_map_finish_kernel(const float* __restrict__ acc, const float* __restrict__ rec, int npix, int h,
                                                                     int w, float ratio, float thr, half_t* __restrict__ map,
                                                                     uint8_t* __restrict__ mask) {
    __shared__ float recs[DM_BLOCKS];
    for (int i = threadIdx.x; i < DM_BLOCKS; i += DM_THREADS) recs[i] = rec[i];
    __syncthreads();
    double sum = 0.0;
    for (int b = 0; b < DM_BLOCKS; ++b) sum += (double)recs[b];   // record order: every thread of every block forms the same value
    const double mean = sum / (double)npix;
    const float scale = mean > 0.0 ? (float)((double)ratio / mean) : 0.0f;
    const int per = VEC ? 8 : 1;
    const int i = (blockIdx.x * DM_THREADS + threadIdx.x) * per;
    if (i >= npix) return;
    const int x = i % w, y = (i / w) % h, f = i / (w * h);
    const long long W = 8ll * w;
    uint8_t* m0 = mask + ((long long)f * h * 8 + (long long)y * 8) * W + 8ll * x;
    if (VEC) {
        const f4 a0 = *(const f4*)(acc + i), a1 = *(const f4*)(acc + i + 4);
        h8 mv;
        uint32_t bits[16];   // 64 mask bytes of one pixel row: byte 8 e + k is latent pixel e
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            mv[e] = diff_map_value(e < 4 ? a0[e] : a1[e - 4], scale);
            const uint32_t on = (float)mv[e] > thr ? 0x01010101u : 0u;
            bits[2 * e] = on;
            bits[2 * e + 1] = on;
        }
        *(h8*)(map + i) = mv;
        for (int r = 0; r < 8; ++r) {
            u4* row = (u4*)(m0 + r * W);
#pragma unroll
            for (int q = 0; q < 4; ++q) row[q] = u4{bits[4 * q], bits[4 * q + 1], bits[4 * q + 2], bits[4 * q + 3]};
        }
    } else {
        const half_t v = diff_map_value(acc[i], scale);
        map[i] = v;
        const uint8_t on = (float)v > thr ? 1 : 0;
        for (int r = 0; r < 8; ++r)
            for (int c = 0; c < 8; ++c) m0[r * W + c] = on;
    }
}

extern "C" int anyv2v_diff_map_accum_f16(const void* Vtok, int32_t ldv, int32_t C, int32_t F, int32_t HW, float* acc, int32_t first,
                                         const int32_t* first_dev, void* stream) {
    AV_CHECK(Vtok && acc, "diff_map_accum: null pointer");
    AV_CHECK(C > 0 && F > 0 && HW > 0 && ldv >= C, "diff_map_accum: bad arguments (C = %d, F = %d, HW = %d, ldv = %d: all positive, ldv >= C)", C, F,
             HW, ldv);
    AV_CHECK((long long)F * HW < (1ll << 30), "diff_map_accum: 2 * F * HW must fit an int");
    AV_CHECK(first == 0 || first == 1, "diff_map_accum: first = %d must be 0 or 1", first);
    const int npix = F * HW;
    hipLaunchKernelGGL(diff_map_accum_kernel, dim3((unsigned)((npix + DM_THREADS - 1) / DM_THREADS)), dim3(DM_THREADS), 0, (hipStream_t)stream,
                       (const half_t*)Vtok, ldv, C, npix, acc, first, first_dev);
    return av_launch_status("diff_map_accum");
}

extern "C" int anyv2v_diff_map_finish_f16(const float* acc, int32_t F, int32_t h, int32_t w, float ratio, float threshold, float* records,
                                          void* map, void* pixel_mask, void* stream) {
    AV_CHECK(acc && records && map && pixel_mask, "diff_map_finish: null pointer");
    AV_CHECK(F > 0 && h > 0 && w > 0, "diff_map_finish: bad arguments (F = %d, h = %d, w = %d)", F, h, w);
    AV_CHECK((long long)F * h * w < (1ll << 25), "diff_map_finish: 64 * F * h * w (the pixel mask) must fit an int");
    AV_CHECK(isfinite(ratio) && ratio > 0.0f, "diff_map_finish: ratio = %g must be finite and > 0", (double)ratio);
    AV_CHECK(isfinite(threshold) && threshold > 0.0f && threshold < 1.0f, "diff_map_finish: threshold = %g must lie in (0, 1)", (double)threshold);
    const int npix = F * h * w;
    const float thr = (float)(half_t)threshold;   // the comparison is made in fp16: on the rounded map, against the rounded threshold
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(diff_map_sum_kernel, dim3(DM_BLOCKS), dim3(DM_THREADS), 0, st, acc, npix, records);
    const bool vec = w % 8 == 0 && av_aligned16(acc) && av_aligned16(map) && av_aligned16(pixel_mask);
    const int threads = vec ? npix / 8 : npix;
    const dim3 grid((unsigned)((threads + DM_THREADS - 1) / DM_THREADS)), block(DM_THREADS);
    if (vec)
        hipLaunchKernelGGL(diff_map_finish_kernel<true>, grid, block, 0, st, acc, (const float*)records, npix, h, w, ratio, thr, (half_t*)map,
                           (uint8_t*)pixel_mask);
    else
        hipLaunchKernelGGL(diff_map_finish_kernel<false>, grid, block, 0, st, acc, (const float*)records, npix, h, w, ratio, thr, (half_t*)map,
                           (uint8_t*)pixel_mask);
    return av_launch_status("diff_map_finish");
}
