// The two passes of Pillow's 8-bit `Image.resize` (include/anyv2v_hip.h holds the definition; resample_plan.cpp builds the tables):
//   out = clamp((2^21 + sum over x < n of in[xmin + x] * k[x]) >> 22, 0, 255)      int32, per band
// All integers: every result is the same whatever the thread order, so both kernels are tested bit for bit against Pillow.
//   resample_v_kernel   block row = output row: (xmin, n) and the coefficients are uniform (scalar loads); a thread owns 4 bytes of the row
//                       and walks the n input rows, each read a coalesced row segment
//   resample_h_kernel   block = one input row x RS_THREADS output pixels: the input span of the segment is staged in LDS by coalesced
//                       dword loads, then a thread per output pixel walks its taps from LDS
// Rows are W * C bytes, usually no multiple of 4, and the pointers carry no alignment: a dword is loaded where all four bytes are wanted and
// the address allows (directly when aligned, as two aligned dwords and a byte-align when both lie inside the operand), bytes otherwise.
// No atomics; every output byte is written once by one thread.
#include "resample_common.h"   // RS_*, rs_mad, rs_finish, rs_load4 (shared with restore.hip)

// grid (ceil(ceil(RB / 4) / RS_THREADS), out_h, F), RB = W * C bytes per row
__global__ __launch_bounds__(RS_THREADS) void resample_v_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, long long RB,
                                                                int out_h, const int* __restrict__ bounds, const int* __restrict__ coeffs,
                                                                int ksize, long long src_bytes) {
    const int oy = blockIdx.y, f = blockIdx.z;
    const long long b = ((long long)blockIdx.x * RS_THREADS + threadIdx.x) * 4;
    if (b >= RB) return;
    const int nb = RB - b < 4 ? (int)(RB - b) : 4;
    int y0 = bounds[2 * oy], y1 = y0 + bounds[2 * oy + 1];   // cut to the side: no table can make a read leave src
    y0 = min(max(y0, 0), H);
    y1 = min(max(y1, y0), H);
    const int skip = y0 - bounds[2 * oy];
    const int n = min(y1 - y0, ksize - skip);
    const int* k = coeffs + (long long)oy * ksize + skip;
    const uint8_t* p = src + ((long long)f * H + y0) * RB + b;
    int acc[4] = {RS_HALF, RS_HALF, RS_HALF, RS_HALF};
    if (nb == 4) {
        for (int t = 0; t < n; ++t, p += RB) {
            const uint32_t v = rs_load4(p, src, src + src_bytes);
            const int kt = k[t];
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] = rs_mad(acc[j], (v >> (8 * j)) & 0xffu, kt);
        }
    } else {
        for (int t = 0; t < n; ++t, p += RB) {
            const int kt = k[t];
#pragma unroll
            for (int j = 0; j < 3; ++j)
                if (j < nb) acc[j] = rs_mad(acc[j], p[j], kt);
        }
    }
    uint8_t* o = dst + ((long long)f * out_h + oy) * RB + b;
    if (nb == 4 && ((uintptr_t)o & 3) == 0) {
        *(uint32_t*)o = rs_finish(acc[0]) | (rs_finish(acc[1]) << 8) | (rs_finish(acc[2]) << 16) | (rs_finish(acc[3]) << 24);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nb) o[j] = (uint8_t)rs_finish(acc[j]);
    }
}

// grid (ceil(out_w / THREADS), rows, F); dynamic LDS: cap_px * C + 4 bytes rounded up to dwords, cap_px = min(W, THREADS * ksize) -- the
// span of THREADS consecutive outputs of a table of resample_plan.cpp is at most (THREADS - 1) * scale + 2 sup + 1 <= THREADS * ksize pixels
// (a wider one is cut to cap_px).  LDS byte a + i holds byte i of the span, a = the span's address mod 4, so that the staging dwords are
// aligned in memory and in LDS alike.
template <int C>
__global__ __launch_bounds__(RS_THREADS) void resample_h_kernel(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, int H, int W,
                                                                int row0, int rows, int out_w, const int* __restrict__ bounds,
                                                                const int* __restrict__ coeffs, int ksize, int cap_px) {
    extern __shared__ uint32_t span_s[];
    const int r = blockIdx.y, f = blockIdx.z, nthreads = blockDim.x;
    const int ox_first = blockIdx.x * nthreads, ox_last = min(ox_first + nthreads, out_w) - 1;
    int lo = bounds[2 * ox_first], hi = bounds[2 * ox_last] + bounds[2 * ox_last + 1];
    lo = min(max(lo, 0), W);
    hi = min(max(hi, lo), W);
    hi = min(hi, lo + cap_px);
    const uint8_t* g = src + (((long long)f * H + row0 + r) * W + lo) * C;   // the span: (hi - lo) * C bytes from here
    const int span_bytes = (hi - lo) * C;
    const int a = (int)((uintptr_t)g & 3);
    uint8_t* span_b = (uint8_t*)span_s;
    for (int j = threadIdx.x; 4 * j < a + span_bytes; j += nthreads) {
        const int i0 = 4 * j - a;   // span byte of this dword's first byte
        if (i0 >= 0 && i0 + 4 <= span_bytes) {
            span_s[j] = *(const uint32_t*)(g + i0);
        } else {
            for (int i = max(i0, 0); i < min(i0 + 4, span_bytes); ++i) span_b[a + i] = g[i];
        }
    }
    __syncthreads();
    const int ox = ox_first + threadIdx.x;
    if (ox >= out_w) return;
    int x0 = bounds[2 * ox], x1 = x0 + bounds[2 * ox + 1];
    x0 = min(max(x0, lo), hi);   // cut to the staged span (a table of the planner's lies inside it)
    x1 = min(max(x1, x0), hi);
    const int skip = x0 - bounds[2 * ox];
    const int n = min(x1 - x0, ksize - skip);
    const int* k = coeffs + (long long)ox * ksize + skip;
    const uint8_t* s = span_b + a + (x0 - lo) * C;
    int acc[C];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = RS_HALF;
    for (int t = 0; t < n; ++t) {
        const int kt = k[t];
#pragma unroll
        for (int c = 0; c < C; ++c) acc[c] = rs_mad(acc[c], s[t * C + c], kt);
    }
    uint8_t* o = dst + ((((long long)f * rows + r) * out_w) + ox) * C;
#pragma unroll
    for (int c = 0; c < C; ++c) o[c] = (uint8_t)rs_finish(acc[c]);
}

static int resample_args_ok(const char* what, const void* src, const void* dst, int32_t F, int32_t H, int32_t W, int32_t C, int32_t out,
                            const int32_t* bounds, const int32_t* coeffs, int32_t ksize) {
    AV_CHECK(src && dst && bounds && coeffs, "%s: null pointer", what);
    AV_CHECK(F >= 1 && F <= 65535, "%s: F = %d must lie in [1, 65535]", what, F);
    AV_CHECK(H >= 1 && H <= ANYV2V_RESAMPLE_MAX_SIDE && W >= 1 && W <= ANYV2V_RESAMPLE_MAX_SIDE, "%s: H x W = %d x %d: both in [1, %d]", what, H, W,
             ANYV2V_RESAMPLE_MAX_SIDE);
    AV_CHECK(C == 1 || C == 3, "%s: C = %d must be 1 or 3", what, C);
    AV_CHECK(out >= 1 && out <= ANYV2V_RESAMPLE_MAX_SIDE, "%s: output size %d must lie in [1, %d]", what, out, ANYV2V_RESAMPLE_MAX_SIDE);
    AV_CHECK(ksize >= 1, "%s: ksize = %d must be at least 1", what, ksize);
    AV_CHECK((((uintptr_t)bounds) & 3) == 0 && (((uintptr_t)coeffs) & 3) == 0, "%s: the tables must be 4-byte aligned", what);
    return ANYV2V_OK;
}

static bool resample_overlap(const void* a, long long na, const void* b, long long nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

extern "C" int anyv2v_resample_h_u8(const void* src, void* dst, int32_t F, int32_t H, int32_t W, int32_t C, int32_t row0, int32_t rows,
                                    int32_t out_w, const int32_t* bounds, const int32_t* coeffs, int32_t ksize, void* stream) {
    if (int rc = resample_args_ok("resample_h", src, dst, F, H, W, C, out_w, bounds, coeffs, ksize)) return rc;
    AV_CHECK(row0 >= 0 && rows >= 1 && row0 <= H - rows, "resample_h: rows [%d, %d + %d) must lie inside H = %d", row0, row0, rows, H);
    AV_CHECK(!resample_overlap(src, (long long)F * H * W * C, dst, (long long)F * rows * out_w * C), "resample_h: dst may not overlap src");
    const int threads = out_w <= 64 ? 64 : out_w <= 128 ? 128 : RS_THREADS;
    const long long cap = (long long)threads * ksize < W ? (long long)threads * ksize : W;
    const size_t lds = (size_t)((cap * C + 4 + 3) / 4 * 4);   // <= 16384 * 3 + 8 bytes
    const dim3 grid((unsigned)((out_w + threads - 1) / threads), (unsigned)rows, (unsigned)F);
    if (C == 3)
        hipLaunchKernelGGL(resample_h_kernel<3>, grid, dim3(threads), lds, (hipStream_t)stream, (const uint8_t*)src, (uint8_t*)dst, H, W, row0,
                           rows, out_w, bounds, coeffs, ksize, (int)cap);
    else
        hipLaunchKernelGGL(resample_h_kernel<1>, grid, dim3(threads), lds, (hipStream_t)stream, (const uint8_t*)src, (uint8_t*)dst, H, W, row0,
                           rows, out_w, bounds, coeffs, ksize, (int)cap);
    return av_launch_status("resample_h");
}

extern "C" int anyv2v_resample_v_u8(const void* src, void* dst, int32_t F, int32_t H, int32_t W, int32_t C, int32_t out_h, const int32_t* bounds,
                                    const int32_t* coeffs, int32_t ksize, void* stream) {
    if (int rc = resample_args_ok("resample_v", src, dst, F, H, W, C, out_h, bounds, coeffs, ksize)) return rc;
    const long long RB = (long long)W * C, src_bytes = (long long)F * H * RB;
    AV_CHECK(!resample_overlap(src, src_bytes, dst, (long long)F * out_h * RB), "resample_v: dst may not overlap src");
    const long long groups = (RB + 3) / 4;
    const dim3 grid((unsigned)((groups + RS_THREADS - 1) / RS_THREADS), (unsigned)out_h, (unsigned)F);
    hipLaunchKernelGGL(resample_v_kernel, grid, dim3(RS_THREADS), 0, (hipStream_t)stream, (const uint8_t*)src, (uint8_t*)dst, H, RB, out_h, bounds,
                       coeffs, ksize, src_bytes);
    return av_launch_status("resample_v");
}
