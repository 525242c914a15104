// Detail-preserving restore (include/anyv2v_hip.h holds the definition): the way back of restore.hip with the fine detail of the source,
// S - up(P), added to the upscaled edit wherever a gate says that the edit E stayed close to the prepared source P.
//   detail_rowsum_kernel   c = max over the bands of |E - P| per pixel, summed over the 2 radius + 1 columns of the box (clamped to the row)
//                          into a uint16 intermediate: a block owns RS_THREADS pixels of one row and forms c once per pixel, halo included,
//                          in LDS
//   detail_gate_kernel     the column sums of the intermediate (rows clamped to the frame: uniform per block), the rounded mean and the
//                          ramp between lo and hi -> G uint8 [F, h, w]
//   restore_detail_kernel  restore_paste_kernel's sibling: block row = output row, both tables through uniform (scalar) loads, a thread owns
//                          4 bytes of the row, walks the edit's and the prepared source's intermediates together with the same (ymin, n, k),
//                          forms gate and alpha at the at most two pixels it touches, and pastes
// All integers: every result is the same whatever the thread order.  No atomics; every output byte is written once by one thread.
#include "resample_common.h"

// grid (ceil(w / RS_THREADS), h, F)
__global__ __launch_bounds__(RS_THREADS) void detail_rowsum_kernel(const uint8_t* __restrict__ edit, const uint8_t* __restrict__ prep,
                                                                   uint16_t* __restrict__ rows, int w, int radius) {
    __shared__ uint8_t c[RS_THREADS + 2 * ANYV2V_DETAIL_MAX_RADIUS];
    const int x0 = blockIdx.x * RS_THREADS;
    const long long row = ((long long)blockIdx.z * gridDim.y + blockIdx.y) * w;
    const uint8_t* e = edit + row * 3;
    const uint8_t* p = prep + row * 3;
    for (int i = threadIdx.x; i < RS_THREADS + 2 * radius; i += RS_THREADS) {
        const int x = min(max(x0 - radius + i, 0), w - 1);   // replicate edge: no read leaves the row
        int m = 0;
#pragma unroll
        for (int j = 0; j < 3; ++j) m = max(m, abs((int)e[3 * x + j] - (int)p[3 * x + j]));
        c[i] = (uint8_t)m;
    }
    __syncthreads();
    const int x = x0 + threadIdx.x;
    if (x >= w) return;
    uint32_t s = 0;
    for (int i = 0; i <= 2 * radius; ++i) s += c[threadIdx.x + i];
    rows[row + x] = (uint16_t)s;   // <= 255 * 33 < 65536
}

// grid (ceil(w / RS_THREADS), h, F)
__global__ __launch_bounds__(RS_THREADS) void detail_gate_kernel(const uint16_t* __restrict__ rows, uint8_t* __restrict__ gate, int h, int w,
                                                                 int lo, int hi, int radius) {
    const int x = blockIdx.x * RS_THREADS + threadIdx.x, y = blockIdx.y;
    if (x >= w) return;
    const uint16_t* r = rows + (long long)blockIdx.z * h * w + x;
    uint32_t b = 0;
    for (int dy = -radius; dy <= radius; ++dy) b += r[(long long)min(max(y + dy, 0), h - 1) * w];
    const uint32_t n = (uint32_t)((2 * radius + 1) * (2 * radius + 1));
    const int mean = (int)((b + n / 2) / n);
    const int g = mean <= lo ? 255 : mean >= hi ? 0 : (255 * (hi - mean) + (hi - lo) / 2) / (hi - lo);
    gate[((long long)blockIdx.z * h + y) * w + x] = (uint8_t)g;
}

// grid (ceil(ceil(RB / 4) / RS_THREADS), sh, F), RB = 3 * sw bytes per row of source and out, EB = 3 * dw bytes per row of eh and ph
__global__ __launch_bounds__(RS_THREADS) void restore_detail_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ eh,
                                                                    const uint8_t* __restrict__ ph, const uint8_t* __restrict__ gh,
                                                                    const uint8_t* __restrict__ ah, uint8_t* __restrict__ out, int sh, int RB,
                                                                    int dx0, int dy0, int dw, int dh, int e_rows,
                                                                    const int* __restrict__ e_bounds, const int* __restrict__ e_coeffs,
                                                                    int e_ksize, int g_per_frame, int a_per_frame, int a_rows,
                                                                    const int* __restrict__ a_bounds, const int* __restrict__ a_coeffs,
                                                                    int a_ksize, long long src_bytes, long long eh_bytes) {
    const int oy = blockIdx.y, f = blockIdx.z;
    const int b = (blockIdx.x * RS_THREADS + threadIdx.x) * 4;
    if (b >= RB) return;
    const int nb = RB - b < 4 ? RB - b : 4;
    const long long at = ((long long)f * sh + oy) * RB + b;
    const uint8_t* sp = src + at;
    uint32_t s = 0;
    if (nb == 4) {
        s = rs_load4(sp, src, src + src_bytes);
    } else {
#pragma unroll
        for (int j = 0; j < 3; ++j)
            if (j < nb) s |= (uint32_t)sp[j] << (8 * j);
    }
    uint32_t res = s;
    const int r = oy - dy0, EB = 3 * dw;
    const int e0 = b - 3 * dx0;   // the byte of eh's and ph's row under this thread's first byte
    if (r >= 0 && r < dh && e0 + nb > 0 && e0 < EB) {
        int y0 = e_bounds[2 * r], y1 = y0 + e_bounds[2 * r + 1];   // cut to the intermediates: no table can make a read leave them
        y0 = min(max(y0, 0), e_rows);
        y1 = min(max(y1, y0), e_rows);
        const int skip = y0 - e_bounds[2 * r];
        const int n = min(y1 - y0, e_ksize - skip);
        const int* k = e_coeffs + (long long)r * e_ksize + skip;
        const long long eoff = ((long long)f * e_rows + y0) * EB + e0;
        const uint8_t* pe = eh + eoff;
        const uint8_t* pp = ph + eoff;
        int acc[4] = {RS_HALF, RS_HALF, RS_HALF, RS_HALF}, pacc[4] = {RS_HALF, RS_HALF, RS_HALF, RS_HALF};
        if (nb == 4 && e0 >= 0 && e0 + 4 <= EB) {
            for (int t = 0; t < n; ++t, pe += EB, pp += EB) {
                const uint32_t v = rs_load4(pe, eh, eh + eh_bytes), u = rs_load4(pp, ph, ph + eh_bytes);
                const int kt = k[t];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    acc[j] = rs_mad(acc[j], (v >> (8 * j)) & 0xffu, kt);
                    pacc[j] = rs_mad(pacc[j], (u >> (8 * j)) & 0xffu, kt);
                }
            }
        } else {   // the group straddles an edge of dest (or the row's end): the bytes inside, one by one
            for (int t = 0; t < n; ++t, pe += EB, pp += EB) {
                const int kt = k[t];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nb && e0 + j >= 0 && e0 + j < EB) {
                        acc[j] = rs_mad(acc[j], pe[j], kt);
                        pacc[j] = rs_mad(pacc[j], pp[j], kt);
                    }
            }
        }
        // gate and alpha at the (at most two) pixels the group's bytes inside dest belong to: one table, one row range
        const int c0 = max(e0, 0) / 3, c1 = min(e0 + 3, EB - 1) / 3;
        int ay0 = a_bounds[2 * r], ay1 = ay0 + a_bounds[2 * r + 1];
        ay0 = min(max(ay0, 0), a_rows);
        ay1 = min(max(ay1, ay0), a_rows);
        const int askip = ay0 - a_bounds[2 * r];
        const int an = min(ay1 - ay0, a_ksize - askip);
        const int* ak = a_coeffs + (long long)r * a_ksize + askip;
        const uint8_t* pg = gh + ((long long)(g_per_frame ? f : 0) * a_rows + ay0) * dw;
        int g0 = RS_HALF, g1 = RS_HALF;
        uint32_t m0 = 255u, m1 = 255u;
        if (ah != nullptr) {
            const uint8_t* pa = ah + ((long long)(a_per_frame ? f : 0) * a_rows + ay0) * dw;
            int a0 = RS_HALF, a1 = RS_HALF;
            for (int t = 0; t < an; ++t, pg += dw, pa += dw) {
                const int kt = ak[t];
                g0 = rs_mad(g0, pg[c0], kt);
                g1 = rs_mad(g1, pg[c1], kt);
                a0 = rs_mad(a0, pa[c0], kt);
                a1 = rs_mad(a1, pa[c1], kt);
            }
            m0 = rs_finish(a0);
            m1 = rs_finish(a1);
        } else {
            for (int t = 0; t < an; ++t, pg += dw) {
                const int kt = ak[t];
                g0 = rs_mad(g0, pg[c0], kt);
                g1 = rs_mad(g1, pg[c1], kt);
            }
        }
        const int w0 = (int)rs_finish(g0), w1 = (int)rs_finish(g1);
        const int wt0 = w0 + (w0 >> 7), wt1 = w1 + (w1 >> 7);   // 0 .. 256, 255 -> 256
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int pos = e0 + j;
            if (j < nb && pos >= 0 && pos < EB) {
                const bool first = pos < 3 * (c0 + 1);
                const uint32_t m = first ? m0 : m1;
                const int wt = first ? wt0 : wt1;
                const int d = (int)((s >> (8 * j)) & 0xffu);
                const int add = ((d - (int)rs_finish(pacc[j])) * wt + 128) >> 8;
                const uint32_t e2 = (uint32_t)min(max((int)rs_finish(acc[j]) + add, 0), 255);
                const uint32_t t = (uint32_t)d * (255u - m) + e2 * m + 128u;
                res = (res & ~(0xffu << (8 * j))) | ((((t >> 8) + t) >> 8) << (8 * j));
            }
        }
    }
    uint8_t* o = out + at;
    if (nb == 4 && ((uintptr_t)o & 3) == 0) {
        *(uint32_t*)o = res;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j < nb) o[j] = (uint8_t)(res >> (8 * j));
    }
}

static bool detail_overlap(const void* a, long long na, const void* b, long long nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

extern "C" int anyv2v_detail_gate_u8(const void* edit, const void* prepared, void* gate_out, int32_t F, int32_t h, int32_t w, int32_t lo,
                                     int32_t hi, int32_t radius, void* scratch, int64_t scratch_bytes, void* stream) {
    AV_CHECK(edit && prepared && gate_out && scratch, "detail_gate: null pointer");
    AV_CHECK(F >= 1 && F <= 65535, "detail_gate: F = %d must lie in [1, 65535]", F);
    AV_CHECK(h >= 1 && h <= ANYV2V_RESAMPLE_MAX_SIDE && w >= 1 && w <= ANYV2V_RESAMPLE_MAX_SIDE, "detail_gate: h x w = %d x %d: both in [1, %d]", h, w,
             ANYV2V_RESAMPLE_MAX_SIDE);
    AV_CHECK(0 <= lo && lo < hi && hi <= 255, "detail_gate: lo = %d, hi = %d: 0 <= lo < hi <= 255", lo, hi);
    AV_CHECK(radius >= 0 && radius <= ANYV2V_DETAIL_MAX_RADIUS, "detail_gate: radius = %d must lie in [0, %d]", radius, ANYV2V_DETAIL_MAX_RADIUS);
    const long long pixels = (long long)F * h * w;
    AV_CHECK(scratch_bytes >= 2 * pixels, "detail_gate: scratch of %lld bytes, %lld needed", (long long)scratch_bytes, 2 * pixels);
    AV_CHECK((((uintptr_t)scratch) & 1) == 0, "detail_gate: the scratch must be 2-byte aligned");
    AV_CHECK(!detail_overlap(gate_out, pixels, edit, 3 * pixels) && !detail_overlap(gate_out, pixels, prepared, 3 * pixels) &&
                 !detail_overlap(gate_out, pixels, scratch, 2 * pixels),
             "detail_gate: gate_out may not overlap an input or the scratch");
    AV_CHECK(!detail_overlap(scratch, 2 * pixels, edit, 3 * pixels) && !detail_overlap(scratch, 2 * pixels, prepared, 3 * pixels),
             "detail_gate: the scratch may not overlap an input");
    const dim3 grid((unsigned)((w + RS_THREADS - 1) / RS_THREADS), (unsigned)h, (unsigned)F);
    hipLaunchKernelGGL(detail_rowsum_kernel, grid, dim3(RS_THREADS), 0, (hipStream_t)stream, (const uint8_t*)edit, (const uint8_t*)prepared,
                       (uint16_t*)scratch, w, radius);
    if (int rc = av_launch_status("detail_gate (row sums)")) return rc;
    hipLaunchKernelGGL(detail_gate_kernel, grid, dim3(RS_THREADS), 0, (hipStream_t)stream, (const uint16_t*)scratch, (uint8_t*)gate_out, h, w, lo,
                       hi, radius);
    return av_launch_status("detail_gate");
}

static int detail_table_ok(const char* which, int32_t rows, const int32_t* bounds, const int32_t* coeffs, int32_t ksize) {
    AV_CHECK(bounds && coeffs, "restore_detail: null %s table", which);
    AV_CHECK(rows >= 1 && rows <= ANYV2V_RESAMPLE_MAX_SIDE, "restore_detail: %s rows = %d must lie in [1, %d]", which, rows, ANYV2V_RESAMPLE_MAX_SIDE);
    AV_CHECK(ksize >= 1 && ksize <= 2 * ANYV2V_RESAMPLE_MAX_SIDE, "restore_detail: %s ksize = %d must lie in [1, %d]", which, ksize,
             2 * ANYV2V_RESAMPLE_MAX_SIDE);
    AV_CHECK((((uintptr_t)bounds) & 3) == 0 && (((uintptr_t)coeffs) & 3) == 0, "restore_detail: the %s tables must be 4-byte aligned", which);
    return ANYV2V_OK;
}

extern "C" int anyv2v_restore_detail_u8(const void* source, const void* edit_h, const void* prep_h, const void* gate_h, const void* alpha_h,
                                        void* out, int32_t F, int32_t sh, int32_t sw, int32_t dx0, int32_t dy0, int32_t dx1, int32_t dy1,
                                        int32_t e_rows, const int32_t* e_bounds, const int32_t* e_coeffs, int32_t e_ksize, int32_t gate_frames,
                                        int32_t mask_frames, int32_t a_rows, const int32_t* a_bounds, const int32_t* a_coeffs, int32_t a_ksize,
                                        void* stream) {
    AV_CHECK(source && edit_h && prep_h && gate_h && out, "restore_detail: null pointer");
    AV_CHECK(F >= 1 && F <= 65535, "restore_detail: F = %d must lie in [1, 65535]", F);
    AV_CHECK(sh >= 1 && sh <= ANYV2V_RESAMPLE_MAX_SIDE && sw >= 1 && sw <= ANYV2V_RESAMPLE_MAX_SIDE, "restore_detail: sh x sw = %d x %d: both in [1, %d]",
             sh, sw, ANYV2V_RESAMPLE_MAX_SIDE);
    AV_CHECK(0 <= dx0 && dx0 < dx1 && dx1 <= sw && 0 <= dy0 && dy0 < dy1 && dy1 <= sh,
             "restore_detail: dest (%d, %d, %d, %d) must be non-empty and lie inside the %d x %d frame", dx0, dy0, dx1, dy1, sw, sh);
    if (int rc = detail_table_ok("edit", e_rows, e_bounds, e_coeffs, e_ksize)) return rc;
    if (int rc = detail_table_ok("gate", a_rows, a_bounds, a_coeffs, a_ksize)) return rc;
    AV_CHECK(gate_frames == 1 || gate_frames == F, "restore_detail: gate_frames = %d must be 1 or F = %d", gate_frames, F);
    AV_CHECK(alpha_h == nullptr || mask_frames == 1 || mask_frames == F, "restore_detail: mask_frames = %d must be 1 or F = %d", mask_frames, F);
    const int dw = dx1 - dx0, dh = dy1 - dy0;
    const long long frame_bytes = (long long)F * sh * sw * 3, eh_bytes = (long long)F * e_rows * dw * 3;
    AV_CHECK(!detail_overlap(out, frame_bytes, source, frame_bytes), "restore_detail: out may not overlap the source");
    AV_CHECK(!detail_overlap(out, frame_bytes, edit_h, eh_bytes) && !detail_overlap(out, frame_bytes, prep_h, eh_bytes),
             "restore_detail: out may not overlap the edit's or the prepared source's intermediate");
    AV_CHECK(!detail_overlap(out, frame_bytes, gate_h, (long long)gate_frames * a_rows * dw), "restore_detail: out may not overlap the gate's intermediate");
    AV_CHECK(alpha_h == nullptr || !detail_overlap(out, frame_bytes, alpha_h, (long long)mask_frames * a_rows * dw),
             "restore_detail: out may not overlap alpha's intermediate");
    AV_CHECK(!detail_overlap(out, frame_bytes, e_bounds, (long long)dh * 8) && !detail_overlap(out, frame_bytes, e_coeffs, (long long)dh * e_ksize * 4) &&
                 !detail_overlap(out, frame_bytes, a_bounds, (long long)dh * 8) && !detail_overlap(out, frame_bytes, a_coeffs, (long long)dh * a_ksize * 4),
             "restore_detail: out may not overlap the tables");
    const int RB = 3 * sw, groups = (RB + 3) / 4;
    const dim3 grid((unsigned)((groups + RS_THREADS - 1) / RS_THREADS), (unsigned)sh, (unsigned)F);
    hipLaunchKernelGGL(restore_detail_kernel, grid, dim3(RS_THREADS), 0, (hipStream_t)stream, (const uint8_t*)source, (const uint8_t*)edit_h,
                       (const uint8_t*)prep_h, (const uint8_t*)gate_h, (const uint8_t*)alpha_h, (uint8_t*)out, sh, RB, dx0, dy0, dw, dh, e_rows,
                       e_bounds, e_coeffs, e_ksize, gate_frames == F && F > 1 ? 1 : 0, alpha_h != nullptr && mask_frames == F && F > 1 ? 1 : 0, a_rows,
                       a_bounds, a_coeffs, a_ksize, frame_bytes, eh_bytes);
    return av_launch_status("restore_detail");
}
