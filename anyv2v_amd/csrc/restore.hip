// The way back to the source clip's own size (include/anyv2v_hip.h holds the definition): per frame
//   out = S.copy();  out.paste(E.resize(dsize, filter, box), (dx0, dy0), mask = A.resize(dsize, BILINEAR, box))
// of Pillow.  The horizontal passes of E and A are anyv2v_resample_h_u8 (resample.hip); this kernel is the rest in one launch over the whole
// output frame: the vertical taps of E and of A (resample_v_kernel's arithmetic) and Pillow's 8-bit paste against the source byte
//   t = d * (255 - m) + e * m + 128;   out = ((t >> 8) + t) >> 8          (m = 0 gives d, m = 255 gives e: no select is needed)
// Bytes outside dest are copied from the source.  All integers: every result is the same whatever the thread order, and the kernel is
// tested bit for bit against Pillow.
//   restore_paste_kernel   block row = output row: the row's class (inside dest or not), (ymin, n) and the coefficients of both tables are
//                          uniform (scalar loads); a thread owns 4 bytes of the row -- at most two pixels, hence at most two alpha columns --
//                          and walks the input rows of the intermediates, each read a coalesced row segment
// Rows are 3 * sw bytes, usually no multiple of 4, dx0 lets the rectangle start at any byte, and the pointers carry no alignment: dwords are
// loaded as in resample.hip (rs_load4), bytes where a group straddles an edge of dest.  No atomics; every output byte is written once by
// one thread.
#include "resample_common.h"

// grid (ceil(ceil(RB / 4) / RS_THREADS), sh, F), RB = 3 * sw bytes per row of source and out, EB = 3 * dw bytes per row of eh
__global__ __launch_bounds__(RS_THREADS) void restore_paste_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ eh,
                                                                   const uint8_t* __restrict__ ah, uint8_t* __restrict__ out, int sh, int RB,
                                                                   int dx0, int dy0, int dw, int dh, int e_rows,
                                                                   const int* __restrict__ e_bounds, const int* __restrict__ e_coeffs,
                                                                   int e_ksize, int a_per_frame, int a_rows, const int* __restrict__ a_bounds,
                                                                   const int* __restrict__ a_coeffs, int a_ksize, long long src_bytes,
                                                                   long long eh_bytes) {
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
    const int e0 = b - 3 * dx0;   // the byte of eh's row under this thread's first byte
    if (r >= 0 && r < dh && e0 + nb > 0 && e0 < EB) {
        int y0 = e_bounds[2 * r], y1 = y0 + e_bounds[2 * r + 1];   // cut to the intermediate: no table can make a read leave eh
        y0 = min(max(y0, 0), e_rows);
        y1 = min(max(y1, y0), e_rows);
        const int skip = y0 - e_bounds[2 * r];
        const int n = min(y1 - y0, e_ksize - skip);
        const int* k = e_coeffs + (long long)r * e_ksize + skip;
        const uint8_t* p = eh + ((long long)f * e_rows + y0) * EB + e0;
        int acc[4] = {RS_HALF, RS_HALF, RS_HALF, RS_HALF};
        if (nb == 4 && e0 >= 0 && e0 + 4 <= EB) {
            for (int t = 0; t < n; ++t, p += EB) {
                const uint32_t v = rs_load4(p, eh, eh + eh_bytes);
                const int kt = k[t];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[j] = rs_mad(acc[j], (v >> (8 * j)) & 0xffu, kt);
            }
        } else {   // the group straddles an edge of dest (or the row's end): the bytes inside, one by one
            for (int t = 0; t < n; ++t, p += EB) {
                const int kt = k[t];
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j < nb && e0 + j >= 0 && e0 + j < EB) acc[j] = rs_mad(acc[j], p[j], kt);
            }
        }
        // alpha at the (at most two) pixels the group's bytes inside dest belong to
        const int c0 = max(e0, 0) / 3, c1 = min(e0 + 3, EB - 1) / 3;
        uint32_t m0 = 255u, m1 = 255u;
        if (ah != nullptr) {
            int ay0 = a_bounds[2 * r], ay1 = ay0 + a_bounds[2 * r + 1];
            ay0 = min(max(ay0, 0), a_rows);
            ay1 = min(max(ay1, ay0), a_rows);
            const int askip = ay0 - a_bounds[2 * r];
            const int an = min(ay1 - ay0, a_ksize - askip);
            const int* ak = a_coeffs + (long long)r * a_ksize + askip;
            const uint8_t* pa = ah + ((long long)(a_per_frame ? f : 0) * a_rows + ay0) * dw;
            int a0 = RS_HALF, a1 = RS_HALF;
            for (int t = 0; t < an; ++t, pa += dw) {
                const int kt = ak[t];
                a0 = rs_mad(a0, pa[c0], kt);
                a1 = rs_mad(a1, pa[c1], kt);
            }
            m0 = rs_finish(a0);
            m1 = rs_finish(a1);
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int pos = e0 + j;
            if (j < nb && pos >= 0 && pos < EB) {
                const uint32_t m = pos < 3 * (c0 + 1) ? m0 : m1;
                const uint32_t d = (s >> (8 * j)) & 0xffu, e = rs_finish(acc[j]);
                const uint32_t t = d * (255u - m) + e * m + 128u;
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

static bool restore_overlap(const void* a, long long na, const void* b, long long nb) {
    const uintptr_t pa = (uintptr_t)a, pb = (uintptr_t)b;
    return pa < pb + (uintptr_t)nb && pb < pa + (uintptr_t)na;
}

static int restore_table_ok(const char* which, int32_t rows, const int32_t* bounds, const int32_t* coeffs, int32_t ksize) {
    AV_CHECK(bounds && coeffs, "restore_paste: null %s table", which);
    AV_CHECK(rows >= 1 && rows <= ANYV2V_RESAMPLE_MAX_SIDE, "restore_paste: %s rows = %d must lie in [1, %d]", which, rows, ANYV2V_RESAMPLE_MAX_SIDE);
    AV_CHECK(ksize >= 1 && ksize <= 2 * ANYV2V_RESAMPLE_MAX_SIDE, "restore_paste: %s ksize = %d must lie in [1, %d]", which, ksize,
             2 * ANYV2V_RESAMPLE_MAX_SIDE);
    AV_CHECK((((uintptr_t)bounds) & 3) == 0 && (((uintptr_t)coeffs) & 3) == 0, "restore_paste: the %s tables must be 4-byte aligned", which);
    return ANYV2V_OK;
}

extern "C" int anyv2v_restore_paste_u8(const void* source, const void* edit_h, const void* alpha_h, void* out, int32_t F, int32_t sh, int32_t sw,
                                       int32_t dx0, int32_t dy0, int32_t dx1, int32_t dy1, int32_t e_rows, const int32_t* e_bounds,
                                       const int32_t* e_coeffs, int32_t e_ksize, int32_t mask_frames, int32_t a_rows, const int32_t* a_bounds,
                                       const int32_t* a_coeffs, int32_t a_ksize, void* stream) {
    AV_CHECK(source && edit_h && out, "restore_paste: null pointer");
    AV_CHECK(F >= 1 && F <= 65535, "restore_paste: F = %d must lie in [1, 65535]", F);
    AV_CHECK(sh >= 1 && sh <= ANYV2V_RESAMPLE_MAX_SIDE && sw >= 1 && sw <= ANYV2V_RESAMPLE_MAX_SIDE, "restore_paste: sh x sw = %d x %d: both in [1, %d]",
             sh, sw, ANYV2V_RESAMPLE_MAX_SIDE);
    AV_CHECK(0 <= dx0 && dx0 < dx1 && dx1 <= sw && 0 <= dy0 && dy0 < dy1 && dy1 <= sh,
             "restore_paste: dest (%d, %d, %d, %d) must be non-empty and lie inside the %d x %d frame", dx0, dy0, dx1, dy1, sw, sh);
    if (int rc = restore_table_ok("edit", e_rows, e_bounds, e_coeffs, e_ksize)) return rc;
    const int dw = dx1 - dx0, dh = dy1 - dy0;
    const long long frame_bytes = (long long)F * sh * sw * 3, eh_bytes = (long long)F * e_rows * dw * 3;
    AV_CHECK(!restore_overlap(out, frame_bytes, source, frame_bytes), "restore_paste: out may not overlap the source");
    AV_CHECK(!restore_overlap(out, frame_bytes, edit_h, eh_bytes), "restore_paste: out may not overlap the edit's intermediate");
    AV_CHECK(!restore_overlap(out, frame_bytes, e_bounds, (long long)dh * 8) && !restore_overlap(out, frame_bytes, e_coeffs, (long long)dh * e_ksize * 4),
             "restore_paste: out may not overlap the edit tables");
    if (alpha_h != nullptr) {
        AV_CHECK(mask_frames == 1 || mask_frames == F, "restore_paste: mask_frames = %d must be 1 or F = %d", mask_frames, F);
        if (int rc = restore_table_ok("alpha", a_rows, a_bounds, a_coeffs, a_ksize)) return rc;
        AV_CHECK(!restore_overlap(out, frame_bytes, alpha_h, (long long)mask_frames * a_rows * dw), "restore_paste: out may not overlap alpha's intermediate");
        AV_CHECK(!restore_overlap(out, frame_bytes, a_bounds, (long long)dh * 8) && !restore_overlap(out, frame_bytes, a_coeffs, (long long)dh * a_ksize * 4),
                 "restore_paste: out may not overlap the alpha tables");
    }
    const int RB = 3 * sw, groups = (RB + 3) / 4;
    const dim3 grid((unsigned)((groups + RS_THREADS - 1) / RS_THREADS), (unsigned)sh, (unsigned)F);
    hipLaunchKernelGGL(restore_paste_kernel, grid, dim3(RS_THREADS), 0, (hipStream_t)stream, (const uint8_t*)source, (const uint8_t*)edit_h,
                       (const uint8_t*)alpha_h, (uint8_t*)out, sh, RB, dx0, dy0, dw, dh, e_rows, e_bounds, e_coeffs, e_ksize,
                       mask_frames == F && F > 1 ? 1 : 0, a_rows, a_bounds, a_coeffs, a_ksize, frame_bytes, eh_bytes);
    return av_launch_status("restore_paste");
}
