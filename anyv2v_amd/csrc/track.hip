// Carry a first-frame edit mask through the clip along block-matched motion of the SOURCE frames (classical full-search block matching on
// the latent grid's 8 x 8 cells; nothing in the reference does this; include/anyv2v_hip.h holds the definition).  All integers: every
// result is the same whatever the thread order, so every kernel is tested bit for bit.
//   luma_kernel              Y = (77 R + 150 G + 29 B + 128) >> 8, four pixels per thread where the pointers allow
//   block_match_kernel       per frame k >= 1 and cell: the displacement in [-R, R]^2 that minimises (SAD, dy^2 + dx^2, dy, dx) of the cell's
//                            16 x 16 window of Y_k against Y_{k-1}; a block owns 4 x 4 cells, 16 lanes share a cell's candidates
//   flow_median_kernel       3 x 3 median of each component over the cells, replicate border
//   mask_propagate_kernel    one thread per output pixel: q <- clamp(q + D_j[cell(q)]) for j = k .. 1, then mask_0[q]
//   first_frame_mask_kernel  one wave per cell: a lane per pixel, the count by ballot
// No atomics, no floating point; every output element is written exactly once by one thread.
#include "common.h"

#define TR_THREADS 256
#define TR_MAX_R ANYV2V_TRACK_MAX_RADIUS
#define TR_TILE 4                              // cells per block edge
#define TR_LANES 16                            // lanes that share one cell's candidates (TR_TILE^2 * TR_LANES == TR_THREADS)
#define TR_CUR (8 * TR_TILE + 8)               // the tile's Y_k region: its cells and the 4-pixel window margin, 40 x 40
#define TR_MAX_GROUPS (TR_MAX_R / 2 + 1)       // groups of four dx: ceil((2 R + 1) / 4)
#define TR_PREV_W (TR_CUR + 4 * TR_MAX_GROUPS) // widest Y_{k-1} row (R = 32): 108 bytes
#define TR_PREV_H (TR_CUR + 2 * TR_MAX_R)      // 104 rows

static_assert(TR_TILE * TR_TILE * TR_LANES == TR_THREADS, "16 lanes per cell, 16 cells per block");

__device__ __forceinline__ int clampi(int v, int hi) { return min(max(v, 0), hi); }

__device__ __forceinline__ uint32_t luma_of(uint32_t r, uint32_t g, uint32_t b) { return (77u * r + 150u * g + 29u * b + 128u) >> 8; }

// VEC: 4 pixels per thread -- 12 bytes in as three dwords, one dword out (n % 4 == 0, both pointers 4-byte aligned)
template <bool VEC>
__global__ __launch_bounds__(TR_THREADS) void luma_kernel(const uint8_t* __restrict__ rgb, uint8_t* __restrict__ y, long long n) {
    const long long p = ((long long)blockIdx.x * TR_THREADS + threadIdx.x) * (VEC ? 4 : 1);
    if (p >= n) return;
    if (VEC) {
        const uint32_t* s = (const uint32_t*)(rgb + 3 * p);
        const uint32_t w[3] = {s[0], s[1], s[2]};
        uint32_t o = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            uint32_t c[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int byte = 3 * k + j;
                c[j] = (w[byte >> 2] >> (8 * (byte & 3))) & 0xffu;
            }
            o |= luma_of(c[0], c[1], c[2]) << (8 * k);
        }
        *(uint32_t*)(y + p) = o;
    } else {
        y[p] = (uint8_t)luma_of(rgb[3 * p], rgb[3 * p + 1], rgb[3 * p + 2]);
    }
}

// The winner of a cell is the smallest key: cost (<= 65 280, 16 bits) | dy^2 + dx^2 (<= 2048, 12 bits) | dy + 32 (7 bits) | dx + 32 (7 bits)
// -- an unsigned comparison of the keys IS the lexicographic comparison of (cost, dy^2 + dx^2, dy, dx), and a minimum does not depend on
// the order its operands arrive in.
__device__ __forceinline__ unsigned long long match_key(uint32_t cost, int dy, int dx) {
    return ((unsigned long long)cost << 26) | ((unsigned long long)(dy * dy + dx * dx) << 14) | ((unsigned long long)(dy + 32) << 7)
           | (unsigned long long)(dx + 32);
}

// Block (tx, ty, k): the 4 x 4 cells at (4 ty, 4 tx) of frame k.  LDS holds, already clamped (replicate border), the Y_k bytes of the
// tile's windows (origin 4 pixels up and left of the tile) and the Y_{k-1} bytes every candidate of every window can touch (origin R + 4
// up and left).  With that origin the window of local cell column c displaced by dx = j - R starts at byte 8 c + j of a row: for j = 4 g
// it is dword-aligned, and the windows of j = 4 g + 1 .. 4 g + 3 are the same five dwords shifted by one to three bytes -- for EVERY dx,
// whatever its sign or parity.  A task is (dy, g): 16 rows x (5 dword reads, 12 byte-aligns, 16 v_sad_u8) give the costs of four
// candidates; the window of Y_k stays in 64 registers.  The 16 lanes of a cell stride over its tasks and fold their keys by shuffles.
__global__ __launch_bounds__(TR_THREADS) void block_match_kernel(const uint8_t* __restrict__ luma, int16_t* __restrict__ flow, int H, int W,
                                                                 int R) {
    __shared__ uint32_t cur_s[TR_CUR * TR_CUR / 4];
    __shared__ uint32_t prev_s[TR_PREV_H * TR_PREV_W / 4];
    const int h = H >> 3, w = W >> 3, k = blockIdx.z;
    const int cell = threadIdx.x / TR_LANES, sub = threadIdx.x % TR_LANES;
    const int cyl = cell / TR_TILE, cxl = cell % TR_TILE;
    const int cy = blockIdx.y * TR_TILE + cyl, cx = blockIdx.x * TR_TILE + cxl;
    const bool live = cy < h && cx < w;
    uint32_t* dst = (uint32_t*)(flow + (((long long)k * h + cy) * w + cx) * 2);
    if (k == 0 || R == 0) {   // D_0 = 0; a radius of 0 has one candidate
        if (live && sub == 0) *dst = 0u;
        return;
    }
    const int groups = R / 2 + 1, pw = TR_CUR + 4 * groups, ph = TR_CUR + 2 * R;   // pw % 4 == 0
    const uint8_t* yk = luma + (long long)k * H * W;
    const uint8_t* yp = yk - (long long)H * W;
    const int y0 = blockIdx.y * (8 * TR_TILE) - 4, x0 = blockIdx.x * (8 * TR_TILE) - 4;
    uint8_t* cur_b = (uint8_t*)cur_s;
    uint8_t* prev_b = (uint8_t*)prev_s;
    for (int i = threadIdx.x; i < TR_CUR * TR_CUR; i += TR_THREADS) {
        const int r = i / TR_CUR, c = i - r * TR_CUR;
        cur_b[i] = yk[(long long)clampi(y0 + r, H - 1) * W + clampi(x0 + c, W - 1)];
    }
    for (int i = threadIdx.x; i < ph * pw; i += TR_THREADS) {   // (columns beyond 39 + 2 R are read by masked candidates only)
        const int r = i / pw, c = i - r * pw;
        prev_b[i] = yp[(long long)clampi(y0 - R + r, H - 1) * W + clampi(x0 - R + c, W - 1)];
    }
    __syncthreads();
    uint32_t cw[16][4];   // this cell's window of Y_k
#pragma unroll
    for (int r = 0; r < 16; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) cw[r][i] = cur_s[((8 * cyl + r) * TR_CUR + 8 * cxl) / 4 + i];
    unsigned long long best = ~0ull;
    const int tasks = (2 * R + 1) * groups, pw4 = pw / 4;
    for (int t = sub; t < tasks; t += TR_LANES) {
        const int jy = t / groups, g = t - jy * groups;
        const uint32_t* row = prev_s + (8 * cyl + jy) * pw4 + 2 * cxl + g;
        uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            uint32_t q[5];
#pragma unroll
            for (int i = 0; i < 5; ++i) q[i] = row[r * pw4 + i];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                c0 = __builtin_amdgcn_sad_u8(cw[r][i], q[i], c0);
                c1 = __builtin_amdgcn_sad_u8(cw[r][i], __builtin_amdgcn_alignbyte(q[i + 1], q[i], 1), c1);
                c2 = __builtin_amdgcn_sad_u8(cw[r][i], __builtin_amdgcn_alignbyte(q[i + 1], q[i], 2), c2);
                c3 = __builtin_amdgcn_sad_u8(cw[r][i], __builtin_amdgcn_alignbyte(q[i + 1], q[i], 3), c3);
            }
        }
        const int dy = jy - R, dx = 4 * g - R;
        const uint32_t cost[4] = {c0, c1, c2, c3};
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const unsigned long long key = match_key(cost[s], dy, dx + s);
            if (dx + s <= R && key < best) best = key;
        }
    }
#pragma unroll
    for (int o = TR_LANES / 2; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o, 64);
        best = other < best ? other : best;
    }
    if (live && sub == 0) {
        const int dy = (int)((best >> 7) & 127) - 32, dx = (int)(best & 127) - 32;
        *dst = ((uint32_t)dy & 0xffffu) | ((uint32_t)dx << 16);   // (dy, dx) as two int16, one dword store
    }
}

__device__ __forceinline__ void order2(int& a, int& b) {
    const int lo = min(a, b), hi = max(a, b);
    a = lo;
    b = hi;
}

// median of nine by the 19-exchange network (Paeth, Graphics Gems)
__device__ __forceinline__ int median9(int p[9]) {
    order2(p[1], p[2]); order2(p[4], p[5]); order2(p[7], p[8]);
    order2(p[0], p[1]); order2(p[3], p[4]); order2(p[6], p[7]);
    order2(p[1], p[2]); order2(p[4], p[5]); order2(p[7], p[8]);
    order2(p[0], p[3]); order2(p[5], p[8]); order2(p[4], p[7]);
    order2(p[3], p[6]); order2(p[1], p[4]); order2(p[2], p[5]);
    order2(p[4], p[7]); order2(p[4], p[2]); order2(p[6], p[4]);
    order2(p[4], p[2]);
    return p[4];
}

__global__ __launch_bounds__(TR_THREADS) void flow_median_kernel(const int16_t* __restrict__ in, int16_t* __restrict__ out, int n, int h, int w) {
    const int i = blockIdx.x * TR_THREADS + threadIdx.x;   // over [F, h, w, 2]
    if (i >= n) return;
    const int c = i & 1, cx = (i >> 1) % w, cy = (i >> 1) / w % h, f = (i >> 1) / (w * h);
    const int16_t* plane = in + (long long)f * h * w * 2 + c;
    int p[9];
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) p[3 * a + b] = plane[(clampi(cy + a - 1, h - 1) * w + clampi(cx + b - 1, w - 1)) * 2];
    out[i] = (int16_t)median9(p);
}

__global__ __launch_bounds__(TR_THREADS) void mask_propagate_kernel(const uint8_t* __restrict__ mask0, const int16_t* __restrict__ flow,
                                                                    uint8_t* __restrict__ out, int n, int H, int W) {
    const int i = blockIdx.x * TR_THREADS + threadIdx.x;   // over [F, H, W]
    if (i >= n) return;
    const int w = W >> 3, h = H >> 3;
    int x = i % W, y = i / W % H;
    for (int j = i / (W * H); j >= 1; --j) {
        const int16_t* d = flow + (((long long)j * h + (y >> 3)) * w + (x >> 3)) * 2;
        y = clampi(y + d[0], H - 1);
        x = clampi(x + d[1], W - 1);
    }
    out[i] = mask0[y * W + x] != 0 ? 1 : 0;
}

// wave = cell, lane = pixel of the cell (row lane / 8, column lane % 8); whole waves leave together, so the ballot sees 64 lanes
__global__ __launch_bounds__(TR_THREADS) void first_frame_mask_kernel(const uint8_t* __restrict__ src, const uint8_t* __restrict__ edit,
                                                                      uint8_t* __restrict__ mask, int cells, int W, int threshold, int min_count) {
    const int cell = blockIdx.x * (TR_THREADS / WAVE) + threadIdx.x / WAVE, lane = threadIdx.x % WAVE;
    if (cell >= cells) return;
    const int w = W >> 3;
    const int p = ((cell / w) * 8 + lane / 8) * W + (cell % w) * 8 + lane % 8;
    int d = 0;
#pragma unroll
    for (int c = 0; c < 3; ++c) d = max(d, abs((int)edit[3 * p + c] - (int)src[3 * p + c]));
    const int count = __popcll(__ballot(d > threshold));
    mask[p] = count >= min_count ? 1 : 0;
}

static int track_shape_ok(const char* what, int32_t F, int32_t H, int32_t W) {
    AV_CHECK(F >= 1, "%s: F = %d must be at least 1", what, F);
    AV_CHECK(H >= 8 && W >= 8 && H % 8 == 0 && W % 8 == 0, "%s: H x W = %d x %d must be positive multiples of 8", what, H, W);
    AV_CHECK(3ll * F * H * W < (1ll << 31), "%s: 3 * F * H * W must fit an int", what);
    return ANYV2V_OK;
}

extern "C" int anyv2v_luma_u8(const void* frames, void* luma, int32_t F, int32_t H, int32_t W, void* stream) {
    AV_CHECK(frames && luma, "luma: null pointer");
    if (int rc = track_shape_ok("luma", F, H, W)) return rc;
    const long long n = (long long)F * H * W;   // a multiple of 64
    const bool vec = (((uintptr_t)frames) & 3) == 0 && (((uintptr_t)luma) & 3) == 0;
    const long long threads = vec ? n / 4 : n;
    const dim3 grid((unsigned)((threads + TR_THREADS - 1) / TR_THREADS)), block(TR_THREADS);
    if (vec)
        hipLaunchKernelGGL(luma_kernel<true>, grid, block, 0, (hipStream_t)stream, (const uint8_t*)frames, (uint8_t*)luma, n);
    else
        hipLaunchKernelGGL(luma_kernel<false>, grid, block, 0, (hipStream_t)stream, (const uint8_t*)frames, (uint8_t*)luma, n);
    return av_launch_status("luma");
}

extern "C" int anyv2v_block_match_u8(const void* luma, void* flow, int32_t F, int32_t H, int32_t W, int32_t radius, void* stream) {
    AV_CHECK(luma && flow, "block_match: null pointer");
    if (int rc = track_shape_ok("block_match", F, H, W)) return rc;
    AV_CHECK(radius >= 0 && radius <= TR_MAX_R, "block_match: radius = %d must lie in [0, %d]", radius, TR_MAX_R);
    AV_CHECK((((uintptr_t)flow) & 3) == 0, "block_match: flow must be 4-byte aligned");
    AV_CHECK(F <= 65535, "block_match: F = %d must be at most 65535", F);
    const int h = H / 8, w = W / 8;
    const dim3 grid((unsigned)((w + TR_TILE - 1) / TR_TILE), (unsigned)((h + TR_TILE - 1) / TR_TILE), (unsigned)F);
    hipLaunchKernelGGL(block_match_kernel, grid, dim3(TR_THREADS), 0, (hipStream_t)stream, (const uint8_t*)luma, (int16_t*)flow, H, W, radius);
    return av_launch_status("block_match");
}

extern "C" int anyv2v_flow_median_i16(const void* flow, void* out, int32_t F, int32_t h, int32_t w, void* stream) {
    AV_CHECK(flow && out, "flow_median: null pointer");
    AV_CHECK(F >= 1, "flow_median: F = %d must be at least 1", F);
    AV_CHECK(h >= 1 && w >= 1, "flow_median: h x w = %d x %d cells: both at least 1", h, w);
    AV_CHECK(2ll * F * h * w < (1ll << 31), "flow_median: 2 * F * h * w must fit an int");
    AV_CHECK(flow != out, "flow_median: out may not alias the input");
    const int n = 2 * F * h * w;
    hipLaunchKernelGGL(flow_median_kernel, dim3((unsigned)((n + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0, (hipStream_t)stream,
                       (const int16_t*)flow, (int16_t*)out, n, h, w);
    return av_launch_status("flow_median");
}

extern "C" int anyv2v_mask_propagate_u8(const void* mask0, const void* flow, void* out, int32_t F, int32_t H, int32_t W, void* stream) {
    AV_CHECK(mask0 && flow && out, "mask_propagate: null pointer");
    if (int rc = track_shape_ok("mask_propagate", F, H, W)) return rc;
    AV_CHECK(out != mask0 && out != flow, "mask_propagate: out may not alias an input");
    const int n = F * H * W;
    hipLaunchKernelGGL(mask_propagate_kernel, dim3((unsigned)((n + TR_THREADS - 1) / TR_THREADS)), dim3(TR_THREADS), 0, (hipStream_t)stream,
                       (const uint8_t*)mask0, (const int16_t*)flow, (uint8_t*)out, n, H, W);
    return av_launch_status("mask_propagate");
}

extern "C" int anyv2v_first_frame_mask_u8(const void* source, const void* edited, void* mask, int32_t H, int32_t W, int32_t threshold,
                                          int32_t min_count, void* stream) {
    AV_CHECK(source && edited && mask, "first_frame_mask: null pointer");
    if (int rc = track_shape_ok("first_frame_mask", 1, H, W)) return rc;
    AV_CHECK(threshold >= 0 && threshold <= 255, "first_frame_mask: threshold = %d must lie in [0, 255]", threshold);
    AV_CHECK(min_count >= 1 && min_count <= 64, "first_frame_mask: min_count = %d must lie in [1, 64]", min_count);
    AV_CHECK(mask != source && mask != edited, "first_frame_mask: mask may not alias an input");
    const int cells = (H / 8) * (W / 8), per = TR_THREADS / WAVE;
    hipLaunchKernelGGL(first_frame_mask_kernel, dim3((unsigned)((cells + per - 1) / per)), dim3(TR_THREADS), 0, (hipStream_t)stream,
                       (const uint8_t*)source, (const uint8_t*)edited, (uint8_t*)mask, cells, W, threshold, min_count);
    return av_launch_status("first_frame_mask");
}
