// Stitch of the tiled AutoencoderKL encode / decode (diffusers-0.26.3 AutoencoderKL.tiled_encode / tiled_decode / blend_v / blend_h, which
// the reference pipeline switches on with enable_vae_tiling, pipeline_i2vgen_xl.py:208-221): one launch gathers every output pixel of a
// batch of images from the RAW tiles the encoder / decoder wrote (channels-last token matrices [(image)(h w), ld], C <= 8 channels) and
// writes the planar [n_img, C, H, W] fp16 image that decode / encode_moments return.
//
// The definition blends in place, tile after tile in row-major order (first with the tile above, then with the tile on the left, each
// already blended), then keeps tile[:limit, :limit].  Unrolled, an output pixel that lies in tile (ky, kx) at (py, px) is
//     out = wy wx R[py, px] + wy (1 - wx) L[py, qx] + (1 - wy) wx^2 U[qy, px] + (1 - wy)(1 - wx^2) UL[qy, qx]
// with R / L / U / UL the raw tiles (ky, kx), (ky, kx - 1), (ky - 1, kx), (ky - 1, kx - 1); wy = py / e'_y inside the vertical blend
// band (qy = the row of the tile above it is blended with) and 1 outside, wx likewise.  The corner is NOT the separable bilinear
// weight: the tile above has itself been blended with ITS left neighbour before it is blended into this one (DESIGN.md "VAE tiling").
// The host (anyv2v_amd/vae_tiling.py) tabulates (k, p, q) and w per output row and per output column; the kernel searches nothing.
//
// Arithmetic: the four products and their sum in fp64, ONE rounding to fp16.  fp16 x (p / e') products are exact in fp64 and so is their
// sum whenever e' is a power of two, so the result is then the correctly rounded value of the definition -- bit-equal to the sequential
// algorithm evaluated exactly; fp32 cannot promise that (a 7-bit weight squared times an 11-bit value already has 32 bits), nor a bound
// relative to the RESULT when tiles of opposite sign cancel.  The kernel is bound by memory (one 16-byte load per term, C 2-byte stores);
// the fp64 work is 4 FMAs per channel.
// Mapping: one thread per output pixel, x fastest.  Lanes of a wave read consecutive 16-byte token rows of a tile row (1 KiB per
// instruction inside a tile; a wave that straddles a tile seam splits in two) and write 128 consecutive bytes of each channel plane.
#include "common.h"

#include <math.h>

#define TB_THREADS 256
#define TB_MAX_C 8

// double -> fp16 with a single rounding: round to odd into fp32 (24 bits >= 11 + 2), then the hardware's nearest-even fp32 -> fp16
__device__ __forceinline__ half_t tb_round_f16(double d) {
    float f = (float)d;
    if ((double)f != d && isfinite(f)) {   // inexact: the truncated neighbour with its last bit set
        uint32_t u = __float_as_uint(f);
        if (fabs((double)f) > fabs(d)) --u;   // sign-magnitude: one step towards zero (f is never +-0 here: d != f and f = 0 means |d| tiny, f < |d|)
        u |= 1u;
        f = __uint_as_float(u);
    }
    return (half_t)f;
}

__global__ __launch_bounds__(TB_THREADS) void tile_blend_kernel(const half_t* __restrict__ T, long long tile_rows, int ld, int C,
                                                                const int* __restrict__ tiles, int ntx, const int* __restrict__ ytab,
                                                                const double* __restrict__ ywt, const int* __restrict__ xtab,
                                                                const double* __restrict__ xwt, half_t* __restrict__ O, long long total,
                                                                int H, int W) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int x = (int)(i % W);
        const int y = (int)((i / W) % H);
        const long long n = i / ((long long)W * H);
        const int ky = ytab[3 * y], py = ytab[3 * y + 1], qy = ytab[3 * y + 2];
        const int kx = xtab[3 * x], px = xtab[3 * x + 1], qx = xtab[3 * x + 2];
        const double wy = ywt[y], wx = xwt[x];
        const bool by = wy < 1.0, bx = wx < 1.0;
        // tile record: {first row of image 0, height, width, 0}; image n of a tile follows image n - 1
        auto load = [&](int ty, int tx, int r, int c, h8& v) -> bool {
            const int* t = tiles + 4 * (ty * ntx + tx);
            const long long row = (long long)t[0] + (n * t[1] + r) * t[2] + c;
            if (row < 0 || row >= tile_rows) return false;   // (the entry point has checked the tables: never taken)
            v = *(const h8*)(T + row * ld);
            return true;
        };
        h8 r, l, u, ul;
        bool ok = load(ky, kx, py, px, r);
        if (bx) ok = load(ky, kx - 1, py, qx, l) && ok;
        if (by) ok = load(ky - 1, kx, qy, px, u) && ok;
        if (bx && by) ok = load(ky - 1, kx - 1, qy, qx, ul) && ok;
        if (!ok) continue;
        const double wr = wy * wx, wl = wy * (1.0 - wx), wu = (1.0 - wy) * (wx * wx), wul = (1.0 - wy) * (1.0 - wx * wx);
        half_t* dst = O + (n * C * H + y) * (long long)W + x;
#pragma unroll
        for (int c = 0; c < TB_MAX_C; ++c) {
            if (c >= C) break;
            double a = wr * (double)r[c];
            if (bx) a = fma(wl, (double)l[c], a);
            if (by) a = fma(wu, (double)u[c], a);
            if (bx && by) a = fma(wul, (double)ul[c], a);
            dst[(long long)c * H * W] = (bx || by) ? tb_round_f16(a) : r[c];
        }
    }
}

// One axis of the plan, on the host copy: every entry inside the tiles it names.  `ext(k, j)`: extent of tile k of this axis in the
// j-th tile of the other axis.
static bool tb_axis_ok(const int32_t* tab, const double* wt, int n, int nt, int nother, const int32_t* tiles, bool rows, int ntx) {
    for (int o = 0; o < n; ++o) {
        const int k = tab[3 * o], p = tab[3 * o + 1], q = tab[3 * o + 2];
        const double w = wt[o];
        if (k < 0 || k >= nt || !(w >= 0.0 && w <= 1.0)) return false;
        if (w < 1.0 && k < 1) return false;
        for (int j = 0; j < nother; ++j) {
            const int32_t* t = tiles + 4 * (rows ? k * ntx + j : j * ntx + k);
            if (p < 0 || p >= (rows ? t[1] : t[2])) return false;
            if (w < 1.0) {
                const int32_t* s = tiles + 4 * (rows ? (k - 1) * ntx + j : j * ntx + k - 1);
                if (q < 0 || q >= (rows ? s[1] : s[2])) return false;
            }
        }
    }
    return true;
}

extern "C" int anyv2v_tile_blend_f16(const void* tiles, int64_t tile_rows, int32_t ld, int32_t C, const int32_t* plan_host,
                                     const double* weight_host, const int32_t* plan_dev, const double* weight_dev, int32_t nty,
                                     int32_t ntx, void* out, int32_t n_img, int32_t H, int32_t W, void* stream) {
    AV_CHECK(tiles && out && plan_host && weight_host && plan_dev && weight_dev, "tile_blend: null pointer");
    AV_CHECK(n_img >= 1 && H >= 1 && W >= 1 && nty >= 1 && ntx >= 1 && nty <= H && ntx <= W,
             "tile_blend: n_img = %d, H = %d, W = %d, tile grid %d x %d", n_img, H, W, nty, ntx);
    AV_CHECK(C >= 1 && C <= TB_MAX_C && ld >= 8 && ld % 8 == 0 && av_aligned16(tiles),
             "tile_blend: C = %d must be 1..8 and the token rows 16-byte aligned (ld = %d, a multiple of 8)", C, ld);
    AV_CHECK((((uintptr_t)out) & 1) == 0 && (((uintptr_t)plan_dev) & 3) == 0 && (((uintptr_t)weight_dev) & 7) == 0,
             "tile_blend: misaligned output or table");
    AV_CHECK(tile_rows >= 1 && tile_rows < ((int64_t)1 << 31), "tile_blend: tile_rows = %lld outside [1, 2^31)", (long long)tile_rows);
    const int32_t* trec = plan_host;
    const int32_t* ytab = trec + 4 * (int64_t)nty * ntx;
    const int32_t* xtab = ytab + 3 * (int64_t)H;
    for (int t = 0; t < nty * ntx; ++t) {
        const int32_t* r = trec + 4 * t;
        AV_CHECK(r[0] >= 0 && r[1] >= 1 && r[2] >= 1 && (int64_t)r[0] + (int64_t)n_img * r[1] * r[2] <= tile_rows,
                 "tile_blend: tile %d (first row %d, %d x %d, %d images) leaves the %lld rows of the tile matrix", t, r[0], r[1], r[2],
                 n_img, (long long)tile_rows);
    }
    AV_CHECK(tb_axis_ok(ytab, weight_host, H, nty, ntx, trec, true, ntx), "tile_blend: a row-table entry leaves its tile");
    AV_CHECK(tb_axis_ok(xtab, weight_host + H, W, ntx, nty, trec, false, ntx), "tile_blend: a column-table entry leaves its tile");
    const long long total = (long long)n_img * H * W;
    long long blocks = (total + TB_THREADS - 1) / TB_THREADS;
    if (blocks > 8192) blocks = 8192;
    const int32_t* dtiles = plan_dev;
    const int32_t* dy = dtiles + 4 * (int64_t)nty * ntx;
    const int32_t* dx = dy + 3 * (int64_t)H;
    hipLaunchKernelGGL(tile_blend_kernel, dim3((unsigned)blocks), dim3(TB_THREADS), 0, (hipStream_t)stream, (const half_t*)tiles,
                       (long long)tile_rows, ld, C, dtiles, ntx, dy, weight_dev, dx, weight_dev + H, (half_t*)out, total, H, W);
    return av_launch_status("tile_blend");
}
