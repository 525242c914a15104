// Definitions shared by the GEMM translation units (gemm.hip = host entry; gemm_mfma / gemm_big / gemm_pp / gemm_ref / gemm_ws /
// gemm_sw / gemm_swh .hip = one kernel family each; ff_fused.hip): kernel argument block, gather addressing, the inline-asm
// fragment reads with their counted waits, and the family launchers.
#pragma once
#include "common.h"
#include "gemm_plan.h"   // MODE_*, ACT_*, GemmPlan

struct GemmK {
    const half_t* A0;
    const half_t* A1;
    const half_t* W;
    half_t* C;
    const half_t* bias;
    const half_t* rowvec;
    const half_t* R;
    const half_t* zeros;
    int M, N, C0, C1, lda0, lda1, ldc, ldr, ldrv, rowvec_div;
    int mode, Hi, Wi, Ho, Wo, stride, up, F, HW, act;
    int pad_lo;  // conv2d: zero rows / columns before the first pixel (1 = "same" 3x3; 0 = pad only right / bottom)
    int taps, Ktot, nt0, nt1, tilesN;
    int vec_epi;  // bias / rowvec may be read as 8-byte vectors
    int splits;   // split-K factor (128-row kernel only): each split writes an fp32 partial tile, reduced afterwards
    float* partial;  // [splits][M][N] fp32 workspace
    long long* trace;  // debug (ANYV2V_GEMM_PROBE_TRACE): 32 timestamps per block, see tools/gemm_trace.py
    const float* ln_c1;  // LayerNorm fold (gemm_ws.hip): column sums of the gamma-scaled weights, or nullptr
    float ln_eps;
    // persistent kernel, rastered tile order (0 = classic): an XCD round covers rast_gm x rast_gn output tiles; rast_sm x rast_sn
    // super-tiles, walked M-fastest (rast_nfast = 0) or N-fastest
    int rast_gm, rast_gn, rast_sm, rast_sn, rast_nfast;
    // GroupNorm records from the epilogue (GN instantiations only): [M / 16][gn_groups][3] floats, gn_cg = N / gn_groups
    float* gn_stats;
    int gn_groups, gn_cg;
};

struct RowInfo {
    int base;  // linear/temporal: row m (or -1); conv2d: img * Hi * Wi
    int y, x;  // conv2d: yo*stride-1, xo*stride-1 ; temporal: y = frame index
};

template <int MODE>
__device__ __forceinline__ RowInfo make_row(const GemmK& p, int m) {
    RowInfo r;
    const bool ok = m < p.M;
    if constexpr (MODE == MODE_CONV2D) {
        const int hw = p.Ho * p.Wo;
        const int img = m / hw, rem = m - img * hw;
        const int yo = rem / p.Wo, xo = rem - yo * p.Wo;
        r.base = img * p.Hi * p.Wi;
        r.y = ok ? yo * p.stride - p.pad_lo : -(1 << 28);
        r.x = xo * p.stride - p.pad_lo;
    } else if constexpr (MODE == MODE_TEMPORAL) {
        r.base = m;
        r.y = ok ? (m / p.HW) % p.F : -(1 << 28);
        r.x = 0;
    } else {
        r.base = ok ? m : -1;
        r.y = r.x = 0;
    }
    return r;
}

// source row of output row `r` for filter tap `tap`, or -1 when the tap falls into the zero padding (branch-free)
template <int MODE>
__device__ __forceinline__ int src_row(const GemmK& p, const RowInfo& r, int tap) {
    if constexpr (MODE == MODE_CONV2D) {
        const int dy = tap / 3, dx = tap - dy * 3;
        int yi = r.y + dy, xi = r.x + dx;
        const int ly = p.Hi << p.up, lx = p.Wi << p.up;
        const bool ok = (yi >= 0) & (yi < ly) & (xi >= 0) & (xi < lx);
        yi >>= p.up;
        xi >>= p.up;
        return ok ? r.base + yi * p.Wi + xi : -1;
    } else if constexpr (MODE == MODE_TEMPORAL) {
        const int f = r.y + tap - 1;
        const bool ok = (f >= 0) & (f < p.F);
        return ok ? r.base + (tap - 1) * p.HW : -1;
    } else {
        return r.base;
    }
}

// per-K-tile A source: wave-uniform (base pointer, leading dim, column offset) + per-row select against the zero line
struct ASrc {
    const half_t* base;
    int ld;
};
__device__ __forceinline__ ASrc a_source(const GemmK& p, int kt_c, int kc) {
    ASrc s;
    const bool first = kt_c < p.nt0;
    s.base = (first ? p.A0 + kt_c * 64 : p.A1 + (kt_c - p.nt0) * 64) + kc * 8;
    s.ld = first ? p.lda0 : p.lda1;
    return s;
}
__device__ __forceinline__ const half_t* a_addr(const GemmK& p, const ASrc& s, int sr) {
    const half_t* g = s.base + (long long)sr * s.ld;
    return sr < 0 ? p.zeros : g;
}

// Incremental gather addressing of the ROWS A rows a thread stages per K-tile: inside one (tap, source) run consecutive K-tiles only
// advance the channel offset (+128 bytes); the row -> shifted-row math is redone only when the tap or the source changes
// (wave-uniform branch).
// ORD (conv2d): 0 = tap-major K order (tap, channel slice); 1 = slice-major (channel slice, dy, dx): the three dx taps of one
// (slice, dy) are consecutive K-tiles and touch the same A lines shifted by one pixel -- L1 (TCP) hits when nothing else allocates
// there in between (the W pieces then go past L1, `sc1`; probe builds of gemm_sw.hip only)
template <int MODE, int ROWS, int ORD = 0>
struct AGen {
    const half_t* ap[ROWS];
    int astep[ROWS];  // halves to advance per K-tile: 64, or 0 for rows that read the zero line
    int ktc, tap;
    __device__ __forceinline__ void recompute(const GemmK& p, const RowInfo (&ri)[ROWS], int kc) {
        const ASrc s = a_source(p, ktc, kc);
#pragma unroll
        for (int i = 0; i < ROWS; ++i) {
            const int sr = src_row<MODE>(p, ri[i], tap);
            ap[i] = a_addr(p, s, sr);
            astep[i] = sr < 0 ? 0 : 64;
        }
    }
    __device__ __forceinline__ void start(const GemmK& p, const RowInfo (&ri)[ROWS], int kc, int kt0 = 0, int ntap = 1) {
        tap = kt0 / ntap;          // (tap-major order; ORD 1 launches always start at K-tile 0)
        ktc = kt0 - tap * ntap;
        recompute(p, ri, kc);
    }
    __device__ __forceinline__ void next(const GemmK& p, const RowInfo (&ri)[ROWS], int kc, int ntap) {
        if constexpr (ORD == 1) {
            if (++tap == p.taps) {
                tap = 0;
                ++ktc;
            }
            recompute(p, ri, kc);
            return;
        }
        if (++ktc == ntap) {
            ktc = 0;
            ++tap;
        }
        if (ktc == 0 || ktc == p.nt0) {
            recompute(p, ri, kc);
        } else {
#pragma unroll
            for (int i = 0; i < ROWS; ++i) ap[i] += astep[i];
        }
    }
    // The same step in two parts (ORD 0; the one-wave kernel of gemm_sw.hip only): `bump` = the pointer adds, UNCONDITIONAL, issued
    // inside the K-tile body as fillers between MFMAs; `count` = the counters and -- when the tap or the source changes -- the
    // recomputation that overwrites the bumped pointers, between two bodies.  With one wave per SIMD every VALU instruction between
    // two bodies is matrix-pipe idle time.
    __device__ __forceinline__ void bump() {
#pragma unroll
        for (int i = 0; i < ROWS; ++i) ap[i] += astep[i];
    }
    __device__ __forceinline__ void count(const GemmK& p, const RowInfo (&ri)[ROWS], int kc, int ntap) {
        if (++ktc == ntap) {
            ktc = 0;
            ++tap;
        }
        if (ktc == 0 || ktc == p.nt0) recompute(p, ri, kc);
    }
};

__device__ __forceinline__ void glds16(const half_t* g, char* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)g,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

// The fragment reads below are inline asm with hand-counted waits; what that relies on is checked over the generated assembly by
// tests/test_isa_guards.py (no scratch access / copy of a pending destination, every MFMA covered by its counted wait).  Validated
// with ROCm 7.2's hipcc only: a different compiler may schedule around the asm differently -- rerun that test and `-m gpu`.
#if defined(HIP_VERSION_MAJOR) && (HIP_VERSION_MAJOR != 7 || HIP_VERSION_MINOR != 2)
#warning "GEMM kernels: inline-asm LDS fragment reads were validated with ROCm 7.2 only; rerun tests/test_isa_guards.py and the -m gpu suite"
#endif
// Fragment reads of a K-tile are issued as inline asm with hand-counted `s_waitcnt lgkmcnt(n)`: with an LDS-DMA load
// (global_load_lds) in flight hipcc treats the LGKM counter as out of order and waits lgkmcnt(0) before every fragment use,
// i.e. also for the fragment it has just requested two groups ahead -- the roll degenerates into issue -> full LDS latency ->
// use (tools/wait_probe.hip reproduces it in 30 lines).  LDS reads return in order among themselves, and the DMA completes on
// vmcnt, so the wait a use needs is "all but the reads issued after mine".
__device__ __forceinline__ h8 lds_frag(unsigned base, int off) {  // off: a constant after unrolling (16-bit immediate)
    h8 v;
    asm volatile("ds_read_b128 %0, %1 offset:%2" : "=v"(v) : "v"(base), "n"(off) : "memory");
    return v;
}
__device__ __forceinline__ h8 lds_frag(unsigned addr) {
    h8 v;
    asm volatile("ds_read_b128 %0, %1" : "=v"(v) : "v"(addr) : "memory");
    return v;
}
__device__ __forceinline__ void lgkm_wait(int n) {  // n is a constant after unrolling; the switch folds to one s_waitcnt
    switch (n) {
#define AV_LGW(k) case k: asm volatile("s_waitcnt lgkmcnt(" #k ")" ::: "memory"); break;
        AV_LGW(0) AV_LGW(1) AV_LGW(2) AV_LGW(3) AV_LGW(4) AV_LGW(5) AV_LGW(6) AV_LGW(7) AV_LGW(8) AV_LGW(9) AV_LGW(10)
        AV_LGW(11) AV_LGW(12) AV_LGW(13) AV_LGW(14) AV_LGW(15)
#undef AV_LGW
        default: asm volatile("s_waitcnt lgkmcnt(15)" ::: "memory"); break;  // (more than 15 younger reads: the counter saturates there)
    }
}

// ---- the arithmetic of the weight-stationary kernels' K-step and LayerNorm fold, shared by gemm_ws.hip and tattn_fused.hip: both
// kernels call these, so a row's projection has the same bits whichever of them computes it (same MFMA shape, same K order, same
// statistics, same fold).  D = W x^T: lane (token l & 15, l >> 4) holds output channels 4 (l >> 4) .. + 3 of a 16-channel fragment.
// one weight fragment against the two 16-token halves of a strip
__device__ __forceinline__ void ws_mfma_pair(const h8& wfr, const h8& x0, const h8& x1, f4& acc0, f4& acc1) {
    acc0 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wfr, x0, acc0, 0, 0, 0);
    acc1 = __builtin_amdgcn_mfma_f32_16x16x32_f16(wfr, x1, acc1, 0, 0, 0);
}
// row statistics of one K-step out of the matrix pipe: the activation fragment with itself (Gram matrix: its diagonal is sum x^2)
// and with a fragment of ones (sum x)
__device__ __forceinline__ void ws_ln_stats_step(const h8& x, const h8& ones, f4& accq, f4& accs) {
    accq = __builtin_amdgcn_mfma_f32_16x16x32_f16(x, x, accq, 0, 0, 0);
    accs = __builtin_amdgcn_mfma_f32_16x16x32_f16(ones, x, accs, 0, 0, 0);
}
// mean / rstd of token l15 over K channels from the two statistics accumulators.  D[i][j] of the Gram MFMA sits in lane (j = l15,
// lq = i >> 2), register i & 3: token j's own sum x^2 is register l15 & 3 of the lane with lq == l15 >> 2 -- select, then fetch it
// from that lane; sum x is in every register
template <int K>
__device__ __forceinline__ void ws_ln_row_stats(const f4& accq, const f4& accs, int l15, float eps, float& mean_out, float& rstd_out) {
    const int r3 = l15 & 3;
    float d = r3 == 0 ? accq[0] : (r3 == 1 ? accq[1] : (r3 == 2 ? accq[2] : accq[3]));
    d = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(((l15 >> 2) * 16 + l15) * 4, __builtin_bit_cast(int, d)));
    const float mean = accs[0] * (1.0f / K);
    const float var = fmaxf(d * (1.0f / K) - mean * mean, 0.0f);
    mean_out = mean;
    rstd_out = __builtin_amdgcn_rsqf(var + eps);
}
// LN(x) W^T + b = rstd (x W'^T - mean c1) + b' on one accumulator fragment
__device__ __forceinline__ void ws_ln_fold(f4& acc, const f4& c1, const h4& b, float mean, float rstd) {
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[r] = fmaf(fmaf(-mean, c1[r], acc[r]), rstd, (float)b[r]);
}

// accumulator element -> VGPR, AT the use (one-wave kernels, accumulators in AGPRs): left to hipcc, the AGPR -> VGPR copies of all 240
// accumulators are hoisted to the top of the epilogue (they are copies of phi values), which overflows the 256 arch VGPRs into AGPRs
// and the accumulators into scratch
__device__ __forceinline__ float acc_read(const float& a) {
    float v;
    asm volatile("v_accvgpr_read_b32 %0, %1" : "=v"(v) : "a"(a));
    return v;
}

// GroupNorm records (K, sum(x - K), sum((x - K)^2)) of one 16-row x 160-column slab of the stored fp16 output, read back from LDS
// (row stride `ld` halves): one record per channel group of `cg` channels (cg divides 40), K = the record's first element.  Lane
// (r = lane & 15, q = lane >> 4) sums row r of the groups of column quarter q in ascending channel order; the 16 rows are then
// combined by an xor butterfly (every lane ends with the same bits).  The order depends on nothing but the position inside the
// record, and both tile kernels call this one function: a record's bits do not depend on the tile origin or the kernel family.
// dst: the record of (this 16-row fragment, first channel group of the slab).  Vector stores only.
__device__ __forceinline__ void gn_slab_records(const half_t* slab, int ld, int cg, int lane, float* dst) {
    const int r = lane & 15, q = lane >> 4;
    const int ngq = 40 / cg;  // channel groups per column quarter
    for (int gi = 0; gi < ngq; ++gi) {
        const int gl = q * ngq + gi;
        const half_t* g0 = slab + gl * cg;
        const float K = (float)g0[0];
        const half_t* x = g0 + r * ld;
        float s = 0.f, qq = 0.f;
        for (int c = 0; c < cg; ++c) {
            const float f = (float)x[c] - K;
            s += f;
            qq = fmaf(f, f, qq);
        }
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            s += __shfl_xor(s, o, 64);
            qq += __shfl_xor(qq, o, 64);
        }
        if (r == 0) {
            float* o = dst + gl * 3;
            o[0] = K;
            o[1] = s;
            o[2] = qq;
        }
    }
}

// ---- launchers, one per kernel family: k filled by anyv2v_gemm_f16 (gemm.hip) from the descriptor and the plan (tiles, grid, split-K
// factor, raster); a launcher only picks the template instantiation ----
// 128 x NF*32 tile kernel (gemm_mfma.hip), persistent 192 x 320 kernel (gemm_big.hip), its ping-pong form (gemm_pp.hip; opt-in)
int av_gemm_mfma_launch(const GemmK& k, const AnyV2VGemmDesc* d, const GemmPlan& plan, hipStream_t s);
int av_gemm_big_launch(const GemmK& k, const AnyV2VGemmDesc* d, const GemmPlan& plan, hipStream_t s);
int av_gemm_pp_launch(const GemmK& k, const AnyV2VGemmDesc* d, const GemmPlan& plan, hipStream_t s);
// one thread per output element; the second pass of the split-K launches of the two kernels above (gemm_ref.hip)
int av_gemm_naive_launch(const GemmK& k, const AnyV2VGemmDesc* d, const GemmPlan& plan, hipStream_t s);
void av_gemm_splitk_reduce_launch(const GemmK& k, hipStream_t s);
// weight-stationary kernel (gemm_ws.hip): how (slab, row range) are dealt to the 256 blocks
struct WsPlan {
    int S;        // 160-column W slabs (= blocks per row range)
    int px;       // row ranges per XCD (px * S <= 32 blocks of the 32 CUs of an XCD)
    int nstrips;  // 32-row strips in M
    int spr;      // strips per row range
    int trace_waves;  // probe build: waves of a block that work (8; 4 / 1 = one wave per SIMD / per CU), tools/gemm_ws_trace.py
};
int av_gemm_ws_launch(const GemmK& k, const AnyV2VGemmDesc* d, const GemmPlan& plan, hipStream_t s);
// one-wave-per-SIMD persistent kernel (gemm_sw.hip): 192 x 320 tiles, 4 waves, direct 16-byte stores; its stream-K form
int av_gemm_sw_launch(const GemmK& k, const AnyV2VGemmDesc* d, const GemmPlan& plan, hipStream_t s);
int av_gemm_sw_sk_launch(const GemmK& k, const AnyV2VGemmDesc* d, const GemmPlan& plan, hipStream_t s);
// 3x3 convolution with the A operand reused from LDS across the dx taps (gemm_swh.hip)
int av_gemm_swh_launch(const GemmK& k, const AnyV2VGemmDesc* d, const GemmPlan& plan, hipStream_t s);
