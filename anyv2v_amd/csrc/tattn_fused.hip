// Temporal self-attention at the 320-channel (64x64) level with its QKV projection inside (gfx950): LayerNorm-folded projection,
// the 16 x 16 attention of every (pixel, head) and the output store in ONE kernel -- the [rows, 960] QKV tensor never reaches HBM.
//
// Replaces (reference = TIGER-AI-Lab/AnyV2V): attn.to_q / to_k / to_v and F.scaled_dot_product_attention of the temporal
// self-attention (i2vgen-xl/pnp_utils.py:283-316, plain form: no injection) behind BasicTransformerBlock.norm1 / norm2 of
// TransformerTemporalModel; to_out + residual stays the weight-stationary GEMM.  Bit-equal to the two launches it stands for
// (gemm_ws_kernel<320, 160, ..., LN> then short_attn_d64_kernel<1>): the K-step, the LayerNorm statistics and fold are the helpers of
// gemm_common.h, the score / softmax / PV arithmetic those of attn_short.h, and an output element depends on its own row / sequence only.
//
// Structure, following gemm_ws.hip:
//   * a block owns ONE head for its whole life: the head's 64 Q, 64 K and 64 V rows of W' [192][320] = 120 KB sit in LDS (five
//     [192][64] K-tiles, 16-byte chunks XOR-swizzled by row & 7, filled once by LDS-DMA), c1 and b' of those 192 columns beside it;
//   * every wave is autonomous and walks 32-row strips of its block's range; a strip is 2 neighbouring pixels x 16 frames (the rows
//     of a pixel lie HW apart; the two pixels give 1280 contiguous bytes per frame), i.e. the two MFMA row blocks of a strip are
//     two whole attention sequences.  Activations: the register ring of gemm_ws.hip (10 K-steps ahead, across strip boundaries);
//   * after the K loop: statistics, fold, fp16 rounding (what the GEMM would have stored), then per pixel Q | K through a wave-private
//     LDS patch into fragment layout, softmax, V and the output tile through the same patch, 128-byte row-segment stores;
//   * no barrier and no LDS-DMA after the slab fill: hipcc counts vmcnt / lgkmcnt itself.
// The five heads of a strip range run on the same XCD at the same time (tattn_plan.h), so x comes from HBM once per range.
#include "attn_short.h"
#include "gemm_common.h"
#include "tattn_plan.h"

namespace {
struct TattnK {
    const half_t* X;
    const half_t* W;      // [960][320]: W' = [Wq; Wk; Wv] diag(gamma)
    const half_t* bias;   // [960]
    const float* c1;      // [960]
    half_t* O;
    int ldx, ldo, HW;
    long long FHW;        // rows of one batch element
    float ln_eps, scale_log2;
};
constexpr int TA_K = TATTN_C, TA_NS = TATTN_SLAB_ROWS;
constexpr int TA_KS = TA_K / 32;      // MFMA K-steps per strip
constexpr int TA_NF = TA_NS / 16;     // 16-column fragments per slab: 4 Q, 4 K, 4 V
#ifndef TATTN_RING
#define TATTN_RING 5
#endif
#ifndef TATTN_WRING
#define TATTN_WRING 4
#endif
constexpr int TA_R = TATTN_RING, TA_WQ = TATTN_WRING;   // activation ring depth (K-steps) / weight-fragment ring, as in gemm_ws_kernel
constexpr bool TA_PAIRS = TA_R % 2 == 0;               // even ring: the two 64-byte halves of a 128-byte line are requested back to back
}  // namespace

__global__ __launch_bounds__(64 * TATTN_WAVES) void temporal_qkv_attn_c320_kernel(const TattnK p, const TattnPlan plan) {
    __shared__ __attribute__((aligned(16))) char smem[TATTN_LDS_BYTES];
    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int l15 = lane & 15, lq = lane >> 4;
    int head, s_begin, s_end;
    av_tattn_block(plan, blockIdx.x, TATTN_HEADS, &head, &s_begin, &s_end);
    if (s_begin >= s_end) return;   // block-uniform

    // first row of a strip: sequences 2 s and 2 s + 1 = pixels pix, pix + 1 of batch element b (HW is even)
    // (the strip index is wave-uniform: the row base stays in scalar registers)
    auto strip_row = [&](int strip) {
        const unsigned seq = 2u * (unsigned)strip;
        const unsigned b = seq / (unsigned)p.HW;
        return (long long)b * p.FHW + (seq - b * (unsigned)p.HW);
    };
    // activations as [16 rows][32 k] pieces, lane = (row l >> 2, 16-byte chunk l & 3), turned into the MFMA B-operand layout by
    // ds_bpermute (gemm_ws.hip); row l >> 2 of half mf is frame l >> 2 of pixel mf.  Address = uniform base of (strip, mf) + one
    // 32-bit lane offset (the plan keeps 16 HW ldx below 2^30 elements): one VGPR instead of four 64-bit pointers across the K loop
    const unsigned a_lane = ((unsigned)(lane >> 2) * (unsigned)p.HW * (unsigned)p.ldx + (lane & 3) * 8) * 2;   // bytes
    auto a_row = [&](int strip, int mf) {
        return (const char*)(p.X + (size_t)(strip_row(strip) + mf) * p.ldx);
    };
    auto a_load = [&](const char* base, int kstep) { return *(const h8*)(base + a_lane + kstep * 64); };
    const int bperm_addr = ((lane & 15) * 4 + (lane >> 4)) * 4;
    auto to_frag = [&](const h8& raw) {
        typedef int i4 __attribute__((ext_vector_type(4)));
        const i4 r = __builtin_bit_cast(i4, raw);
        i4 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = __builtin_amdgcn_ds_bpermute(bperm_addr, r[i]);
        return __builtin_bit_cast(h8, o);
    };
    h8 a[TA_R][2];
    int strip = s_begin + w;
    const char *pc0, *pc1;
    {   // first strip: requested before the W slab, lands while the DMA runs
        const int s0 = strip < s_end ? strip : s_begin;
        pc0 = a_row(s0, 0);
        pc1 = a_row(s0, 1);
#pragma unroll
        for (int s = 0; s < TA_R; ++s) {
            a[s][0] = a_load(pc0, s);
            a[s][1] = a_load(pc1, s);
        }
    }
    {   // W slab -> LDS: 120 pieces of 1 KB (8 rows x 128 B of one K-tile), source-side swizzle, destination lane-linear.  Slab row r
        // is row (r / 64) * 320 + 64 head + r % 64 of W': the head's Q, K, V rows
        for (int j = w; j < (TA_K / 64) * (TA_NS / 8); j += TATTN_WAVES) {
            const int kt = j / (TA_NS / 8), rg = j - kt * (TA_NS / 8);
            const int row = rg * 8 + (lane >> 3), kc = (lane & 7) ^ (row & 7);
            const int grow = (row >> 6) * TATTN_C + head * 64 + (row & 63);
            glds16(p.W + (size_t)grow * TA_K + kt * 64 + kc * 8, smem + kt * (TA_NS * 128) + rg * 1024);
        }
        if (tid < TA_NS / 4) {
            const int col = tid * 4, gcol = (col >> 6) * TATTN_C + head * 64 + (col & 63);
            *(h4*)(smem + TATTN_W_BYTES + tid * 8) = *(const h4*)(p.bias + gcol);
            *(f4*)(smem + TATTN_W_BYTES + TA_NS * 2 + tid * 16) = *(const f4*)(p.c1 + gcol);
        }
    }
    __syncthreads();  // (hipcc drains the LDS-DMA with vmcnt(0) here; nothing LDS-bound is in flight afterwards)

    const char* const wl = smem + l15 * 128;
    const int wsw[2] = {((0 * 4 + lq) ^ (l15 & 7)) * 16, ((1 * 4 + lq) ^ (l15 & 7)) * 16};
    half_t* const patch = (half_t*)(smem + TATTN_W_BYTES + TATTN_BIAS_BYTES + w * TATTN_PATCH_BYTES);
    const half_t* const bias_l = (const half_t*)(smem + TATTN_W_BYTES);
    static_assert(TA_KS % TA_R == 0, "static ring indices need TA_R | TA_KS");

    while (strip < s_end) {
        const int next = strip + TATTN_WAVES;
        const int pre = next < s_end ? next : strip;   // last strip of the wave: harmless re-read of its own rows
        const char* const pn0 = a_row(pre, 0);
        const char* const pn1 = a_row(pre, 1);
        const long long row0 = strip_row(strip);
        f4 acc[2][TA_NF];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < TA_NF; ++j) acc[i][j] = (f4){0.f, 0.f, 0.f, 0.f};
        f4 accq[2] = {(f4){0.f, 0.f, 0.f, 0.f}, (f4){0.f, 0.f, 0.f, 0.f}}, accs[2] = {(f4){0.f, 0.f, 0.f, 0.f}, (f4){0.f, 0.f, 0.f, 0.f}};
        h8 ones;
#pragma unroll
        for (int e = 0; e < 8; ++e) ones[e] = (half_t)1.0f;

        // K loop in issue order, pinned: the loop of gemm_ws_kernel (weight fragments TA_WQ - 1 MFMA pairs ahead, next K-step's
        // fragments during the current one, ring slots re-requested in (even, odd) pairs) over 12 instead of 10 fragments
        constexpr int NFR = TA_KS * TA_NF;
        auto wfrag = [&](int idx) {
            const int s = idx / TA_NF, nf = idx - s * TA_NF;
            return *(const h8*)(wl + (s >> 1) * (TA_NS * 128) + wsw[s & 1] + nf * 2048);
        };
        auto request = [&](int t, int n) {
#pragma unroll
            for (int mf = 0; mf < 2; ++mf)
#pragma unroll
                for (int i = 0; i < n; ++i) {
                    const int u = t + i;
                    const char* q = u < TA_KS ? (mf ? pc1 : pc0) : (mf ? pn1 : pn0);
                    a[u % TA_R][mf] = a_load(q, u < TA_KS ? u : u - TA_KS);
                }
        };
        h8 wq[TA_WQ], fr[2][2];
#pragma unroll
        for (int i = 0; i < TA_WQ - 1; ++i) wq[i] = wfrag(i);
        fr[0][0] = to_frag(a[0][0]);
        fr[0][1] = to_frag(a[0][1]);
        if (!TA_PAIRS) request(TA_R, 1);
        __builtin_amdgcn_s_setprio(1);   // the SIMD's other wave is usually in its epilogue while this one multiplies: MFMAs first
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int s = 0; s < TA_KS; ++s)
#pragma unroll
        for (int nf = 0; nf < TA_NF; ++nf) {
            const int idx = s * TA_NF + nf;
            if (idx + TA_WQ - 1 < NFR) wq[(idx + TA_WQ - 1) % TA_WQ] = wfrag(idx + TA_WQ - 1);
            ws_mfma_pair(wq[idx % TA_WQ], fr[s & 1][0], fr[s & 1][1], acc[0][nf], acc[1][nf]);
            if (nf == 4 || nf == 5) ws_ln_stats_step(fr[s & 1][nf - 4], ones, accq[nf - 4], accs[nf - 4]);   // row statistics, row block nf - 4
            if (nf == 2 && s + 1 < TA_KS) {
                fr[(s + 1) & 1][0] = to_frag(a[(s + 1) % TA_R][0]);
                fr[(s + 1) & 1][1] = to_frag(a[(s + 1) % TA_R][1]);
                if (!TA_PAIRS) request(s + 1 + TA_R, 1);
                if (TA_PAIRS && ((s + 1) & 1)) request(s + TA_R, 2);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        __builtin_amdgcn_s_setprio(0);
        pc0 = pn0;
        pc1 = pn1;

        // ---- wave-private epilogue.  The lane-derived offsets must not be hoisted out of the strip loop (they would live across the
        // K loop next to ~220 accumulator / fragment registers and spill): launder the lane id once per strip
        int lane_e = lane;
        asm volatile("" : "+v"(lane_e));
        const int l15_e = lane_e & 15, lq_e = lane_e >> 4;
        float ln_mean[2], ln_rstd[2];
#pragma unroll
        for (int mf = 0; mf < 2; ++mf) ws_ln_row_stats<TA_K>(accq[mf], accs[mf], l15_e, p.ln_eps, ln_mean[mf], ln_rstd[mf]);
#pragma unroll
        for (int mf = 0; mf < 2; ++mf)
#pragma unroll
            for (int nf = 0; nf < TA_NF; ++nf) {
                const f4 c1 = *(const f4*)((const char*)bias_l + TA_NS * 2 + (nf * 16 + 4 * lq_e) * 4);
                const h4 b = *(const h4*)(bias_l + nf * 16 + 4 * lq_e);
                ws_ln_fold(acc[mf][nf], c1, b, ln_mean[mf], ln_rstd[mf]);
            }
        // attention of the two sequences, one after the other through the patch.  Same-wave LDS traffic is ordered (in-order DS
        // queue); the fences keep hipcc from moving the accesses of one phase across those of the next
#pragma unroll
        for (int mf = 0; mf < 2; ++mf) {
            // Q | K as the GEMM would have stored them (one rounding to fp16), token-major: [16][TATTN_QK_LD]
#pragma unroll
            for (int nf = 0; nf < 8; ++nf) {
                h4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = (half_t)acc[mf][nf][r];
                *(h4*)(patch + l15_e * TATTN_QK_LD + nf * 16 + 4 * lq_e) = o;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            h8 qf[2], kf[2];   // lane (row = l15, k-chunk g): 8 halves at column 8 g + 32 ks
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                qf[ks] = *(const h8*)(patch + l15_e * TATTN_QK_LD + 8 * lq_e + 32 * ks);
                kf[ks] = *(const h8*)(patch + l15_e * TATTN_QK_LD + 64 + 8 * lq_e + 32 * ks);
            }
            h4 pf;
            float inv;
            short_attn_softmax(kf, qf, lq_e, TATTN_F, p.scale_log2, pf, inv);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // V overwrites the Q | K tile
            half_t* const vs = patch;
            half_t* const ow = patch + 16 * 64;
#pragma unroll
            for (int nf = 8; nf < TA_NF; ++nf) {   // V row-major [16 keys][64 d]
                h4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) o[r] = (half_t)acc[mf][nf][r];
                *(h4*)(vs + l15_e * 64 + (nf - 8) * 16 + 4 * lq_e) = o;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            short_attn_pv(vs, ow, pf, inv, l15_e, lq_e);
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
#pragma unroll
            for (int ps = 0; ps < 2; ++ps) {
                const int q = 8 * ps + (lane_e >> 3), ch = lane_e & 7;
                const h8 ov = *(const h8*)(ow + q * 72 + ch * 8);
                *(h8*)(p.O + (size_t)(row0 + mf + (long long)q * p.HW) * p.ldo + head * 64 + ch * 8) = ov;
            }
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the next sequence overwrites the patch
        }
        __builtin_amdgcn_sched_barrier(0);
        strip = next;
    }
}

extern "C" int anyv2v_temporal_qkv_attn_f16(const AnyV2VTattnDesc* d, void* stream) {
    AV_CHECK(d != nullptr, "temporal_qkv_attn: null descriptor");
    AV_CHECK(d->X && d->W && d->bias && d->ln_c1 && d->O, "temporal_qkv_attn: null X/W/bias/ln_c1/O");
    AV_CHECK(d->B > 0 && d->F > 0 && d->HW > 0, "temporal_qkv_attn: bad B/F/HW (%d %d %d)", d->B, d->F, d->HW);
    const TattnPlan plan = av_tattn_plan((int64_t)d->F * d->HW, d->B, d->C, d->heads, d->F, d->HW);
    if (!plan.supported) {
        anyv2v_set_error("temporal_qkv_attn: implemented for F = 16, C = 320, 5 heads, even HW, rows < 2^31 (got F %d C %d heads %d HW %d B %d)",
                         d->F, d->C, d->heads, d->HW, d->B);
        return ANYV2V_EUNSUPPORTED;
    }
    AV_CHECK(d->ldx >= d->C && d->ldo >= d->C && d->ldx % 8 == 0 && d->ldo % 8 == 0, "temporal_qkv_attn: ldx / ldo must be multiples of 8 and >= C");
    AV_CHECK((int64_t)16 * d->HW * (d->ldx > d->ldo ? d->ldx : d->ldo) < (1 << 30), "temporal_qkv_attn: 16 HW ld must stay below 2^30 elements");
    AV_CHECK(av_aligned16(d->X) && av_aligned16(d->O) && av_aligned16(d->W) && av_aligned16(d->ln_c1) && (((uintptr_t)d->bias) & 7) == 0,
             "temporal_qkv_attn: X / O / W / ln_c1 must be 16-byte aligned, bias 8-byte aligned");
    TattnK k;
    k.X = (const half_t*)d->X;
    k.W = (const half_t*)d->W;
    k.bias = (const half_t*)d->bias;
    k.c1 = d->ln_c1;
    k.O = (half_t*)d->O;
    k.ldx = d->ldx;
    k.ldo = d->ldo;
    k.HW = d->HW;
    k.FHW = (long long)d->F * d->HW;
    k.ln_eps = d->ln_eps;
    k.scale_log2 = d->scale * 1.4426950408889634f;
    hipLaunchKernelGGL(temporal_qkv_attn_c320_kernel, dim3(plan.grid), dim3(64 * TATTN_WAVES), 0, (hipStream_t)stream, k, plan);
    return av_launch_status("temporal_qkv_attn_c320");
}
