// Gather-GEMM for gfx950, the 128-row tile kernel: Linear / 1x1 conv, implicit-GEMM conv2d 3x3 (stride 1|2, optional folded nearest x2
// upsample) and the temporal (3,1,1) conv, all over channels-last token matrices, fp16 in / fp32 MFMA
// accumulate / fp16 out, with the bias / temb-broadcast / SiLU / GELU / GEGLU / residual epilogues fused.
//
// Replaces (reference = TIGER-AI-Lab/AnyV2V, i2vgen-xl/pnp_utils.py): conv1/conv2 :78,:107, time_emb_proj :81-88,
// conv_shortcut :117-122, residual :124, attn.to_q/to_k/to_v :175,:182-183, attn.to_out[0] :216, and the
// diffusers-0.26.3 Linear/Conv2d/Conv3d layers of I2VGenXLUNet behind pipeline_i2vgen_xl.py:1146.
//
// Wave tile: 64 x NF*16 via v_mfma_f32_16x16x32_f16 with SWAPPED operands (a = weight fragment, b = activation
// fragment) so that a lane ends up with 4 consecutive output channels of one token -> 8-byte LDS writes in the
// epilogue and full-line coalesced 16-byte global stores.  LDS tiles are [row][64 k] with the 16-byte chunk index
// XOR-swizzled by (row & 7): conflict-free for the ds_read_b128 fragment reads (MI355X guide, T2); with LDS-DMA the
// swizzle is applied on the global SOURCE address (destination stays lane-linear, guide rule 21).
//   gemm_mfma_kernel  : 128 x NF*32 x 64, 4 waves 2x2, 2 LDS stages (register- or LDS-DMA-staged), 2 blocks/CU.
// (the persistent large-M kernels on the same operand layout: gemm_big.hip, gemm_pp.hip, gemm_sw.hip, gemm_swh.hip)
#include <type_traits>

#include "gemm_common.h"

// ---------------------------------------------------------------------------------------------------------
// Shared epilogue: accumulators -> (+bias, +temb row vector, activation / GEGLU) -> fp16 tile staged in LDS ->
// (+residual) -> coalesced 16-byte stores.  Caller guarantees all waves are done with the pipeline LDS.
// GN: the launch also writes GroupNorm records of the stored tile (gn_slab_records; NF = 5, no GEGLU / split-K / fp32 output).
template <int NF, bool GEGLU, int BM, int NTHREADS, bool GN = false>
__device__ __forceinline__ void epilogue(const GemmK& p, f4 (&acc)[4][NF], char* smem, int m_blk, int n_blk, int wr,
                                         int wc, int lane, int tid, int split = 0, long long* tr = nullptr) {
    constexpr int BN = NF * 32;
    constexpr int BNO = GEGLU ? BN / 2 : BN;
    constexpr int CS_LD = BNO + 8;
    half_t* const Cs = (half_t*)smem;
    const int l15 = lane & 15, lq = lane >> 4;
    if (p.splits > 1) {  // split-K: raw fp32 partial tile; bias / temb / activation / residual happen in the reduce kernel
        float* dst = p.partial + (size_t)split * p.M * p.N;
#pragma unroll
        for (int mf = 0; mf < 4; ++mf) {
            const int m = m_blk + wr * 64 + mf * 16 + l15;
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) {
                const int n = n_blk + wc * NF * 16 + nf * 16 + 4 * lq;
                if (m < p.M && n + 4 <= p.N) *(f4*)(dst + (size_t)m * p.N + n) = acc[mf][nf];
            }
        }
        return;
    }
    if (p.act == ACT_F32OUT) {  // raw fp32 result (+bias): attention logits of the VAE's 512-wide single head
        float* dst = (float*)p.C;
#pragma unroll
        for (int mf = 0; mf < 4; ++mf) {
            const int m = m_blk + wr * 64 + mf * 16 + l15;
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) {
                const int n = n_blk + wc * NF * 16 + nf * 16 + 4 * lq;
                if (m < p.M && n + 4 <= p.N) {
                    f4 v = acc[mf][nf];
                    if (p.bias != nullptr) {
                        const h4 b = *(const h4*)(p.bias + n);
#pragma unroll
                        for (int r = 0; r < 4; ++r) v[r] += (float)b[r];
                    }
                    *(f4*)(dst + (size_t)m * p.ldc + n) = v;
                }
            }
        }
        return;
    }
    const int Nout = GEGLU ? p.N / 2 : p.N;
    const int n_out_blk = GEGLU ? n_blk / 2 : n_blk;
    constexpr int CPR = BNO / 8;                // 16-byte chunks per output-tile row
    constexpr int NIT = BM * CPR / NTHREADS;    // chunks per thread in the store phase
    static_assert(BM * CPR % NTHREADS == 0, "store phase assumes an exact chunk split");
    const bool full_chunks = (Nout & 7) == 0;   // wave-uniform; false only for the tiny-N layers (conv_out, N = 4)
    // Every global operand of the epilogue is requested up front, in one batch, so that their latencies overlap each
    // other and the convert / LDS-staging work below (in-kernel timestamps showed the previous form -- loads next to
    // their consumers -- spending 5-7 us per block in serialized L2 round trips, and 8-9 us in the residual loop):
    //   residual chunks of the store phase -> rr[], bias -> bvec[], temb row vector -> tvec[][] (only when present).
    h8 rr[NIT];
    if (p.R != nullptr && full_chunks) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int id = tid + it * NTHREADS;
            const int r = id / CPR, cc = id - r * CPR;
            const int m = m_blk + r, n0 = n_out_blk + cc * 8;
            rr[it] = *(const h8*)((m < p.M && n0 < Nout) ? p.R + (size_t)m * p.ldr + n0 : p.zeros);
        }
    }
    h4 bvec[NF];
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) {
        const int n = n_blk + wc * NF * 16 + nf * 16 + 4 * lq;
        const half_t* src = (p.bias != nullptr && n + 4 <= p.N) ? p.bias + n : p.zeros;
        bvec[nf] = *(const h4*)src;
    }
    h4 tvec[GEGLU ? 1 : 4][GEGLU ? 1 : NF];
    const bool has_rowvec = !GEGLU && p.rowvec != nullptr;
    if constexpr (!GEGLU) {
        if (has_rowvec) {
#pragma unroll
            for (int mf = 0; mf < 4; ++mf) {
                const int m = m_blk + wr * 64 + mf * 16 + l15;
                const bool ok = m < p.M;
                const half_t* rv = p.rowvec + (size_t)((ok ? m : 0) / p.rowvec_div) * p.ldrv;
#pragma unroll
                for (int nf = 0; nf < NF; ++nf) {
                    const int n = n_blk + wc * NF * 16 + nf * 16 + 4 * lq;
                    tvec[mf][nf] = *(const h4*)((ok && n + 4 <= p.N) ? rv + n : p.zeros);
                }
            }
        }
    }
    if constexpr (GEGLU) {
#pragma unroll
        for (int mf = 0; mf < 4; ++mf) {
            const int ml = wr * 64 + mf * 16 + l15;
#pragma unroll
            for (int np = 0; np < NF / 2; ++np) {
                h4 o;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    // h * gelu(gate) in fp32, ONE rounding (torch's fp16 path rounds proj, gelu and the product; its fp32 path --
                    // the reference this is checked against -- none of them)
                    const float hv = acc[mf][2 * np][r] + (float)bvec[2 * np][r];
                    const float gv = acc[mf][2 * np + 1][r] + (float)bvec[2 * np + 1][r];
                    o[r] = (half_t)(hv * av_gelu(gv));
                }
                *(h4*)(Cs + ml * CS_LD + wc * NF * 8 + np * 16 + 4 * lq) = o;
            }
        }
    } else {
        // The activation switch is hoisted out of the element loops (one wave-uniform branch per tile): left inside,
        // hipcc if-converts it and evaluates SiLU *and* erf-GELU for all 80 outputs of every thread (measured 5-7 us
        // per block on plain linear layers).
        auto stage = [&](auto act_tag) {
            constexpr int ACT = decltype(act_tag)::value;
#pragma unroll
            for (int mf = 0; mf < 4; ++mf) {
                const int ml = wr * 64 + mf * 16 + l15;
#pragma unroll
                for (int nf = 0; nf < NF; ++nf) {
                    const int nl = wc * NF * 16 + nf * 16 + 4 * lq;
                    h4 o;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v = acc[mf][nf][r] + (float)bvec[nf][r];
                        if (has_rowvec) v += (float)tvec[mf][nf][r];
                        if constexpr (ACT == ACT_SILU) v = av_silu(v);
                        if constexpr (ACT == ACT_GELU) v = av_gelu(v);
                        o[r] = (half_t)v;
                    }
                    *(h4*)(Cs + ml * CS_LD + nl) = o;
                }
            }
        };
        if (p.act == ACT_SILU)
            stage(std::integral_constant<int, ACT_SILU>{});
        else if (p.act == ACT_GELU)
            stage(std::integral_constant<int, ACT_GELU>{});
        else
            stage(std::integral_constant<int, ACT_NONE>{});
    }
    if (tr != nullptr && tid == 0) tr[24] = (long long)__builtin_amdgcn_s_memtime();
    __syncthreads();
    if (tr != nullptr && tid == 0) tr[25] = (long long)__builtin_amdgcn_s_memtime();
    if (full_chunks) {
#pragma unroll
        for (int it = 0; it < NIT; ++it) {
            const int id = tid + it * NTHREADS;
            const int r = id / CPR, cc = id - r * CPR;
            const int m = m_blk + r, n0 = n_out_blk + cc * 8;
            h8 v = *(const h8*)(Cs + r * CS_LD + cc * 8);
            if (p.R != nullptr) {
                v = v + rr[it];  // fp16 add: correctly rounded, i.e. what the fp32 add + rounding of two fp16 values gives
                if constexpr (GN) *(h8*)(Cs + r * CS_LD + cc * 8) = v;  // the records are taken of what is stored
            }
            if (m < p.M && n0 < Nout) *(h8*)(p.C + (size_t)m * p.ldc + n0) = v;
        }
        if constexpr (GN) {
            static_assert(!GEGLU && BN == 160 && BM % 16 == 0, "GroupNorm records: 160-column tiles of 16-row fragments");
            if (p.R != nullptr) __syncthreads();  // (block-uniform) the tile with the residual added is back in LDS
            const int wv = tid >> 6;
            for (int f = wv; f < BM / 16; f += NTHREADS / 64) {
                const int m0 = m_blk + f * 16;   // M % 16 == 0 (dispatch): a fragment lies inside M or outside, never across
                if (m0 < p.M)
                    gn_slab_records(Cs + f * 16 * CS_LD, CS_LD, p.gn_cg, lane,
                                    p.gn_stats + ((size_t)(m0 >> 4) * p.gn_groups + n_blk / p.gn_cg) * 3);
            }
        }
        return;
    }
    for (int id = tid; id < BM * CPR; id += NTHREADS) {  // ragged N: element-wise tail
        const int r = id / CPR, cc = id - r * CPR;
        const int m = m_blk + r;
        const int n0 = n_out_blk + cc * 8;
        if (m >= p.M || n0 >= Nout) continue;
        const h8 v = *(const h8*)(Cs + r * CS_LD + cc * 8);
        for (int e = 0; e < 8 && n0 + e < Nout; ++e) {
            float x = (float)v[e];
            if (p.R != nullptr) x += (float)p.R[(size_t)m * p.ldr + n0 + e];
            p.C[(size_t)m * p.ldc + n0 + e] = (half_t)x;
        }
    }
}

// one K-tile (64) of MFMA work for a 64 x NF*16 wave tile: all 2*(4+NF) fragment reads are issued first, so the
// compiler can retire them with counted lgkmcnt waits while the MFMAs of the first K-step already run (loading per
// K-step made it emit a full lgkmcnt(0) in front of every MFMA batch).
// KO (debug knock-outs, tools/gemm_trace.py): 4 = no fragment reads (register constants), 5 = no MFMAs
template <int NF, int KO = 0>
__device__ __forceinline__ void mma_tile(f4 (&acc)[4][NF], const char* as, const char* bs, int wr, int wc, int lane) {
    const int l15 = lane & 15, lq = lane >> 4;
    h8 af[2][4], bf[2][NF];
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        const int c = (ks * 4 + lq) ^ (l15 & 7);
        if constexpr (KO == 4) {
            h8 x;
#pragma unroll
            for (int e = 0; e < 8; ++e) x[e] = (half_t)(float)(lane + e);
            asm volatile("" : "+v"(x));
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) bf[ks][nf] = x;
#pragma unroll
            for (int mf = 0; mf < 4; ++mf) af[ks][mf] = x;
        } else {
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) bf[ks][nf] = *(const h8*)(bs + ((wc * NF * 16 + nf * 16 + l15) * 8 + c) * 16);
#pragma unroll
            for (int mf = 0; mf < 4; ++mf) af[ks][mf] = *(const h8*)(as + ((wr * 64 + mf * 16 + l15) * 8 + c) * 16);
        }
    }
    if constexpr (KO == 5) {
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) asm volatile("" ::"v"(bf[ks][nf]));
#pragma unroll
            for (int mf = 0; mf < 4; ++mf) asm volatile("" ::"v"(af[ks][mf]));
        }
        return;
    }
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int mf = 0; mf < 4; ++mf)
#pragma unroll
            for (int nf = 0; nf < NF; ++nf)
                acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[ks][nf], af[ks][mf], acc[mf][nf], 0, 0, 0);
    if constexpr (KO == 4) {
        __builtin_amdgcn_sched_barrier(0);
        return;
    }
    // scheduling contract for this region: all fragment reads first, then the MFMAs (hipcc otherwise sinks each read
    // next to its consumer and drains with lgkmcnt(0) four to six times per tile)
    // K-step 0 fragments, then K-step 0 MFMAs with the K-step 1 reads slotted in (1 read per 2 MFMAs), then the rest
    __builtin_amdgcn_sched_group_barrier(0x100, 4 + NF, 0);
#pragma unroll
    for (int i = 0; i < 4 + NF; ++i) {
        __builtin_amdgcn_sched_group_barrier(0x008, 2, 0);
        __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
    }
    __builtin_amdgcn_sched_group_barrier(0x008, 8 * NF - 2 * (4 + NF), 0);
    // keep the MFMAs above the caller's end-of-tile s_waitcnt (an asm "memory" clobber does not order register-only MFMAs)
    __builtin_amdgcn_sched_barrier(0);
}

// The same K-tile with the fragment reads as inline asm and counted waits (LDS-DMA kernel: the next tile's pieces are already in
// flight here, so hipcc would wait lgkmcnt(0) in front of both MFMA batches, see lds_frag): K-step 0's reads, then its MFMAs
// each waiting only for its own two fragments, K-step 1's reads slotted in one per two MFMAs.
template <int NF>
__device__ __forceinline__ void mma_tile_asm(f4 (&acc)[4][NF], const char* as, const char* bs, int wr, int wc, int lane) {
    const int l15 = lane & 15, lq = lane >> 4;
    const int c0 = ((0 * 4 + lq) ^ (l15 & 7)) * 16, c1 = ((1 * 4 + lq) ^ (l15 & 7)) * 16;
    const char* a0 = as + (wr * 64 + l15) * 128;
    const char* b0 = bs + (wc * NF * 16 + l15) * 128;
    const unsigned abase[2] = {(unsigned)(size_t)(a0 + c0), (unsigned)(size_t)(a0 + c1)};
    const unsigned bbase[2] = {(unsigned)(size_t)(b0 + c0), (unsigned)(size_t)(b0 + c1)};
    h8 af[2][4], bf[2][NF];
    int seq = 0, done = 0, a_seq[2][4] = {}, b_seq[2][NF] = {};
#define AV_RA(ks, mf) (af[ks][mf] = lds_frag(abase[ks], (mf) * 2048), a_seq[ks][mf] = ++seq)
#define AV_RB(ks, nf) (bf[ks][nf] = lds_frag(bbase[ks], (nf) * 2048), b_seq[ks][nf] = ++seq)
    AV_RA(0, 0);
#pragma unroll
    for (int nf = 0; nf < NF; ++nf) AV_RB(0, nf);
#pragma unroll
    for (int mf = 1; mf < 4; ++mf) AV_RA(0, mf);
    __builtin_amdgcn_sched_barrier(0);
    int slot = 0;  // K-step 1 reads issued so far, in the order a(1,0), b(1,0..NF-1), a(1,1..3)
#pragma unroll
    for (int ks = 0; ks < 2; ++ks)
#pragma unroll
        for (int mf = 0; mf < 4; ++mf)
#pragma unroll
            for (int nf = 0; nf < NF; ++nf) {
                const int need = a_seq[ks][mf] > b_seq[ks][nf] ? a_seq[ks][mf] : b_seq[ks][nf];
                if (need > done) {
                    lgkm_wait(seq - need);
                    done = need;
                    __builtin_amdgcn_sched_barrier(0);
                }
                acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[ks][nf], af[ks][mf], acc[mf][nf], 0, 0, 0);
                if (ks == 0 && ((mf * NF + nf) & 1) && slot < 4 + NF) {
                    __builtin_amdgcn_sched_barrier(0);
                    if (slot == 0)
                        AV_RA(1, 0);
                    else if (slot <= NF)
                        AV_RB(1, slot - 1);
                    else
                        AV_RA(1, slot - NF);
                    ++slot;
                    __builtin_amdgcn_sched_barrier(0);
                }
            }
#undef AV_RA
#undef AV_RB
    __builtin_amdgcn_sched_barrier(0);
}

// ---------------------------------------------------------------------------------------------------------
// KO (debug knock-outs): 2 = K loop issues only the W tiles, 3 = K loop issues no loads, 4 / 5 see mma_tile
template <int NF, bool GLDS, bool GEGLU, int MODE, bool TRACE = false, int KO = 0, bool GN = false>
__global__ __launch_bounds__(256, 2) void gemm_mfma_kernel(const GemmK p) {
    constexpr int BM = 128, BN = NF * 32;
    constexpr int A_BYTES = BM * 64 * 2;
    constexpr int B_BYTES = BN * 64 * 2;
    constexpr int NB = BN / 32;
    __shared__ __attribute__((aligned(16))) char smem[2 * (A_BYTES + B_BYTES)];
    char* const As0 = smem;
    char* const Bs0 = smem + 2 * A_BYTES;

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wr = w >> 1, wc = w & 1;
    int bid = blockIdx.x;
    const int nwg = gridDim.x;
    long long* tr = nullptr;
    if constexpr (TRACE) {
        tr = p.trace + (size_t)blockIdx.x * 32;
        if (tid == 0) {
            tr[0] = ((long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) << 32) | (unsigned)__builtin_amdgcn_s_getreg((31 << 11) | 4);
            tr[1] = (long long)__builtin_amdgcn_s_memrealtime();
            tr[2] = (long long)__builtin_amdgcn_s_memtime();
        }
    }
    if ((nwg & 7) == 0) bid = (bid & 7) * (nwg >> 3) + (bid >> 3);  // XCD-contiguous tile order (bijective)
    const int ntiles = nwg / p.splits;
    const int split = bid / ntiles;  // split-K: this block covers K-tiles [kt_begin, kt_end) of its output tile
    bid -= split * ntiles;
    const int mt = bid / p.tilesN, nt = bid - mt * p.tilesN;
    const int m_blk = mt * BM, n_blk = nt * BN;

    // staging: thread -> rows srow0 + 32 i, physical 16-B chunk pc, logical chunk kc
    const int srow0 = tid >> 3;
    const int pc = tid & 7;
    const int kc = pc ^ (srow0 & 7);
    RowInfo ri[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) ri[i] = make_row<MODE>(p, m_blk + srow0 + 32 * i);
    const half_t* bptr[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        int n = n_blk + srow0 + 32 * i;
        n = n < p.N ? n : p.N - 1;
        bptr[i] = p.W + (size_t)n * p.Ktot + kc * 8;
    }

    h8 ra[4], rb[NB];
    const int ntap = p.nt0 + p.nt1;
    const int nk_all = p.taps * ntap;
    const int kt_begin = (int)(((long long)nk_all * split) / p.splits);
    const int kt_end = (int)(((long long)nk_all * (split + 1)) / p.splits);
#pragma unroll
    for (int i = 0; i < NB; ++i) bptr[i] += (size_t)kt_begin * 64;
    AGen<MODE, 4> gen;
    gen.start(p, ri, kc, kt_begin, ntap);
    auto issue = [&](int buf, bool with_a = true) {  // loads the generator's current tile, then advances it
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if constexpr (GLDS) {
                if (with_a) glds16(gen.ap[i], As0 + buf * A_BYTES + (i * 256 + w * 64) * 16);
            } else {
                ra[i] = *(const h8*)gen.ap[i];
            }
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            if constexpr (GLDS)
                glds16(bptr[i], Bs0 + buf * B_BYTES + (i * 256 + w * 64) * 16);
            else
                rb[i] = *(const h8*)bptr[i];
            bptr[i] += 64;
        }
        gen.next(p, ri, kc, ntap);
    };
    auto commit = [&](int buf) {
#pragma unroll
        for (int i = 0; i < 4; ++i) *(h8*)(As0 + buf * A_BYTES + ((srow0 + 32 * i) * 8 + pc) * 16) = ra[i];
#pragma unroll
        for (int i = 0; i < NB; ++i) *(h8*)(Bs0 + buf * B_BYTES + ((srow0 + 32 * i) * 8 + pc) * 16) = rb[i];
    };

    f4 acc[4][NF];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = (f4){0.f, 0.f, 0.f, 0.f};

    const int nk = kt_end - kt_begin;
    issue(0);
    if constexpr (!GLDS) commit(0);
    if constexpr (GLDS) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    if constexpr (TRACE) if (tid == 0) tr[3] = (long long)__builtin_amdgcn_s_memtime();
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        const bool has_next = kt + 1 < nk;
        if (has_next && KO != 3) issue(cur ^ 1, KO != 2);
        if constexpr (GLDS && KO == 0)
            mma_tile_asm<NF>(acc, As0 + cur * A_BYTES, Bs0 + cur * B_BYTES, wr, wc, lane);
        else
            mma_tile<NF, KO>(acc, As0 + cur * A_BYTES, Bs0 + cur * B_BYTES, wr, wc, lane);
        if constexpr (TRACE) if (tid == 0 && kt < 8) tr[4 + kt] = (long long)__builtin_amdgcn_s_memtime();
        if constexpr (!GLDS) {
            if (has_next) commit(cur ^ 1);
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        __syncthreads();
        if constexpr (TRACE) if (tid == 0 && kt < 8) tr[12 + kt] = (long long)__builtin_amdgcn_s_memtime();
    }
    if constexpr (TRACE) if (tid == 0) tr[20] = (long long)__builtin_amdgcn_s_memtime();
    epilogue<NF, GEGLU, BM, 256, GN>(p, acc, smem, m_blk, n_blk, wr, wc, lane, tid, split, tr);
    if constexpr (TRACE) {
        if (tid == 0) tr[26] = (long long)__builtin_amdgcn_s_memtime();
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if (tid == 0) {
            tr[21] = (long long)__builtin_amdgcn_s_memtime();
            tr[22] = (long long)__builtin_amdgcn_s_memrealtime();
            tr[23] = nk;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side (eligibility, NF, tiles, grid and split-K factor: gemm_plan.cpp)
#define AV_GO(kernel, threads) hipLaunchKernelGGL((kernel), grid, dim3(threads), 0, s, k)
template <int MODE>
static int mfma_launch_mode(GemmK k, const AnyV2VGemmDesc* d, const GemmPlan& plan, hipStream_t s) {   // (k by value: the probe build sets k.trace)
    const bool geglu = d->act == ACT_GEGLU, gn = k.gn_stats != nullptr;
    const bool glds = (d->flags & ANYV2V_GEMM_LDS_DMA) != 0;
    const dim3 grid((unsigned)plan.grid);
#ifdef ANYV2V_EXPERIMENTS  // probe build only: phase timestamps / K-loop knock-outs (ANYV2V_GEMM_PROBE_*), tools/gemm_trace.py
#include "../../tools/experiments/gemm_dispatch_mfma_probe.inc"
#endif
    if (gn) AV_GO((gemm_mfma_kernel<5, true, false, MODE, false, 0, true>), 256);
    else if (geglu && glds) AV_GO((gemm_mfma_kernel<4, true, true, MODE>), 256);
    else if (geglu) AV_GO((gemm_mfma_kernel<4, false, true, MODE>), 256);
    else if (plan.nf == 5 && glds) AV_GO((gemm_mfma_kernel<5, true, false, MODE>), 256);
    else if (plan.nf == 5) AV_GO((gemm_mfma_kernel<5, false, false, MODE>), 256);
    else if (glds) AV_GO((gemm_mfma_kernel<4, true, false, MODE>), 256);
    else AV_GO((gemm_mfma_kernel<4, false, false, MODE>), 256);
    if (plan.splits > 1) av_gemm_splitk_reduce_launch(k, s);
    return av_launch_status("gemm_mfma");
}
#undef AV_GO

int av_gemm_mfma_launch(const GemmK& k, const AnyV2VGemmDesc* d, const GemmPlan& plan, hipStream_t s) {
    if (d->mode == MODE_CONV2D) return mfma_launch_mode<MODE_CONV2D>(k, d, plan, s);
    if (d->mode == MODE_TEMPORAL) return mfma_launch_mode<MODE_TEMPORAL>(k, d, plan, s);
    return mfma_launch_mode<MODE_LINEAR>(k, d, plan, s);
}
