// Persistent gather-GEMM for gfx950, the large-M workhorse: Linear / 1x1 conv, implicit-GEMM conv2d 3x3 (stride 1|2, optional folded
// nearest x2 upsample) and the temporal (3,1,1) conv over channels-last token matrices, fp16 in / fp32 MFMA accumulate / fp16 out,
// with the bias / temb-broadcast / GEGLU / residual epilogues fused (operand layout, swizzle and the swapped-operand MFMA: see
// gemm_mfma.hip).
//   gemm_big_kernel   : 64 MF x 320 x 64 (MF = 3: 192 rows), 8 waves 4x2 (wave tile 16 MF x 160), 2 LDS stages by LDS-DMA,
//                       persistent blocks with cross-tile prefetch and a wave-private epilogue; its split-K, residual and
//                       GroupNorm-record instantiations.
//
// Replaces (reference = TIGER-AI-Lab/AnyV2V, i2vgen-xl/pnp_utils.py): conv1/conv2 :78,:107, conv_shortcut :117-122, residual :124,
// attn.to_q/to_k/to_v :175,:182-183, attn.to_out[0] :216, and the diffusers-0.26.3 Linear/Conv2d/Conv3d layers of I2VGenXLUNet
// behind pipeline_i2vgen_xl.py:1146.
#include "gemm_common.h"

#ifdef ANYV2V_EXPERIMENTS
#include "../../tools/experiments/gemm_probe_config.h"   // AV_TRACE_TILE (which tile of a block the probe stamps)
#else
constexpr int AV_TRACE_TILE = 0;
#endif

// ---------------------------------------------------------------------------------------------------------
// Large-M persistent kernel: 256 x 320 x 64 block tile, 8 waves 4(M) x 2(N), wave tile 64 x 160 (4 x 10 MFMA 16x16x32
// fragments, 160 accumulator registers), two LDS stages of 72 KB filled by LDS-DMA.
//
// Why this shape (measured on the 128-row kernel with in-kernel timestamps and knock-outs, tools/gemm_trace.py):
// removing the MFMAs from its K loop saved 19 %, removing the LDS-DMA loads 45 % -- the loop is bound by the operand
// stream (14 KB of L2->LDS traffic and 14 DMA instructions per MFLOP), not by the matrix cores.  A 256 x 320 tile
// halves both (7 KB and 7 DMA instructions per MFLOP) and cuts fragment re-reads from LDS by 28 %.  All channel
// counts of the UNet are multiples of 320, so the 320-wide tile has no N waste.
//
// One block per CU (147 KB of LDS), grid = min(tiles, 256) persistent blocks walking tiles in XCD-contiguous order.
// The first K-tile of a block's NEXT output tile is requested during the last K-tile of the current one, so the
// prologue latency is paid once per block, and the epilogue runs wave-privately (16-row slabs staged through the
// just-consumed LDS stage, no block barriers) while that prefetch is in flight.
// One K-tile (64) for the 64 x 160 wave tile, written in the exact order it should issue (sched_barrier pins it):
//  * weight fragments roll: bf[nf] is read two fragments ahead of its four MFMAs, so at most three are live; the
//    activation fragments of the next K-step are read during the last four fragment groups (44 fragment registers
//    live next to the 160 accumulators, instead of 112 when hipcc hoists all 28 reads of the tile to the top);
//  * the next tile's LDS-DMA pieces are threaded through the first half of the MFMA stream, one per fragment group
//    (they have to sit here textually: an LDS-DMA load writes LDS, so hipcc never moves it across a ds_read).
template <int MF, typename PieceFn>
__device__ __forceinline__ void mma_tile_big(f4 (&acc)[MF][10], const char* as, const char* bs, int wr, int wc, int lane,
                                             PieceFn&& piece) {
    const int l15 = lane & 15, lq = lane >> 4;
    const char* a0 = as + (wr * MF * 16 + l15) * 128;
    const char* b0 = bs + (wc * 160 + l15) * 128;
    const int c0 = ((0 * 4 + lq) ^ (l15 & 7)) * 16, c1 = ((1 * 4 + lq) ^ (l15 & 7)) * 16;
    h8 af[2][MF], bf[2][10];
    // issue order of the reads (seq = running count) and, per fragment, its position in that order
    int seq = 0, a_seq[2] = {0, 0}, b_seq[2][10] = {};
    const unsigned abase[2] = {(unsigned)(size_t)(a0 + c0), (unsigned)(size_t)(a0 + c1)};
    const unsigned bbase[2] = {(unsigned)(size_t)(b0 + c0), (unsigned)(size_t)(b0 + c1)};
#define AV_RA(ks, mf) (af[ks][mf] = lds_frag(abase[ks], (mf) * 2048), a_seq[ks] = ++seq)
#define AV_RB(ks, nf) (bf[ks][nf] = lds_frag(bbase[ks], (nf) * 2048), b_seq[ks][nf] = ++seq)
#pragma unroll
    for (int mf = 0; mf < MF; ++mf) AV_RA(0, mf);
    AV_RB(0, 0);
    AV_RB(0, 1);
    __builtin_amdgcn_sched_barrier(0);
    int npiece = 0;
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
#pragma unroll
        for (int nf = 0; nf < 10; ++nf) {
            {   // everything up to the later of (this group's weight fragment, this K-step's last activation fragment)
                const int need = b_seq[ks][nf] > a_seq[ks] ? b_seq[ks][nf] : a_seq[ks];
                lgkm_wait(seq - need);
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int mf = 0; mf < MF; ++mf)
                acc[mf][nf] = __builtin_amdgcn_mfma_f32_16x16x32_f16(bf[ks][nf], af[ks][mf], acc[mf][nf], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
            // (activation fragment of the next K-step first: group (1, 0) then waits for all but the weight read behind it)
            if (ks == 0 && nf >= 10 - MF) AV_RA(1, nf - (10 - MF));
            if (nf + 2 < 10) {
                AV_RB(ks, nf + 2);
            } else if (ks == 0) {
                AV_RB(1, nf + 2 - 10);
            }
            if (npiece < MF + 5) piece(npiece++);
            __builtin_amdgcn_sched_barrier(0);
        }
    }
#undef AV_RA
#undef AV_RB
}

// RES: the launch adds a residual (p.R != nullptr).  A separate instantiation: its epilogue holds the residual rows of the whole
// wave tile in registers (requested right after the K loop, so that they land under the settle wait and the barrier that follow,
// and the epilogue itself issues no load at all -- a load there makes hipcc wait for the stores of the slabs before it).
// GN: the launch also writes GroupNorm records of every stored 16-row slab (gn_slab_records), a separate instantiation as well.
template <int MF, bool GEGLU, int MODE, bool TRACE = false, bool SPLIT = false, bool RES = false, bool GN = false>
__global__ __launch_bounds__(512) void gemm_big_kernel(const GemmK p) {
    static_assert(!(RES && (GEGLU || SPLIT)), "no residual on GEGLU / split-K launches");
    static_assert(!(GN && (GEGLU || SPLIT)), "no GroupNorm records on GEGLU / split-K launches");
    constexpr int BM = 64 * MF, BN = 320;  // four wave rows of MF 16-row fragments
    constexpr int A_BYTES = BM * 128, B_BYTES = BN * 128, STAGE_BYTES = A_BYTES + B_BYTES;
    constexpr int SLAB_LD = (GEGLU ? 80 : 160) + 8;          // halves; 16-byte aligned rows
    constexpr int SLAB_BYTES = 16 * SLAB_LD * 2;             // per wave
    static_assert(8 * SLAB_BYTES <= STAGE_BYTES, "epilogue slabs must fit in one pipeline stage");
    __shared__ __attribute__((aligned(16))) char smem[2 * STAGE_BYTES];

    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, wr = w >> 1, wc = w & 1;
    const int G = gridDim.x;
    // Tile order.  Classic: output tiles N-fastest, dealt to the XCDs in contiguous runs of G / 8 (an XCD's 32 blocks then share
    // A panels in its L2).  Rastered (p.rast_gm > 0; wide-N launches, G = 256): the 32 concurrent blocks of XCD x (= blockIdx & 7)
    // cover ONE super-tile of rast_gm x rast_gn output tiles, and an XCD's consecutive super-tiles keep the same W slabs -- with
    // N = 16 / 32 tiles the classic order makes every XCD stream the whole W (6.6 / 26 MB > its 4 MB L2) once per round.
    const bool rast = !SPLIT && p.rast_gm > 0;
    const int b0 = rast ? (int)blockIdx.x : (((G & 7) == 0) ? (blockIdx.x & 7) * (G >> 3) + (blockIdx.x >> 3) : blockIdx.x);
    const int tilesM = (p.M + BM - 1) / BM;
    const int ntiles_out = tilesM * p.tilesN;
    // SPLIT: work items are (split, output tile) -- split-K for launches whose tiles alone cannot fill the CUs (a separate
    // instantiation: the extra per-item state costs registers the plain kernel does not have)
    const int ntiles = SPLIT ? ntiles_out * p.splits : (rast ? G * ((p.rast_sm * p.rast_sn + 7) >> 3) : ntiles_out);
    // item -> output tile; false = a hole of the rastered order (ragged M, or past the last super-tile)
    auto decode = [&](int t, int& mt, int& nt) -> bool {
        if (!rast) {
            const int to = SPLIT ? t % ntiles_out : t;
            mt = to / p.tilesN;
            nt = to - mt * p.tilesN;
            return true;
        }
        const int q = (t & 7) + 8 * (t / G), j = (t % G) >> 3;
        int sm, sn;
        if (p.rast_nfast) {
            sm = q / p.rast_sn;
            sn = q - sm * p.rast_sn;
        } else {
            sn = q / p.rast_sm;
            sm = q - sn * p.rast_sm;
        }
        const int jm = j / p.rast_gn, jn = j - jm * p.rast_gn;
        mt = sm * p.rast_gm + jm;
        nt = sn * p.rast_gn + jn;
        return q < p.rast_sm * p.rast_sn && mt < tilesM;
    };
    auto next_valid = [&](int t) {
        int mt_, nt_;
        while (t < ntiles && !decode(t, mt_, nt_)) t += G;
        return t;
    };

    const int srow0 = tid >> 3, pc = tid & 7, kc = pc ^ (srow0 & 7);
    const int ntap = p.nt0 + p.nt1;
    const int nk_all = p.taps * ntap;
    auto k_begin = [&](int item) { return SPLIT ? (nk_all * (item / ntiles_out)) / p.splits : 0; };
    auto k_end = [&](int item) { return SPLIT ? (nk_all * (item / ntiles_out + 1)) / p.splits : nk_all; };

    // ---- producer state (the tile whose K-tiles are being requested; runs ahead of the consumer by one K-tile) ----
    RowInfo ri[4];  // (entries >= MF unused)
    const half_t* bptr;               // W row (n_blk + srow0); the other four rows sit 64 * Ktot halves apart
    const size_t brow = (size_t)64 * p.Ktot;
    AGen<MODE, 4> gen;
    auto producer_start = [&](int item) {
        int mt, nt;
        decode(item, mt, nt);
        const int kb = k_begin(item);
#pragma unroll
        for (int i = 0; i < 4; ++i) ri[i] = make_row<MODE>(p, i < MF ? mt * BM + srow0 + 64 * i : p.M);
        bptr = p.W + (size_t)(nt * BN + srow0) * p.Ktot + kc * 8 + (size_t)kb * 64;
        if constexpr (SPLIT)
            gen.start(p, ri, kc, kb, ntap);
        else
            gen.start(p, ri, kc);
    };
    auto advance = [&]() {
        bptr += 64;
        gen.next(p, ri, kc, ntap);
    };
    auto issue = [&](int stage) {
        char* st = smem + stage * STAGE_BYTES;
#pragma unroll
        for (int i = 0; i < MF; ++i) glds16(gen.ap[i], st + (i * 512 + w * 64) * 16);
#pragma unroll
        for (int i = 0; i < 5; ++i) glds16(bptr + i * brow, st + A_BYTES + (i * 512 + w * 64) * 16);
        advance();
    };

    f4 acc[MF][10];
    int tile = next_valid(b0);
    if (tile >= ntiles) return;
    producer_start(tile);
    issue(0);
    int stage = 0;
    bool landed = false;
    bool rederive = false;  // producer state is not carried across an epilogue (register pressure): re-derive it  // the current tile's first K-tile was already waited for (before the previous epilogue)
    while (true) {
        int mt, nt;
        decode(tile, mt, nt);
        const int nk = k_end(tile) - k_begin(tile);
        const int m_wave = mt * BM + wr * MF * 16;
        const int n_wave = nt * BN + wc * 160;
        const int next_tile = next_valid(tile + G);
        const bool has_next = next_tile < ntiles;
#pragma unroll
        for (int i = 0; i < MF; ++i)
#pragma unroll
            for (int j = 0; j < 10; ++j) acc[i][j] = (f4){0.f, 0.f, 0.f, 0.f};
        if (rederive) {
            producer_start(tile);
            advance();  // K-tile 0 of this tile was requested during the previous tile's last K-tile
        }

        for (int kt = 0; kt < nk; ++kt) {
            if constexpr (TRACE) if (tid == 0 && tile == b0 + AV_TRACE_TILE * G && kt < 8) p.trace[(size_t)blockIdx.x * 32 + 2 + 3 * kt] = (long long)__builtin_amdgcn_s_memtime();
            if (kt > 0 || !landed) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if constexpr (TRACE) if (tid == 0 && tile == b0 + AV_TRACE_TILE * G && kt == 3) p.trace[(size_t)blockIdx.x * 32 + 29] = (long long)__builtin_amdgcn_s_memtime();
            __builtin_amdgcn_s_barrier();  // K-tile kt landed for everyone; everyone is done with the other stage
            if constexpr (TRACE) if (tid == 0 && tile == b0 + AV_TRACE_TILE * G && kt < 8) p.trace[(size_t)blockIdx.x * 32 + 3 + 3 * kt] = (long long)__builtin_amdgcn_s_memtime();
            const bool last = kt + 1 == nk;
            // the pieces below then fetch K-tile 0 of the next tile -- or, when the block has none, K-tile 0 of THIS tile again into the idle
            // stage (never read): the producer always addresses data that exists, so no piece needs a per-lane "fetch ? pointer : zero
            // line" select (16 v_cndmask per wave and K-tile out of the MFMA stream)
            if (last) producer_start(has_next ? next_tile : tile);
            const bool fetch = !last || has_next;
            const char* as = smem + stage * STAGE_BYTES;
            char* st = smem + (stage ^ 1) * STAGE_BYTES;
            mma_tile_big<MF>(acc, as, as + A_BYTES, wr, wc, lane, [&](int i) {
                if (i < MF)
                    glds16(gen.ap[i], st + (i * 512 + w * 64) * 16);
                else
                    glds16(bptr + (i - MF) * brow, st + A_BYTES + ((i - MF) * 512 + w * 64) * 16);
            });
            if constexpr (TRACE) if (tid == 0 && tile == b0 + AV_TRACE_TILE * G && kt < 8) p.trace[(size_t)blockIdx.x * 32 + 4 + 3 * kt] = (long long)__builtin_amdgcn_s_memtime();
            if (fetch) advance();
            stage ^= 1;
        }
        if constexpr (TRACE) if (tid == 0 && tile == b0 + AV_TRACE_TILE * G) p.trace[(size_t)blockIdx.x * 32 + 26] = (long long)__builtin_amdgcn_s_memtime();
        // `stage` now names the buffer holding the prefetched K-tile 0 of the next tile; stage ^ 1 was just consumed
        constexpr int OUT_W = GEGLU ? 80 : 160;       // output columns of this wave
        constexpr int CPRW = OUT_W / 8;               // 16-byte chunks per slab row
        constexpr int NIT = (16 * CPRW + 63) / 64;    // store iterations per slab (5, or 3 with a half-empty last one)
        const int n_out_wave = GEGLU ? n_wave / 2 : n_wave;
        h8 rr[RES ? MF : 1][NIT];
        if constexpr (RES) {   // all residual rows of the wave tile (rows past M: clamped, never stored)
            int lane_r = lane;
            asm volatile("" : "+v"(lane_r));   // (not hoisted out of the tile loop: see lane_e below)
#pragma unroll
            for (int mf = 0; mf < MF; ++mf)
#pragma unroll
                for (int it = 0; it < NIT; ++it) {
                    const int c = it * 64 + lane_r;
                    const int row = c / CPRW, cc = c - row * CPRW;
                    int m = m_wave + mf * 16 + row;
                    m = m < p.M ? m : p.M - 1;
                    rr[mf][it] = *(const h8*)(p.R + (size_t)m * p.ldr + n_out_wave + cc * 8);
                }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // settle the prefetch BEFORE the stores below enter the queue
        if constexpr (TRACE) if (tid == 0 && tile == b0 + AV_TRACE_TILE * G) p.trace[(size_t)blockIdx.x * 32 + 30] = (long long)__builtin_amdgcn_s_memtime();
        __builtin_amdgcn_s_barrier();                     // every wave is done reading the consumed stage
        if constexpr (TRACE) if (tid == 0 && tile == b0 + AV_TRACE_TILE * G) p.trace[(size_t)blockIdx.x * 32 + 31] = (long long)__builtin_amdgcn_s_memtime();
        landed = true;
        rederive = true;

        // ---------------- wave-private epilogue: MF slabs of 16 rows x 160 (GEGLU: 80) output columns ----------------
        // (measured alternatives, both bit-equal and slower: pair-wise LDS exchange for full-row stores, round 1; a block-cooperative
        //  form -- four barrier-separated steps through LDS, all 512 threads storing whole rows -- round 2, 5-40 % slower on the
        //  3-clip shapes: with one block per CU nothing overlaps its serial steps.  profiles/r02_gemm_coop_epilogue_ab.txt)
        // the epilogue's lane-derived offsets must not be hoisted out of the tile loop (they would live across the K loop
        // and spill): launder the lane id once per tile
        int lane_e = lane;
        asm volatile("" : "+v"(lane_e));
        const int l15 = lane_e & 15, lq = lane_e >> 4;
        if constexpr (SPLIT) {  // raw fp32 partial tile; gemm_splitk_reduce_kernel sums the splits in order and finishes
            float* dst = p.partial + (size_t)(tile / ntiles_out) * p.M * p.N;
#pragma unroll
            for (int mf = 0; mf < MF; ++mf) {
                const int m = m_wave + mf * 16 + l15;
#pragma unroll
                for (int nf = 0; nf < 10; ++nf)
                    if (m < p.M) *(f4*)(dst + (size_t)m * p.N + n_wave + nf * 16 + 4 * lq) = acc[mf][nf];
            }
            if (!has_next) break;
            tile = next_tile;
            continue;
        }
        if constexpr (SPLIT) __builtin_unreachable();
        half_t* const slab = (half_t*)(smem + (stage ^ 1) * STAGE_BYTES + w * SLAB_BYTES);
        // (dispatch guarantees N % 320 == 0 and act in {none, GEGLU}; rows are guarded: M need not be a multiple of BM)
        h4 bvec[10];
#pragma unroll
        for (int nf = 0; nf < 10; ++nf)
            bvec[nf] = *(const h4*)(p.bias != nullptr ? p.bias + n_wave + nf * 16 + 4 * lq : p.zeros);
        if constexpr (RES) {   // they landed under the settle wait above; tell the compiler so ONCE, before the first store
#pragma unroll
            for (int mf = 0; mf < MF; ++mf)
#pragma unroll
                for (int it = 0; it < NIT; ++it) asm volatile("" : "+v"(rr[mf][it]));
        }
        // per 16-row slab: (+bias, +temb row vector | GEGLU) -> fp16 -> LDS (turns lane-owns-4-channels into
        // row-contiguous 16-byte chunks) -> (+residual) -> store.
#pragma unroll
        for (int mf = 0; mf < MF; ++mf) {
            if constexpr (GEGLU) {
#pragma unroll
                for (int np = 0; np < 5; ++np) {
                    h4 o;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float hv = acc[mf][2 * np][r] + (float)bvec[2 * np][r];
                        const float gv = acc[mf][2 * np + 1][r] + (float)bvec[2 * np + 1][r];
                        o[r] = (half_t)(hv * av_gelu(gv));
                    }
                    *(h4*)(slab + l15 * SLAB_LD + np * 16 + 4 * lq) = o;
                }
            } else {
                const bool has_rv = p.rowvec != nullptr;
                const int mrow = m_wave + mf * 16 + l15;
                const half_t* rv = has_rv ? p.rowvec + (size_t)((mrow < p.M ? mrow : 0) / p.rowvec_div) * p.ldrv + n_wave + 4 * lq
                                          : p.zeros;
#pragma unroll
                for (int nf = 0; nf < 10; ++nf) {
                    h4 tv = (h4){0, 0, 0, 0};
                    if (has_rv) tv = *(const h4*)(rv + nf * 16);
                    h4 o;
#pragma unroll
                    for (int r = 0; r < 4; ++r) o[r] = (half_t)(acc[mf][nf][r] + (float)bvec[nf][r] + (float)tv[r]);
                    *(h4*)(slab + l15 * SLAB_LD + nf * 16 + 4 * lq) = o;
                }
            }
            // same-wave LDS traffic is ordered; the compiler inserts the lgkmcnt wait for the read-back
#pragma unroll
            for (int it = 0; it < NIT; ++it) {
                const int c = it * 64 + lane_e;
                const int row = c / CPRW, cc = c - row * CPRW;
                const bool ok = (16 * CPRW % 64 == 0 || c < 16 * CPRW) && m_wave + mf * 16 + row < p.M;
                h8 v = *(const h8*)(slab + (ok ? row * SLAB_LD + cc * 8 : 0));
                if constexpr (RES) v = v + rr[mf][it];  // fp16 add: correctly rounded, == the fp32 add + rounding of two fp16 values
                if constexpr (RES && GN) {   // the records are taken of what is stored
                    if (ok) *(h8*)(slab + row * SLAB_LD + cc * 8) = v;
                }
                if (ok) *(h8*)(p.C + (size_t)(m_wave + mf * 16 + row) * p.ldc + n_out_wave + cc * 8) = v;
            }
            if constexpr (GN) {   // M % 16 == 0 (dispatch): a slab lies inside M or outside, never across
                const int m0 = m_wave + mf * 16;
                if (m0 < p.M)
                    gn_slab_records(slab, SLAB_LD, p.gn_cg, lane_e, p.gn_stats + ((size_t)(m0 >> 4) * p.gn_groups + n_wave / p.gn_cg) * 3);
            }
        }

        if constexpr (TRACE) {
            if (tid == 0 && tile == b0 + AV_TRACE_TILE * G) {
                p.trace[(size_t)blockIdx.x * 32 + 27] = (long long)__builtin_amdgcn_s_memtime();
                p.trace[(size_t)blockIdx.x * 32 + 28] = nk;
            }
        }
        if (!has_next) break;
        tile = next_tile;
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side (eligibility, tiles, grid, split-K factor and tile order: gemm_plan.cpp)
#define AV_GO(kernel, threads) hipLaunchKernelGGL((kernel), grid, dim3(threads), 0, s, k)
template <int MODE>
static int big_launch_mode(GemmK k, const AnyV2VGemmDesc* d, const GemmPlan& plan, hipStream_t s) {   // (k by value: the probe build sets k.trace)
    const bool geglu = d->act == ACT_GEGLU, res = d->R != nullptr, gn = k.gn_stats != nullptr;
    const dim3 grid((unsigned)plan.grid);
    if (plan.splits > 1) {
        AV_GO((gemm_big_kernel<3, false, MODE, false, true>), 512);
        av_gemm_splitk_reduce_launch(k, s);
        return av_launch_status("gemm_big<split-K>");
    }
#ifdef ANYV2V_EXPERIMENTS  // probe build only (make experiments): phase-timestamp instantiations, tools/gemm_big_trace.py
#include "../../tools/experiments/gemm_dispatch_big_probe.inc"
#endif
    if (gn) {   // (never GEGLU: the plan declines)
        if (res) AV_GO((gemm_big_kernel<3, false, MODE, false, false, true, true>), 512);
        else AV_GO((gemm_big_kernel<3, false, MODE, false, false, false, true>), 512);
        return av_launch_status("gemm_big<gn>");
    }
    if constexpr (MODE == MODE_LINEAR) {
        if (geglu) {
            AV_GO((gemm_big_kernel<3, true, MODE_LINEAR>), 512);
            return av_launch_status("gemm_big");
        }
    }
    if (res) AV_GO((gemm_big_kernel<3, false, MODE, false, false, true>), 512);
    else AV_GO((gemm_big_kernel<3, false, MODE>), 512);
    return av_launch_status("gemm_big");
}
#undef AV_GO

int av_gemm_big_launch(const GemmK& k, const AnyV2VGemmDesc* d, const GemmPlan& plan, hipStream_t s) {
    if (d->mode == MODE_CONV2D) return big_launch_mode<MODE_CONV2D>(k, d, plan, s);
    if (d->mode == MODE_TEMPORAL) return big_launch_mode<MODE_TEMPORAL>(k, d, plan, s);
    return big_launch_mode<MODE_LINEAR>(k, d, plan, s);
}
