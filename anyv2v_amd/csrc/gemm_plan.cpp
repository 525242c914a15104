// Launch planning of anyv2v_gemm_f16 (gemm_plan.h): every rule that decides which kernel runs a descriptor and how, with the
// measurements behind each threshold.  Host code only.
#include "gemm_plan.h"

const char* av_gemm_family_name(GemmFamily f) {
    static const char* const names[] = {"naive", "ws", "ws_ln", "mfma128", "big", "pp", "sw", "sw_streamk", "swh"};
    static_assert(sizeof(names) / sizeof(names[0]) == GEMM_FAMILY_COUNT, "one name per family");
    return names[f];
}

namespace {
bool aligned16(const void* p) { return (((uintptr_t)p) & 15) == 0; }
int ceil_div(int a, int b) { return (a + b - 1) / b; }

#define PLAN_FAIL(code, ...) do { anyv2v_set_error(__VA_ARGS__); p.status = code; return p; } while (0)
#define PLAN_CHECK(cond, ...) if (!(cond)) PLAN_FAIL(ANYV2V_EINVAL, __VA_ARGS__)

// ---- weight-stationary kernel (gemm_ws.hip): can this launch run on it, and at which slab width ----
int ws_slab_cols(const AnyV2VGemmDesc& d) {   // 0 = shape not covered
    if (d.C0 == 320) return 160;
    // K = 512 (transformer_in): GEGLU with 128-column slabs (1291 -> 834 us at 196608 rows); plain launches would need 64-column
    // slabs (128 + their epilogue slabs exceed LDS), which only pays for N = 512 (x 1.07-1.16; QKV N = 1536: x 0.87-0.96, left to
    // the tile kernels) -- profiles/r03_gemm_ws_ab.txt
    if (d.C0 == 512) return d.act == ACT_GEGLU ? 128 : (d.N == 512 ? 64 : 0);
    return 0;
}
bool ws_eligible(const AnyV2VGemmDesc& d) {
    const int ns = ws_slab_cols(d);
    if (d.ln_c1 != nullptr && (d.R != nullptr || (d.C0 == 512 && d.act != ACT_GEGLU))) return false;
    return d.mode == MODE_LINEAR && ns > 0 && d.C1 == 0 && d.N % ns == 0 && d.N / ns <= 32 &&
           (d.act == ACT_NONE || (d.act == ACT_GEGLU && d.R == nullptr)) && d.rowvec == nullptr && d.M > 0;
}

// ---- one-wave-per-SIMD persistent kernel (gemm_sw.hip) ----
bool sw_eligible(const AnyV2VGemmDesc& d, int nk) {
    const bool geglu = d.act == ACT_GEGLU;
    return d.N % 320 == 0 && (geglu ? d.mode == MODE_LINEAR && d.R == nullptr && d.rowvec == nullptr : d.act == ACT_NONE) &&
           !(d.R != nullptr && d.rowvec != nullptr) && nk >= 2 && d.ldc % 8 == 0 && (d.R == nullptr || d.ldr % 8 == 0) &&
           (d.rowvec == nullptr || d.ldrv % 8 == 0);
}
size_t sw_sk_workspace(int blocks) { return (size_t)2 * blocks * AV_GEMM_BM * AV_GEMM_BN * sizeof(float); }   // 2 fp32 tiles per block
// Blocks the stream-K form would use, or 0 when it should not be taken: the launch's (tile, K-tile) units are dealt evenly to
// min(256, units / 4) blocks.  It pays where whole tiles quantise badly onto 256 CUs (tiles / (rounds x 256) below ~0.9) and every
// block still gets a few K-tiles.
int sw_sk_blocks(int tiles, int nk, bool force) {
    const long long U = (long long)tiles * nk;
    if (U < 256 * 4 || U > (1ll << 22)) return force && U >= 8 ? (int)(U / 4 < 256 ? U / 4 : 256) : 0;
    if (force) return 256;
    const int rounds = (tiles + 255) / 256;
    const double eff = (double)tiles / (rounds * 256.0);
    return eff < 0.9 ? 256 : 0;
}

// ---- LDS-patch 3x3 convolution (gemm_swh.hip) ----
bool swh_eligible(const AnyV2VGemmDesc& d) {
    return d.mode == MODE_CONV2D && d.stride == 1 && d.up == 0 && d.asym == 0 && d.Hi == d.Ho && d.Wi == d.Wo &&
           (d.Wi == 16 || d.Wi == 32 || d.Wi == 64) && d.N % 320 == 0 && d.act == ACT_NONE && d.C0 % 64 == 0 && d.C1 % 64 == 0 &&
           !(d.R != nullptr && d.rowvec != nullptr) && d.ldc % 8 == 0 && (d.R == nullptr || d.ldr % 8 == 0) &&
           (d.rowvec == nullptr || d.ldrv % 8 == 0);
}

// GroupNorm records from the epilogue (AnyV2VGemmDesc.gn_stats): shapes the record layout covers, whatever the plan.
bool gn_shape_ok(const AnyV2VGemmDesc& d) {
    if (d.gn_groups <= 0 || d.gn_rows_per_group <= 0 || d.N % 160 != 0 || d.N % d.gn_groups != 0) return false;
    const int cg = d.N / d.gn_groups;
    return 40 % cg == 0 && d.M % 16 == 0 && d.gn_rows_per_group % 16 == 0 && d.M % d.gn_rows_per_group == 0 &&
           (d.act == ACT_NONE || d.act == ACT_SILU || d.act == ACT_GELU);
}

// 192 x 320 tiles of a persistent kernel on min(tiles, 256) blocks.
void persistent_grid(GemmPlan& p, const AnyV2VGemmDesc& d) {
    p.tilesN = d.N / AV_GEMM_BN;
    p.tiles = ceil_div(d.M, AV_GEMM_BM) * p.tilesN;
    p.grid = p.tiles < 256 ? p.tiles : 256;
}
// Tile order of wide-N launches (gemm_big_kernel, gemm_sw_kernel): 8 x 4 super-tiles per XCD round when N has >= 8 tiles (the GEGLU
// up-projections at 640 / 1280 channels: 16 / 32 N-tiles).  ANYV2V_GEMM_RASTER_SHIFT code: 0 auto, 1 classic order, 2..6 force
// rast_gm = 4, 8, 16, 32, 2; ANYV2V_GEMM_RASTER_NFAST: super-tiles N-fastest.  Same arithmetic per output element in every order.
void raster(GemmPlan& p, const AnyV2VGemmDesc& d) {
    const int code = (d.flags >> ANYV2V_GEMM_RASTER_SHIFT) & 7;
    static const int gm_of[8] = {0, 0, 4, 8, 16, 32, 2, 0};
    int gm = gm_of[code];
    if (code == 0 && p.tilesN >= 8 && p.tiles >= 512) gm = 8;
    if (gm > 0 && p.grid == 256 && p.tilesN % (32 / gm) == 0) {
        p.rast_gm = gm;
        p.rast_gn = 32 / gm;
        p.rast_sm = ceil_div(ceil_div(d.M, AV_GEMM_BM), gm);
        p.rast_sn = p.tilesN / p.rast_gn;
        p.rast_nfast = (d.flags & ANYV2V_GEMM_RASTER_NFAST) != 0;
    }
}

}  // namespace

GemmPlan av_gemm_plan(const AnyV2VGemmDesc& d, int hinted_rows) {
    GemmPlan p = {};   // (ANYV2V_OK)
    p.nf = 4;
    p.splits = p.tilesN = 1;
    // the family is decided: `what` is how a launch with gn_stats hears that this family writes no GroupNorm records
    auto take = [&p](GemmFamily family, const char* what) { p.family = family; p.gn_decline = what; return p; };
    PLAN_CHECK(d.A0 && d.W, "gemm: null A0/W/C");
    PLAN_CHECK(d.M > 0 && d.N > 0 && d.C0 > 0 && d.C1 >= 0, "gemm: bad M/N/C0/C1 (%d %d %d %d)", d.M, d.N, d.C0, d.C1);
    PLAN_CHECK(d.mode >= 0 && d.mode <= 2, "gemm: bad mode %d", d.mode);
    PLAN_CHECK(d.act >= 0 && d.act <= 4, "gemm: bad act %d", d.act);
    PLAN_CHECK(d.act != ACT_F32OUT || (d.rowvec == nullptr && d.R == nullptr && d.N % 4 == 0 && d.ldc % 4 == 0),
               "gemm: fp32 output supports bias only and needs N, ldc multiples of 4");
    PLAN_CHECK(d.asym == 0 || d.asym == 1, "gemm: asym must be 0 or 1");
    PLAN_CHECK(d.C1 == 0 || d.A1 != nullptr, "gemm: C1 > 0 but A1 is null");
    PLAN_CHECK(d.rowvec == nullptr || d.rowvec_div > 0, "gemm: rowvec needs rowvec_div > 0");
    if (d.mode == MODE_CONV2D) {
        PLAN_CHECK(d.Hi > 0 && d.Wi > 0 && d.Ho > 0 && d.Wo > 0 && (d.stride == 1 || d.stride == 2), "gemm: bad conv geometry");
        PLAN_CHECK(d.M % (d.Ho * d.Wo) == 0, "gemm: M not a multiple of Ho*Wo");
        PLAN_CHECK(d.up == 0 || d.up == 1, "gemm: up must be 0 or 1");
    }
    if (d.mode == MODE_TEMPORAL) { PLAN_CHECK(d.F > 0 && d.HW > 0 && d.M % (d.F * d.HW) == 0, "gemm: bad temporal geometry"); }
    const bool geglu = d.act == ACT_GEGLU;
    if (geglu) {
        PLAN_CHECK(d.N % 32 == 0, "gemm: GEGLU needs N %% 32 == 0");
        PLAN_CHECK(d.rowvec == nullptr, "gemm: GEGLU with rowvec unsupported");
    }
    p.taps = d.mode == MODE_LINEAR ? 1 : (d.mode == MODE_CONV2D ? 9 : 3);
    p.nk = p.taps * (d.C0 / 64 + d.C1 / 64);
    p.vec_epi = (((uintptr_t)d.bias & 7) == 0) && (((uintptr_t)d.rowvec & 7) == 0) && (d.ldrv % 4 == 0) && (d.N % 4 == 0);
    const int flags = d.flags, nk = p.nk;
    const bool glds = (flags & ANYV2V_GEMM_LDS_DMA) != 0;
    const bool fast = !(flags & ANYV2V_GEMM_NAIVE) && d.C0 % 64 == 0 && d.C1 % 64 == 0 && d.lda0 % 8 == 0 &&
                      (d.C1 == 0 || d.lda1 % 8 == 0) && d.ldc % 8 == 0 && aligned16(d.A0) && (d.C1 == 0 || aligned16(d.A1)) &&
                      aligned16(d.W) && aligned16(d.C) && (d.R == nullptr || (d.ldr % 8 == 0 && aligned16(d.R))) &&
                      (!geglu || d.N % 128 == 0) && p.vec_epi;

    // K = 320 Linear layers with many rows (the 64x64 level): weight-stationary streaming kernel, 256 blocks, tilesN = its W slabs
    // (forced below the row threshold only by tests: a small M leaves most waves idle)
    const bool ws_ok = fast && glds && ws_eligible(d);
    const bool ws_take = ws_ok && !(flags & (ANYV2V_GEMM_NO_WS | ANYV2V_GEMM_NO_BIG)) && (hinted_rows >= 32768 || (flags & ANYV2V_GEMM_FORCE_WS));
    if (d.ln_c1 != nullptr || ws_take) {   // LayerNorm folded into the GEMM: only the weight-stationary kernel implements it
        p.grid = 256;
        if (ws_ok) p.tilesN = d.N / ws_slab_cols(d);
        if (d.ln_c1 == nullptr) return take(GEMM_WS, "the weight-stationary kernel");
        take(GEMM_WS_LN, "the LayerNorm-fold kernel");
        if (!(ws_ok && aligned16(d.ln_c1)))
            PLAN_FAIL(ANYV2V_EUNSUPPORTED, "gemm: ln_c1 (LayerNorm fold) needs mode 0, C0 = 320 (N %% 160 = 0) or C0 = 512 with GEGLU "
                      "(N %% 128 = 0), no residual / rowvec, 16-byte aligned operands -- got C0 %d N %d act %d", d.C0, d.N, d.act);
        return p;
    }
    if (!fast) {
        p.grid = (int)(unsigned)(((long long)d.M * (geglu ? d.N / 2 : d.N) + 255) / 256);
        return take(GEMM_NAIVE, "the naive kernel");
    }
    const bool sw_on = glds && !(flags & ANYV2V_GEMM_NO_SW);
    // Stream-K form of the one-wave-per-SIMD kernel: never for a batch-hinted launch (its K ranges depend on the launch's own tile
    // count, i.e. they fix the arithmetic, and a hinted launch has to reproduce the arithmetic of the launch it stands for).
    if (sw_on && (flags & (ANYV2V_GEMM_STREAMK | ANYV2V_GEMM_FORCE_STREAMK)) && sw_eligible(d, nk) && hinted_rows == d.M &&
        d.workspace != nullptr) {
        persistent_grid(p, d);
        const int blocks = sw_sk_blocks(p.tiles, nk, (flags & ANYV2V_GEMM_FORCE_STREAMK) != 0);
        if (blocks > 0 && sw_sk_workspace(blocks) <= (size_t)d.workspace_bytes) {
            p.grid = p.sk_blocks = blocks;
            return take(GEMM_SW_STREAMK, "the stream-K kernel");
        }
    }
    if (sw_on && (flags & ANYV2V_GEMM_SWH) && swh_eligible(d)) {
        persistent_grid(p, d);
        return take(GEMM_SWH, "the LDS-patch convolution kernel");
    }
    if (sw_on && (flags & ANYV2V_GEMM_SW) && sw_eligible(d, nk)) {
        persistent_grid(p, d);
        raster(p, d);
        return take(GEMM_SW, "the one-wave-per-SIMD kernel");
    }
    // 128-row kernel tile width: 160 columns (NF = 5) where N allows it, except where 128-column tiles (NF = 4) quantise better onto
    // the 256 CUs x 2 resident blocks -- more CUs busy when there is less than one tile per CU, or the same number of rounds with
    // 20 % smaller tiles (ANYV2V_GEMM_NF4 / NF5 force the width: A/B in tools/gemm_nf_ab.py).  Same arithmetic per output either way.
    // The width does not touch the arithmetic, so a launch picks it on its OWN rows; the split-K factor of a batch-hinted launch is
    // the reference launch's, i.e. planned with the width the reference launch picks.
    auto choose_nf = [&](int rows) -> int {
        int nf_ = geglu ? 4 : (d.N % 160 == 0 ? 5 : 4);
        if (!geglu && nf_ == 5 && d.N % 128 == 0) {
            const int mt = (rows + 127) / 128;
            const int t5 = mt * (d.N / 160), t4 = mt * (d.N / 128);
            // (not where the launch would be split along K: the split factor is derived from the tile count, and 7 x 80 tiles spill
            //  into a second round where 7 x 64 do not -- B = 1 8x8-level convolutions: 45 -> 59 us, profiles/r03_gemm_nf_ab.txt)
            const bool would_split = t4 < 384 && ((t4 <= 128 && nk >= 32) || nk >= 72);
            const bool prefer4 = !would_split && ((t4 <= 256) || (t5 > 256 && (t5 + 511) / 512 == (t4 + 511) / 512));
            if (((flags & ANYV2V_GEMM_NF4) || prefer4) && !(flags & ANYV2V_GEMM_NF5)) nf_ = 4;
        }
        return nf_;
    };
    const bool big_ok = glds && !(flags & ANYV2V_GEMM_NO_BIG) && d.N % 320 == 0 && (!geglu || d.mode == MODE_LINEAR) &&
                        (geglu || d.act == ACT_NONE);
    // Launch plan as a function of the row count: kernel family (persistent 192 x 320 tiles / 128-row tiles) and split-K factor.
    //  * persistent kernel: taken when its tiles fill the 256 CUs for a whole number of rounds well enough (>= 75 %), or when
    //    forced (ANYV2V_GEMM_FORCE_BIG);
    //  * launches that cannot fill the CUs but have a long K loop (8x8-level convs / FF-down of the 3-clip batch, M = 3072): split K
    //    so that (tiles x splits) is one nearly full round of 256 work items; the ordered reduce pass finishes them.  Measured
    //    (profiles/r01_gemm_split_ab.txt): 1.2-1.4x over the 128-row kernel's split path from 80 K-tiles on with >= 224 work items;
    //    slower below 72 K-tiles or with a 3/4-full round (M = 1024), which stay on the 128-row kernel;
    //  * 128-row kernel split-K for launches that cannot fill the chip (512 block slots) and have a long K loop (with 20 K-tiles the
    //    second pass costs more than the idle CUs; with 60 it pays only when fewer than a quarter of the block slots would be busy;
    //    from ~72 K-tiles on it always pays).
    // (the workspace test uses the PLANNED row count as well: a batch-hinted launch must reproduce the decision of the launch it
    //  stands for -- its own, smaller partial tiles could fit where the reference launch's do not, and the two would then split
    //  differently: seen at 16 f x 256^2, tests/test_gpu_parity.py::test_two_branch_steps_bit_equal_at_a_mid_size_full_width)
    // (the split-K rules below see at most the 64 MiB the workspace had when they were tuned: a larger buffer -- the stream-K form
    //  wants 126 MB -- must not change which launches split, i.e. their arithmetic)
    const size_t split_ws_bytes = (size_t)d.workspace_bytes < ((size_t)64 << 20) ? (size_t)d.workspace_bytes : ((size_t)64 << 20);
    struct Choice { bool big; int splits; };
    auto choose = [&](int rows) -> Choice {
        const bool ws_buf = d.workspace != nullptr && d.N % 8 == 0;
        if (big_ok) {
            const int tb = ceil_div(rows, AV_GEMM_BM) * (d.N / 320);
            const int rounds = (tb + 255) / 256;
            const bool fills = tb >= 224 && tb * 4 >= rounds * 256 * 3;
            if (!fills && !geglu && !(flags & (ANYV2V_GEMM_NO_SPLITK | ANYV2V_GEMM_FORCE_BIG)) && ws_buf && tb <= 128 && nk >= 72) {
                int sp = 256 / tb;
                if (sp > 8) sp = 8;
                if (sp > nk / 12) sp = nk / 12;
                if (sp >= 2 && tb * sp >= 224 && (size_t)sp * rows * d.N * sizeof(float) <= split_ws_bytes) return {true, sp};
            }
            if (fills || (flags & ANYV2V_GEMM_FORCE_BIG)) return {true, 1};
        }
        const int tm = ((rows + 127) / 128) * ceil_div(d.N, choose_nf(rows) * 32);
        const bool split_pays = (tm <= 128 && nk >= 32) || nk >= 72;
        if (glds && !geglu && d.act != ACT_F32OUT && !(flags & ANYV2V_GEMM_NO_SPLITK) && ws_buf && tm < 384 && split_pays) {
            int sp = (512 + tm - 1) / tm;
            if (sp > 8) sp = 8;
            if (sp > nk / 8) sp = nk / 8;
            if (sp >= 2 && (size_t)sp * rows * d.N * sizeof(float) <= split_ws_bytes) return {false, sp};
        }
        return {false, 1};
    };
    // Batch hint (anyv2v_set_batch_hint): what fixes the ARITHMETIC is the split-K factor (fp32 partial tiles summed afterwards);
    // the two kernel families accumulate every output element in the same order (tests/gpu_checks.py asserts it bit for bit).  A
    // hinted launch therefore takes the split factor of the launch it stands for and is otherwise planned on its own row count.
    Choice use = choose(d.M);
    if (hinted_rows != d.M) {
        const Choice ref = choose(hinted_rows);
        if (ref.splits > 1)
            use = ref;
        else if (use.splits > 1)
            use = Choice{false, 1};
    }
    p.splits = use.splits;
    // Ping-pong kernel (gemm_pp_kernel), by default on the taller tile unless it quantises worse onto the 256 CUs.  Not split along K (the
    // launches that want that are too small for it), so a batch-hinted launch may only take it when its reference launch is unsplit too.
    // Measured (profiles/r04_gemm_pp_ab_v1_*.txt, interleaved A/B on the edit step's launches): its K loop is 2-6 % faster than
    // gemm_big_kernel's from K = 5760 on (conv 960->320 @64x64 898 -> 845 us, 1.21 -> 1.29 PF), equal at K = 2880, and its tile switch
    // costs more (residual launches 10-30 % slower; temporal convolutions, FF-down slower) -- the R slots, not the M slots, set the
    // slot time (9 LDS-DMA issues per wave and K-tile).  The launches it wins sum to 0.25 ms of the 106 ms step pair (+ 0.08 ms on
    // the inversion step's one-round launches, M = 65536 with 256-row tiles: conv 960->320 322 -> 298 us, r04_gemm_pp_ab_v1_b1_*.txt),
    // so it is never taken by default; a second form with the next tile's start-up hoisted in front of the tile-switch barrier was
    // slower throughout (r04_gemm_pp_ab_v2_*.txt, not kept).
    if (big_ok && !geglu && use.splits == 1 && !(flags & ANYV2V_GEMM_NO_PP) && (flags & ANYV2V_GEMM_PP)) {
        auto tiles_of = [&](int mf) { return ceil_div(d.M, 64 * mf) * (d.N / 320); };
        auto eff = [&](int mf) { return (double)tiles_of(mf) / (((tiles_of(mf) + 255) / 256) * 256.0); };
        p.pp_mf = (flags & ANYV2V_GEMM_PP_192) ? 3 : ((flags & ANYV2V_GEMM_PP_256) ? 4 : (eff(4) + 0.02 >= eff(3) ? 4 : 3));
        p.tilesN = d.N / 320;
        p.tiles = tiles_of(p.pp_mf);
        p.grid = p.tiles < 256 ? p.tiles : 256;
        return take(GEMM_PP, "the ping-pong kernel");
    }
    // GroupNorm records: both tile kernels emit them in their unsplit, fp16-output, non-GEGLU forms (LDS-DMA staging); a split-K plan
    // finishes in the reduce kernel, which has no tile to take them of.  Decided on `use`, i.e. under the batch hint, like the launch.
    if (use.splits > 1)
        p.gn_decline = "a split-K plan";
    else if (geglu || d.act == ACT_F32OUT || !glds || !gn_shape_ok(d))
        p.gn_decline = "a GEGLU / fp32-output / register-staged launch or a shape the record layout does not cover (N % 160 = 0, "
                       "N / gn_groups dividing 40, M and gn_rows_per_group multiples of 16)";
    else
        p.gn_records = true;
    if (use.big) {
        p.family = GEMM_BIG;
        persistent_grid(p, d);
        if (use.splits > 1)
            p.grid = p.tiles * use.splits < 256 ? p.tiles * use.splits : 256;
        else
            raster(p, d);
        return p;
    }
    // (with records: always the 160-column tile -- a channel group must not straddle the tile, and the width does not touch the
    //  arithmetic; the plan above, split-K factor included, is the one the launch without records gets)
    p.family = GEMM_MFMA128;
    p.nf = d.gn_stats != nullptr && p.gn_records ? 5 : choose_nf(d.M);
    p.tilesN = ceil_div(d.N, p.nf * 32);
    p.tiles = ((d.M + 127) / 128) * p.tilesN;
    p.grid = p.tiles * p.splits;
    return p;
}
