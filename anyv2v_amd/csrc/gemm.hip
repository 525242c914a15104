// Gather-GEMM for gfx950, host entry: Linear / 1x1 conv, implicit-GEMM conv2d 3x3 (stride 1|2, optional folded nearest x2
// upsample) and the temporal (3,1,1) conv, all over channels-last token matrices, fp16 in / fp32 MFMA
// accumulate / fp16 out, with the bias / temb-broadcast / SiLU / GELU / GEGLU / residual epilogues fused.
//
// anyv2v_gemm_f16 plans (gemm_plan.cpp decides everything), fills the kernel arguments and hands them to the launcher of the family
// the plan names.  The kernels, one translation unit per family (what each replaces in the reference is said there):
//   gemm_mfma.hip  gemm_mfma_kernel  : 128 x NF*32 x 64, 4 waves 2x2, 2 LDS stages (register- or LDS-DMA-staged), 2 blocks/CU.
//   gemm_big.hip   gemm_big_kernel   : 192 x 320 x 64, 8 waves 4x2 (wave tile 48 x 160), 2 LDS stages by LDS-DMA, persistent
//                                      blocks with cross-tile prefetch and a wave-private epilogue -- the large-M workhorse.
//   gemm_pp.hip    gemm_pp_kernel    : its ping-pong form (opt-in).
//   gemm_ref.hip   gemm_naive_kernel, gemm_splitk_reduce_kernel : one thread per output; the second pass of split-K launches.
//   gemm_ws.hip, gemm_sw.hip, gemm_swh.hip : weight-stationary, one-wave-per-SIMD and LDS-patch convolution kernels.
#include <stdlib.h>

#include "gemm_common.h"

__device__ __attribute__((aligned(256))) half_t g_zero_line[128];  // 256 B of zeros: source for padded taps

static const half_t* zero_line() {
    static const half_t* z = nullptr;
    if (z == nullptr) {
        void* ptr = nullptr;
        if (hipGetSymbolAddress(&ptr, HIP_SYMBOL(g_zero_line)) == hipSuccess) z = (const half_t*)ptr;
    }
    return z;
}

static int64_t g_gn_launches = 0;   // launches that emitted records (anyv2v_gemm_gn_launches); host-side, like the batch hint

extern "C" int anyv2v_gemm_f16(const AnyV2VGemmDesc* d, void* stream) {
    AV_CHECK(d != nullptr, "gemm: null descriptor");
    AV_CHECK(d->A0 && d->W && d->C, "gemm: null A0/W/C");
    const int hinted = av_hint_rows(d->M);
    const GemmPlan plan = av_gemm_plan(*d, hinted);
    // (in front of the plan's own status and over its text: a LayerNorm-fold launch with gn_stats set hears about gn_stats first)
    AV_CHECK(d->gn_stats == nullptr || plan.gn_decline == nullptr,
             "gemm: gn_stats set, but this launch runs on %s, which writes no GroupNorm statistics (ask anyv2v_gemm_gn_stats_floats first)",
             plan.gn_decline);
    if (plan.status != ANYV2V_OK) return plan.status;
    // the kernels hold SOURCE row numbers in int (RowInfo / src_row): a stride-2 convolution reads up to four times M rows
    AV_CHECK(d->mode != MODE_CONV2D || (long long)(d->M / (d->Ho * d->Wo)) * d->Hi * d->Wi < (1ll << 31),
             "gemm: the convolution's source has 2^31 rows or more");
    GemmK k = {};   // (trace, gn_* and what the plan leaves 0 stay off)
    k.A0 = (const half_t*)d->A0;
    k.A1 = d->C1 > 0 ? (const half_t*)d->A1 : (const half_t*)d->A0;
    k.W = (const half_t*)d->W;
    k.C = (half_t*)d->C;
    k.bias = (const half_t*)d->bias;
    k.rowvec = (const half_t*)d->rowvec;
    k.R = (const half_t*)d->R;
    k.zeros = zero_line();
    AV_CHECK(k.zeros != nullptr, "gemm: zero line symbol unavailable");
    k.M = d->M; k.N = d->N; k.C0 = d->C0; k.C1 = d->C1;
    k.lda0 = d->lda0; k.lda1 = d->C1 > 0 ? d->lda1 : d->lda0; k.ldc = d->ldc; k.ldr = d->ldr; k.ldrv = d->ldrv;
    k.rowvec_div = d->rowvec_div > 0 ? d->rowvec_div : 1;
    k.mode = d->mode; k.Hi = d->Hi; k.Wi = d->Wi; k.Ho = d->Ho; k.Wo = d->Wo; k.stride = d->stride; k.up = d->up;
    k.F = d->F; k.HW = d->HW; k.act = d->act;
    k.pad_lo = d->asym ? 0 : 1;
    k.taps = plan.taps; k.Ktot = k.taps * (d->C0 + d->C1); k.nt0 = d->C0 / 64; k.nt1 = d->C1 / 64;
    k.tilesN = plan.tilesN; k.vec_epi = plan.vec_epi; k.splits = plan.splits;
    if (plan.splits > 1 || plan.family == GEMM_SW_STREAMK) k.partial = (float*)d->workspace;
    if (plan.family == GEMM_WS_LN) k.ln_c1 = d->ln_c1, k.ln_eps = d->ln_eps;
    k.rast_gm = plan.rast_gm; k.rast_gn = plan.rast_gn; k.rast_sm = plan.rast_sm; k.rast_sn = plan.rast_sn; k.rast_nfast = plan.rast_nfast;
    if (d->gn_stats != nullptr) {   // (plan.gn_records holds: checked above)
        AV_CHECK(d->gn_stats_floats >= (int64_t)3 * (d->M / 16) * d->gn_groups, "gemm: gn_stats holds %lld floats, the launch writes %lld",
                 (long long)d->gn_stats_floats, (long long)3 * (d->M / 16) * d->gn_groups);
        AV_CHECK((((uintptr_t)d->gn_stats) & 3) == 0, "gemm: gn_stats must be 4-byte aligned");
        k.gn_stats = d->gn_stats;
        k.gn_groups = d->gn_groups;
        k.gn_cg = d->N / d->gn_groups;
        ++g_gn_launches;
    }
    // ANYV2V_GEMM_LOG=1: one line per launch plan on stderr (diagnostics: which launches split, and how, under a batch hint)
    static const bool log_on = getenv("ANYV2V_GEMM_LOG") != nullptr;
    if (log_on)
        fprintf(stderr, "gemm-plan mode %d M %d (hinted %d) N %d K %d act %d res %d big %d splits %d kernel %s nf %d grid %d\n", d->mode, d->M,
                hinted, d->N, k.Ktot, d->act, d->R != nullptr, plan.family == GEMM_BIG, plan.splits, av_gemm_family_name(plan.family),
                plan.nf, plan.grid);
    hipStream_t s = (hipStream_t)stream;
    // One arm per kernel family; its launcher only picks the template instantiation.  Tiles, grid, split-K factor and tile order are in k / plan.
    switch (plan.family) {
    case GEMM_WS:
    case GEMM_WS_LN: return av_gemm_ws_launch(k, d, plan, s);
    case GEMM_SW: return av_gemm_sw_launch(k, d, plan, s);
    case GEMM_SW_STREAMK: return av_gemm_sw_sk_launch(k, d, plan, s);
    case GEMM_SWH: return av_gemm_swh_launch(k, d, plan, s);
    case GEMM_NAIVE: return av_gemm_naive_launch(k, d, plan, s);
    case GEMM_PP: return av_gemm_pp_launch(k, d, plan, s);
    case GEMM_BIG: return av_gemm_big_launch(k, d, plan, s);
    default: return av_gemm_mfma_launch(k, d, plan, s);   // GEMM_MFMA128
    }
}

extern "C" int64_t anyv2v_gemm_gn_stats_floats(const AnyV2VGemmDesc* d) {
    if (d == nullptr) return 0;
    const GemmPlan plan = av_gemm_plan(*d, av_hint_rows(d->M));   // plans only: touches no device
    return plan.status == ANYV2V_OK && plan.gn_records ? (int64_t)3 * (d->M / 16) * d->gn_groups : 0;
}

extern "C" int64_t anyv2v_gemm_gn_launches(int32_t reset) {
    const int64_t n = g_gn_launches;
    if (reset) g_gn_launches = 0;
    return n;
}
