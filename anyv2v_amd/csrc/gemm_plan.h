// Launch plan of anyv2v_gemm_f16: which kernel family runs a descriptor, at which tile width, split-K factor, grid and tile order.
// A pure function of the descriptor and the batch-hinted row count (no HIP, no globals): plain C++17, built for the host alone by
// tests/test_gemm_plan_host.py.  gemm.hip plans, then calls the launcher of the family the plan names; anyv2v_gemm_gn_stats_floats only plans.
#pragma once
#include <stddef.h>

#include "../../include/anyv2v_hip.h"   // (and stdint.h)

enum { MODE_LINEAR = 0, MODE_CONV2D = 1, MODE_TEMPORAL = 2 };
enum { ACT_NONE = 0, ACT_SILU = 1, ACT_GELU = 2, ACT_GEGLU = 3, ACT_F32OUT = 4 };

// naive; weight-stationary (gemm_ws.hip), plain and with the LayerNorm fold; 128-row tiles (gemm_mfma_kernel); persistent 192 x 320 tiles
// (gemm_big_kernel); ping-pong (gemm_pp_kernel); one wave per SIMD (gemm_sw.hip) and its stream-K form; LDS-patch 3x3 conv (gemm_swh.hip)
enum GemmFamily { GEMM_NAIVE, GEMM_WS, GEMM_WS_LN, GEMM_MFMA128, GEMM_BIG, GEMM_PP, GEMM_SW, GEMM_SW_STREAMK, GEMM_SWH, GEMM_FAMILY_COUNT };
const char* av_gemm_family_name(GemmFamily f);
void anyv2v_set_error(const char* fmt, ...);   // errors.hip (the planner test brings its own): the text behind a failed status

constexpr int AV_GEMM_BM = 192, AV_GEMM_BN = 320;   // block tile of the persistent kernels (big, one-wave, stream-K, LDS-patch)

struct GemmPlan {
    int status;              // ANYV2V_OK / ANYV2V_EINVAL / ANYV2V_EUNSUPPORTED (text: anyv2v_last_error())
    GemmFamily family;
    int taps, nk;            // filter taps; K-tiles of 64
    bool vec_epi;            // bias / rowvec may be read as 8-byte vectors
    int nf;                  // 128-row kernel: 32-column fragments per tile, 4 | 5
    int splits;              // split-K factor, 1 = none
    int tilesN, tiles, grid; // column tiles (weight-stationary: 160- / 128- / 64-column slabs), output tiles, blocks to launch
    int rast_gm, rast_gn, rast_sm, rast_sn, rast_nfast;   // tile order of the persistent kernels, all 0 = classic (GemmK)
    int pp_mf;               // ping-pong: 64-row fragments per tile, 3 | 4
    int sk_blocks;           // stream-K: blocks of the main launch
    bool gn_records;         // this launch can emit GroupNorm records (what anyv2v_gemm_gn_stats_floats answers)
    const char* gn_decline;  // if not: the plan that declined, for the error text of a launch with gn_stats set
};

// hinted_rows: av_hint_rows(d.M), the rows the heuristics see (anyv2v_set_batch_hint); grids and bounds use d.M.
GemmPlan av_gemm_plan(const AnyV2VGemmDesc& d, int hinted_rows);
