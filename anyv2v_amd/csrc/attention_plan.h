// Launch plan of the three attention entry points (anyv2v_attention_f16 / _small_f16 / _bias_f16): which kernel instantiation runs a
// descriptor, on which grid, with how much dynamic LDS.  A pure function of the descriptor, the entry point, head_dim and whether a
// bias was handed over (no HIP, no globals): plain C++17, built for the host alone by tests/test_attention_plan_host.py.
// attention.hip plans, then launches the instantiation the plan names.
#pragma once
#include <stddef.h>

#include "../../include/anyv2v_hip.h"   // (and stdint.h)

#define AV_PLAN_LOCAL __attribute__((visibility("hidden")))   // shared between the library's objects, never exported

enum AttnEntry { ATTN_ENTRY_D64 = 0, ATTN_ENTRY_SMALL = 1, ATTN_ENTRY_BIAS = 2 };   // anyv2v_attention_f16 / _small_f16 / _bias_f16

// one thread per query (attn_naive_kernel); one wave per sequence of <= 16 frames (short_attn_d64_kernel<STREAMS>); flash
// (flash_attn_d64_v2_kernel<STAGES, STREAMS, WAVES>); whole-sequence MFMA (small_attn_mfma_kernel<DS, NKB, BIAS>); 96-key loop
// (loop_attn_mfma_kernel<DS>)
enum AttnKernel { ATTN_NAIVE, ATTN_SHORT, ATTN_FLASH, ATTN_SMALL, ATTN_LOOP, ATTN_KERNEL_COUNT };

struct AttnPlan {
    int status;                  // ANYV2V_OK / ANYV2V_EINVAL (text: anyv2v_last_error())
    AttnKernel kernel;
    int stages, streams, waves;  // flash: LDS ring stages 2 | 3, V / O streams 1 | 3, waves per block 4 | 8; short: streams 1 | 3
    int ds, nkb;                 // small / loop: 32-column groups of a head (2..5), padded keys / 16 (6 | 18; loop: 6)
    bool bias;                   // small: the BIAS instantiation; naive: launched with the bias pointer
    int causal;                  // AttnK.causal of the launch
    int q_tiles;                 // AttnK.q_tiles: query tiles of 128 rows (8-wave flash: 256)
    unsigned grid_x, grid_y, grid_z;
    int block;                   // threads per block
    size_t lds_bytes;            // dynamic LDS (the flash and short kernels' LDS is static: 0)
    const char* wide_reason;     // anyv2v_attention_f16 left the flash kernels for the 64-bit ones: why; otherwise nullptr
};

void anyv2v_set_error(const char* fmt, ...);   // errors.hip (the planner test brings its own): the text behind a failed status

// head_dim is ignored (64) for ATTN_ENTRY_D64; has_bias = the bias pointer of ATTN_ENTRY_BIAS is not null.  A null descriptor fails
// where it failed in the entry points (after their head_dim / bias checks).
AV_PLAN_LOCAL AttnPlan av_attn_plan(const AnyV2VAttnDesc* d, AttnEntry entry, int head_dim, bool has_bias);
inline AttnPlan av_attn_plan(const AnyV2VAttnDesc& d, AttnEntry entry, int head_dim, bool has_bias) { return av_attn_plan(&d, entry, head_dim, has_bias); }

// "flash<2,1,4>", "short<3>", "small<4,18>", "small<2,6,bias>", "loop<5>", "naive", "naive+bias": the instantiation behind a plan
AV_PLAN_LOCAL const char* av_attn_kernel_name(const AttnPlan& p);
// Every instantiation av_attn_plan can emit (kernel and template arguments set, the rest zero): 0 <= i < av_attn_instantiation_count()
AV_PLAN_LOCAL int av_attn_instantiation_count();
AV_PLAN_LOCAL AttnPlan av_attn_instantiation(int i);
