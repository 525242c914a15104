// Launch plan of the fused temporal QKV + attention kernel (tattn_fused.hip): what it covers, where it pays, and how the
// (head, strip range) pairs are dealt to the blocks.  Plain C++ (tests/test_tattn_fused_host.py builds tattn_plan.cpp with the host
// compiler); the one inline function below is also what the kernel calls, so the test walks the very ranges the blocks walk.
#pragma once
#include <stdint.h>

#if defined(__HIP__)   // compiled as HIP (the library's build, also for the host-only tattn_plan.cpp)
#define AV_TATTN_HD __attribute__((host)) __attribute__((device)) inline __attribute__((always_inline))
#else
#define AV_TATTN_HD inline
#endif

constexpr int TATTN_C = 320;          // channels = heads x head_dim
constexpr int TATTN_HEADS = 5;
constexpr int TATTN_F = 16;           // frames = sequence length = one MFMA row block
#ifndef TATTN_WAVES_PER_BLOCK
#define TATTN_WAVES_PER_BLOCK 8
#endif
constexpr int TATTN_WAVES = TATTN_WAVES_PER_BLOCK;   // waves per block
constexpr int TATTN_SLAB_ROWS = 192;  // a head's 64 Q + 64 K + 64 V rows of W'
constexpr int TATTN_W_BYTES = TATTN_SLAB_ROWS * TATTN_C * 2;
constexpr int TATTN_BIAS_BYTES = TATTN_SLAB_ROWS * 2 + TATTN_SLAB_ROWS * 4;   // b' (fp16) and c1 (fp32) of the slab
// wave-private patch: first the Q | K tile [16 tokens][128 + 8 halves], then -- in the same bytes -- V [16][64] and the output
// tile [16][72]
constexpr int TATTN_QK_LD = 136;
constexpr int TATTN_PATCH_BYTES = 16 * TATTN_QK_LD * 2;
constexpr int TATTN_LDS_BYTES = TATTN_W_BYTES + TATTN_BIAS_BYTES + TATTN_WAVES * TATTN_PATCH_BYTES;
constexpr int TATTN_LDS_LIMIT = 160 * 1024;
constexpr int TATTN_MIN_ROWS = 32768;   // rows of ONE branch from which the LayerNorm-folded weight-stationary GEMM is taken (gemm_plan.cpp)
static_assert(16 * 64 * 2 + 16 * 72 * 2 <= TATTN_PATCH_BYTES, "V and output tiles reuse the Q | K patch");
static_assert(TATTN_LDS_BYTES <= TATTN_LDS_LIMIT, "W slab + patches must fit in LDS");

struct TattnPlan {
    int supported;   // the kernel computes this shape (F = 16, C = 320, 5 heads of 64, HW even)
    int pays;        // ... and one branch has the rows from which the two launches it replaces take the weight-stationary path
    int nstrips;     // 32-row strips: 2 pixels x 16 frames each
    int px;          // strip ranges per XCD
    int spr;         // strips per range
    int grid;        // 8 XCDs x px ranges x heads blocks
    int lds_bytes;
};

// rows_per_branch = F * HW (one batch element's rows), B = batch elements in the launch
TattnPlan av_tattn_plan(int64_t rows_per_branch, int B, int C, int heads, int F, int HW);

// block -> (head, [begin, end) of its strips).  The heads of one range sit on the same XCD (block % 8: observed placement, speed
// only) and start together, so a strip's rows come from HBM once and from that XCD's L2 for the other heads.
AV_TATTN_HD void av_tattn_block(const TattnPlan& p, int block, int heads, int* head, int* begin, int* end) {
    const int xcd = block & 7, idx = block >> 3;
    *head = idx % heads;
    const int range = xcd * p.px + idx / heads;
    const long long b = (long long)range * p.spr;
    const long long e = b + p.spr;
    *begin = (int)(b < p.nstrips ? b : p.nstrips);
    *end = (int)(e < p.nstrips ? e : p.nstrips);
}
