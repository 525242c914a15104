// What the two one-wave-per-SIMD kernels share (gemm_sw.hip, gemm_swh.hip): the block tile and the W-row permutation behind their
// direct 16-byte stores.
#pragma once
#include "gemm_common.h"

constexpr int SW_MF = 6;               // 16-row fragments per wave (6: 96 rows, two wave rows -> 192-row block tile)
constexpr int SW_BM = 32 * SW_MF, SW_BN = 320;
constexpr int SW_B_BYTES = SW_BN * 128;   // W of one K-tile (64 deep): 40 KiB
static_assert(SW_BM == AV_GEMM_BM && SW_BN == AV_GEMM_BN, "the plan counts tiles of this size");

// W row (relative to the wave slab's first row) that LDS row `s + 32 * piece` of the slab holds, as  row = wrow_thread(s) + wrow_piece(piece):
//  plain : LDS rows of a fragment pair (32 rows) hold W rows 8 (i / 4) + 4 f + i % 4  (f = fragment of the pair, i = row in it)
//  GEGLU : W comes as 32-row blocks [16 h | 16 gate]; two blocks form a 64-row group [hA gA hB gB] whose A / B fragments interleave
//          4-channel runs the same way; the fifth block of the slab stays in natural order (its outputs leave as 8-byte stores)
template <bool GEGLU>
__device__ __forceinline__ int sw_wrow_thread(int s) {
    const int i = s & 15, f = s >> 4;
    if constexpr (GEGLU)
        return 32 * (i >> 3) + 16 * f + 8 * ((i >> 2) & 1) + (i & 3);
    else
        return 8 * (i >> 2) + 4 * f + (i & 3);
}
template <bool GEGLU>
__device__ __forceinline__ constexpr int sw_wrow_piece(int pl) {   // pl: piece within the wave slab, 0..4
    if constexpr (GEGLU)
        return pl < 4 ? 64 * (pl >> 1) + 4 * (pl & 1) : 128;
    else
        return 32 * pl;
}
