// The per-sequence arithmetic of short-sequence attention (S <= 16, head_dim 64), shared by short_attn_d64_kernel (attention.hip)
// and the fused temporal QKV + attention kernel (tattn_fused.hip): both call these, so a sequence's output has the same bits
// whichever of them computes it.  One wave per sequence; lane (l15 = l & 15, g = l >> 4).
#pragma once
#include "common.h"

typedef __fp16 fp16x4_t __attribute__((__vector_size__(8)));

// S^T = K Q^T by 2 x v_mfma_f32_16x16x32_f16 (fragments: lane (row = l15, k-chunk g): 8 halves at column 8 g + 32 ks), D[key = 4 g + r]
// [q = l15]; softmax over the keys: in-lane + 2 shuffles.  Returns the un-normalised probabilities as the P^T B-operand of the PV
// MFMAs and 1 / row sum.
__device__ __forceinline__ void short_attn_softmax(const h8 (&kf)[2], const h8 (&qf)[2], int g, int Sk, float c, h4& pf, float& inv) {
    f4 s = {0.f, 0.f, 0.f, 0.f};
    s = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[0], qf[0], s, 0, 0, 0);
    s = __builtin_amdgcn_mfma_f32_16x16x32_f16(kf[1], qf[1], s, 0, 0, 0);
    float mx = -1e30f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (4 * g + r >= Sk) s[r] = -1e30f;
        mx = fmaxf(mx, s[r]);
    }
    mx = fmaxf(mx, __shfl_xor(mx, 16, 64));
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    float sum = 0.f;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const float e = exp2f((s[r] - mx) * c);
        sum += e;
        pf[r] = (half_t)e;
    }
    sum += __shfl_xor(sum, 16, 64);
    sum += __shfl_xor(sum, 32, 64);
    inv = 1.0f / sum;
}

// O^T[d][q] = sum_key V^T[d][key] P^T[key][q] by 4 x v_mfma_f32_16x16x16_f16; the V^T fragments come from the row-major LDS image
// `vs` [16 keys][64 d] through ds_read_b64_tr_b16 (lane i of a 16-lane group supplies &V[4g + (i>>2)][d0 + 4(i&3)] and receives
// V[4g + 0..3][d0 + i]).  The MFMA leaves lane (q = l15, g) with 4 of every 16 output channels: stored directly that is 32-byte
// pieces of 16 different rows per instruction.  The tile is turned through LDS (`ow`, row stride 144 bytes) so that 8 lanes write
// one full 128-byte row segment.
__device__ __forceinline__ void short_attn_pv(const half_t* vs, half_t* ow, const h4& pf, float inv, int l15, int g) {
#pragma unroll
    for (int db = 0; db < 4; ++db) {
        const half_t* src = &vs[(4 * g + (l15 >> 2)) * 64 + 16 * db + 4 * (l15 & 3)];
        const fp16x4_t vt = __builtin_amdgcn_ds_read_tr16_b64_v4f16((__attribute__((address_space(3))) fp16x4_t*)src);
        h4 vf;
#pragma unroll
        for (int j = 0; j < 4; ++j) vf[j] = (half_t)vt[j];
        f4 o = {0.f, 0.f, 0.f, 0.f};
        o = __builtin_amdgcn_mfma_f32_16x16x16f16(vf, pf, o, 0, 0, 0);
        h4 ov;
#pragma unroll
        for (int r = 0; r < 4; ++r) ov[r] = (half_t)(o[r] * inv);
        *(h4*)(ow + l15 * 72 + 16 * db + 4 * g) = ov;
    }
}
