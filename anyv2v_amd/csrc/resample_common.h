// Device helpers shared by the 8-bit resampling kernels (resample.hip) and the restore kernel built on their vertical pass (restore.hip):
// the fixed-point sample of include/anyv2v_hip.h and the unaligned-safe dword load.
#pragma once
#include "common.h"

#define RS_THREADS 256
#define RS_SHIFT 22
#define RS_HALF (1 << (RS_SHIFT - 1))

__device__ __forceinline__ int rs_mad(int acc, uint32_t sample, int k) { return __mul24((int)sample, k) + acc; }   // v_mad_i32_i24: |k| < 2^23
__device__ __forceinline__ uint32_t rs_finish(int acc) { return (uint32_t)min(max(acc >> RS_SHIFT, 0), 255); }

// four bytes at p, all inside [lo, hi)
__device__ __forceinline__ uint32_t rs_load4(const uint8_t* p, const uint8_t* lo, const uint8_t* hi) {
    const uint32_t a = (uint32_t)((uintptr_t)p & 3);
    if (a == 0) return *(const uint32_t*)p;
    const uint8_t* q = p - a;
    if (q >= lo && q + 8 <= hi) {
        const uint32_t* d = (const uint32_t*)q;
        return __builtin_amdgcn_alignbyte(d[1], d[0], a);
    }
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24);
}
