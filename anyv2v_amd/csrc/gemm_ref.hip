// The two plain kernels of the gather-GEMM (no MFMA, no LDS): gemm_naive_kernel, one thread per output element for any shape, and
// gemm_splitk_reduce_kernel, the second pass of the split-K launches of gemm_mfma_kernel / gemm_big_kernel.
//
// Replaces (reference = TIGER-AI-Lab/AnyV2V): the Linear / Conv2d / Conv3d layers of the diffusers-0.26.3 I2VGenXLUNet behind
// pipeline_i2vgen_xl.py:1146 whose shapes the tile kernels do not take (channel counts that are no multiple of 64).
#include "gemm_common.h"

// ---------------------------------------------------------------------------------------------------------
// Reference-grade kernel: one thread per output element, any shape.  Used for the tiny once-per-clip
// conditioning layers (Cin = 4/16/32 ...) and as the on-device cross-check of the MFMA kernels in the tests.
template <int MODE>
__global__ void gemm_naive_kernel(const GemmK p) {
    const bool geglu = p.act == ACT_GEGLU;
    const int Nout = geglu ? p.N / 2 : p.N;
    const long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (long long)p.M * Nout) return;
    const int m = (int)(idx / Nout), j = (int)(idx - (long long)m * Nout);
    const int n = geglu ? 32 * (j / 16) + (j % 16) : j;
    const RowInfo ri = make_row<MODE>(p, m);
    const int K = p.C0 + p.C1;
    float a0 = 0.f, a1 = 0.f;
    for (int tap = 0; tap < p.taps; ++tap) {
        const int sr = src_row<MODE>(p, ri, tap);
        if (sr < 0) continue;
        const half_t* w0 = p.W + (size_t)n * p.Ktot + (size_t)tap * K;
        const half_t* w1 = w0 + (size_t)16 * p.Ktot;
        const half_t* x0 = p.A0 + (size_t)sr * p.lda0;
        for (int k = 0; k < p.C0; ++k) {
            const float x = (float)x0[k];
            a0 += x * (float)w0[k];
            if (geglu) a1 += x * (float)w1[k];
        }
        if (p.C1 > 0) {
            const half_t* x1 = p.A1 + (size_t)sr * p.lda1;
            for (int k = 0; k < p.C1; ++k) {
                const float x = (float)x1[k];
                a0 += x * (float)w0[p.C0 + k];
                if (geglu) a1 += x * (float)w1[p.C0 + k];
            }
        }
    }
    float v;
    if (geglu) {
        if (p.bias != nullptr) {
            a0 += (float)p.bias[n];
            a1 += (float)p.bias[n + 16];
        }
        v = a0 * av_gelu(a1);
    } else {
        v = a0;
        if (p.bias != nullptr) v += (float)p.bias[n];
        if (p.rowvec != nullptr) v += (float)p.rowvec[(size_t)(m / p.rowvec_div) * p.ldrv + n];
        if (p.act == ACT_SILU)
            v = av_silu(v);
        else if (p.act == ACT_GELU)
            v = av_gelu(v);
    }
    if (p.act == ACT_F32OUT) {
        ((float*)p.C)[(size_t)m * p.ldc + j] = v;
        return;
    }
    if (p.R != nullptr) v = (float)(half_t)v + (float)p.R[(size_t)m * p.ldr + j];
    p.C[(size_t)m * p.ldc + j] = (half_t)v;
}

// split-K second pass: sum the fp32 partial tiles in a fixed order (deterministic), then the usual epilogue
__global__ void gemm_splitk_reduce_kernel(const GemmK p) {
    const int N8 = p.N >> 3;
    const long long total = (long long)p.M * N8;
    for (long long idx = (long long)blockIdx.x * blockDim.x + threadIdx.x; idx < total;
         idx += (long long)gridDim.x * blockDim.x) {
        const int m = (int)(idx / N8), n0 = (int)(idx - (long long)m * N8) * 8;
        float v[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = 0.f;
        for (int s = 0; s < p.splits; ++s) {
            const float* src = p.partial + ((size_t)s * p.M + m) * p.N + n0;
            const f4 a = *(const f4*)src, b = *(const f4*)(src + 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                v[e] += a[e];
                v[4 + e] += b[e];
            }
        }
        h8 o;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float x = v[e];
            if (p.bias != nullptr) x += (float)p.bias[n0 + e];
            if (p.rowvec != nullptr) x += (float)p.rowvec[(size_t)(m / p.rowvec_div) * p.ldrv + n0 + e];
            if (p.act == ACT_SILU)
                x = av_silu(x);
            else if (p.act == ACT_GELU)
                x = av_gelu(x);
            o[e] = (half_t)x;
        }
        if (p.R != nullptr) {
            const h8 rr = *(const h8*)(p.R + (size_t)m * p.ldr + n0);
#pragma unroll
            for (int e = 0; e < 8; ++e) o[e] = (half_t)((float)o[e] + (float)rr[e]);
        }
        *(h8*)(p.C + (size_t)m * p.ldc + n0) = o;
    }
}

// ---------------------------------------------------------------------------------------------------------
// host side (when either runs: gemm_plan.cpp)
int av_gemm_naive_launch(const GemmK& k, const AnyV2VGemmDesc* d, const GemmPlan& plan, hipStream_t s) {
    const dim3 grid((unsigned)plan.grid);
    if (d->mode == MODE_CONV2D)
        hipLaunchKernelGGL(gemm_naive_kernel<MODE_CONV2D>, grid, dim3(256), 0, s, k);
    else if (d->mode == MODE_TEMPORAL)
        hipLaunchKernelGGL(gemm_naive_kernel<MODE_TEMPORAL>, grid, dim3(256), 0, s, k);
    else
        hipLaunchKernelGGL(gemm_naive_kernel<MODE_LINEAR>, grid, dim3(256), 0, s, k);
    return av_launch_status("gemm_naive");
}

void av_gemm_splitk_reduce_launch(const GemmK& k, hipStream_t s) {
    const long long blocks = ((long long)k.M * (k.N / 8) + 255) / 256;   // (grid-stride loop: at most 2048 blocks)
    hipLaunchKernelGGL(gemm_splitk_reduce_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, k);
}
