// Sampler options of the I2VGen-XL step engines: guidance rescale (Lin et al., "Common Diffusion Noise Schedules and Sample Steps
// are Flawed", 3.4; reference consisti2v/consisti2v/pipelines/pipeline_video_editing.py:50-61) and stochastic DDIM (eta > 0;
// seine/diffusion/gaussian_diffusion.py:583-599), fused with the CFG combine and the token -> NCFHW layout change like
// cfg_ddim_step_kernel (elementwise.hip), which stays as it is and keeps serving the default path.
//   guidance_stats_kernel    sums of the text-branch prediction and of the guided prediction about a pivot, one record per block
//   cfg_ddim_step_ex_kernel  folds the records into the rescale factor, then CFG + rescale + DDIM update + sigma * noise
// No atomics and a fixed grid: the records, their fold and therefore the step are bit-reproducible on any device.
#include "common.h"

#define GS_BLOCKS ANYV2V_GUIDANCE_STATS_BLOCKS
#define GS_THREADS ANYV2V_GUIDANCE_STATS_THREADS
#define GS_RECORD ANYV2V_GUIDANCE_STATS_RECORD

// the guided prediction in the reference's fp16 arithmetic order: neg + g * (edit - neg), each operation rounded to fp16 -- the
// expression of cfg_ddim_step_kernel, so that both kernels (and both of this file) form the same value
__device__ __forceinline__ float cfg_guided(float v, float vu, float g) {
    const float diff = (float)(half_t)(v - vu);
    return (float)(half_t)(vu + (float)(half_t)(g * diff));
}

// Record b (GS_RECORD floats) = {S_txt, Q_txt, S_cfg, Q_cfg, K_txt, K_cfg, 0, 0}: S = sum(x - K), Q = sum((x - K)^2) over the
// pixels block b visits (grid-stride, all C channels of a pixel), K = the tensor's first element (pixel 0, channel 0).
__global__ __launch_bounds__(GS_THREADS) void guidance_stats_kernel(const half_t* __restrict__ V, int ldv, int b_unc, int b_cond,
                                                                    float g, float* __restrict__ rec, int C, int F, int HW) {
    __shared__ float red[GS_THREADS / WAVE][4];
    const long long npix = (long long)F * HW;
    const half_t* Vc = V + (long long)b_cond * npix * ldv;
    const half_t* Vu = V + (long long)b_unc * npix * ldv;
    const float kt = (float)Vc[0];
    const float kg = cfg_guided(kt, (float)Vu[0], g);
    float st = 0.f, qt = 0.f, sg = 0.f, qg = 0.f;
    for (long long p = (long long)blockIdx.x * GS_THREADS + threadIdx.x; p < npix; p += (long long)GS_BLOCKS * GS_THREADS) {
        const half_t* pc = Vc + p * ldv;
        const half_t* pu = Vu + p * ldv;
        for (int c = 0; c < C; ++c) {
            const float v = (float)pc[c];
            const float dt = v - kt, dg = cfg_guided(v, (float)pu[c], g) - kg;
            st += dt;
            qt += dt * dt;
            sg += dg;
            qg += dg * dg;
        }
    }
    st = wave_sum(st);
    qt = wave_sum(qt);
    sg = wave_sum(sg);
    qg = wave_sum(qg);
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x / WAVE;
    if (lane == 0) {
        red[w][0] = st;
        red[w][1] = qt;
        red[w][2] = sg;
        red[w][3] = qg;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        f4 s = {0.f, 0.f, 0.f, 0.f};
        for (int i = 0; i < GS_THREADS / WAVE; ++i)   // wave order: fixed
            for (int e = 0; e < 4; ++e) s[e] += red[i][e];
        const f4 k = {kt, kg, 0.f, 0.f};
        f4* out = (f4*)(rec + (size_t)blockIdx.x * GS_RECORD);
        out[0] = s;
        out[1] = k;
    }
}

// The rescale factor phi * std_txt / std_cfg + (1 - phi) from the records: folded in fp64 in record order, unbiased standard
// deviations (n - 1, torch.std), the factor itself in fp32.  Every thread of every block computes the same value.
__device__ __forceinline__ float rescale_factor(const float (*recs)[4], float phi, float n) {
    double st = 0.0, qt = 0.0, sg = 0.0, qg = 0.0;
    for (int b = 0; b < GS_BLOCKS; ++b) {
        st += (double)recs[b][0];
        qt += (double)recs[b][1];
        sg += (double)recs[b][2];
        qg += (double)recs[b][3];
    }
    const double dn = (double)n;
    const float std_t = (float)sqrt(fmax(qt - st * st / dn, 0.0) / (dn - 1.0));
    const float std_g = (float)sqrt(fmax(qg - sg * sg / dn, 0.0) / (dn - 1.0));
    return phi * (std_t / std_g) + (1.0f - phi);
}

// row: 8 floats on the device {sa_t, sb_t, c_x0, c_eps, sigma, phi, n, 0}, rewritten by the host before every step (one captured
// graph serves every timestep).  rec == nullptr or phi == 0 or b_unc < 0: no rescale.  noise == nullptr: no noise term.
__global__ __launch_bounds__(256) void cfg_ddim_step_ex_kernel(const half_t* __restrict__ V, int ldv, int b_unc, int b_cond, float g,
                                                               int pred, const float* __restrict__ row, const float* __restrict__ rec,
                                                               const half_t* __restrict__ noise, const half_t* __restrict__ lat,
                                                               half_t* __restrict__ out, int C, int F, int HW) {
    __shared__ float recs[GS_BLOCKS][4];
    const float sa_t = row[0], sb_t = row[1], c_x0 = row[2], c_eps = row[3], sigma = row[4], phi = row[5];
    const bool rescale = rec != nullptr && b_unc >= 0 && phi > 0.f;   // (uniform over the grid)
    float s = 1.0f;
    if (rescale) {
        for (int i = threadIdx.x; i < GS_BLOCKS; i += blockDim.x) {
            const f4 r = *(const f4*)(rec + (size_t)i * GS_RECORD);
            recs[i][0] = r[0];
            recs[i][1] = r[1];
            recs[i][2] = r[2];
            recs[i][3] = r[3];
        }
        __syncthreads();
        s = rescale_factor(recs, phi, row[6]);
    }
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= F * HW) return;
    const long long rc = ((long long)b_cond * F * HW + idx) * ldv;
    const long long ru = ((long long)(b_unc < 0 ? 0 : b_unc) * F * HW + idx) * ldv;
    const int f = idx / HW, p = idx - f * HW;
    for (int c = 0; c < C; ++c) {
        float v = (float)V[rc + c];
        if (b_unc >= 0) v = cfg_guided(v, (float)V[ru + c], g);
        if (rescale) v = (float)(half_t)(v * s);
        const long long li = ((long long)c * F + f) * HW + p;
        const float x = (float)lat[li];
        float y;
        {
            // every product and sum spelled out (no contraction left to the compiler): with phi = 0 and no noise the v-prediction
            // branch is, operation for operation, what cfg_ddim_step_kernel compiles to -- bit-equal results (tests/test_sampler_options_gpu.py)
#pragma clang fp contract(off)
            float x0, eps;
            if (pred == 0) {          // v_prediction
                x0 = __builtin_fmaf(sa_t, x, -(sb_t * v));
                eps = __builtin_fmaf(sb_t, x, sa_t * v);
            } else if (pred == 1) {   // epsilon
                x0 = (x - sb_t * v) / sa_t;
                eps = v;
            } else {                  // sample
                x0 = v;
                eps = (x - sa_t * v) / sb_t;
            }
            y = c_x0 * x0 + c_eps * eps;
            if (noise != nullptr) y = __builtin_fmaf(sigma, (float)noise[li], y);
        }
        out[li] = (half_t)y;   // the one rounding to fp16
    }
}

extern "C" int anyv2v_guidance_stats_f16(const void* Vtok, int32_t ldv, int32_t b_unc, int32_t b_cond, float guidance, float* records,
                                         int32_t C, int32_t F, int32_t HW, void* stream) {
    AV_CHECK(Vtok && records, "guidance_stats: null pointer");
    AV_CHECK(C > 0 && F > 0 && HW > 0 && ldv >= C && b_unc >= 0 && b_cond >= 0, "guidance_stats: bad arguments (the statistics are those of a guided prediction: b_unc >= 0)");
    AV_CHECK((long long)F * HW < (1ll << 31), "guidance_stats: F * HW must fit an int");
    AV_CHECK((long long)C * F * HW >= 2, "guidance_stats: a standard deviation needs n >= 2 elements");
    AV_CHECK(av_aligned16(records), "guidance_stats: the records must be 16-byte aligned");
    hipLaunchKernelGGL(guidance_stats_kernel, dim3(GS_BLOCKS), dim3(GS_THREADS), 0, (hipStream_t)stream, (const half_t*)Vtok, ldv, b_unc,
                       b_cond, guidance, records, C, F, HW);
    return av_launch_status("guidance_stats");
}

extern "C" int anyv2v_cfg_ddim_step_ex_f16(const void* Vtok, int32_t ldv, int32_t b_unc, int32_t b_cond, float guidance,
                                           int32_t prediction, const float* row, const float* records, float phi, const void* noise,
                                           const void* lat, void* out, int32_t C, int32_t F, int32_t HW, void* stream) {
    AV_CHECK(Vtok && row && lat && out, "cfg_ddim_step_ex: null pointer");
    AV_CHECK(C > 0 && F > 0 && HW > 0 && ldv >= C && b_cond >= 0 && prediction >= 0 && prediction <= 2, "cfg_ddim_step_ex: bad arguments");
    AV_CHECK((long long)F * HW < (1ll << 31), "cfg_ddim_step_ex: F * HW must fit an int (the kernel's pixel index)");
    AV_CHECK(phi >= 0.f && phi <= 1.f, "cfg_ddim_step_ex: phi must lie in [0, 1]");   // (false for NaN)
    const bool rescale = phi > 0.f && b_unc >= 0;   // without guidance the rescale is skipped (pipeline_video_editing.py:685)
    AV_CHECK(!rescale || records, "cfg_ddim_step_ex: null pointer (phi > 0 needs the records of anyv2v_guidance_stats_f16)");
    AV_CHECK(!rescale || (long long)C * F * HW >= 2, "cfg_ddim_step_ex: phi > 0 needs n >= 2 elements");
    AV_CHECK(!rescale || av_aligned16(records), "cfg_ddim_step_ex: the records must be 16-byte aligned");
    hipLaunchKernelGGL(cfg_ddim_step_ex_kernel, dim3((unsigned)(((long long)F * HW + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const half_t*)Vtok, ldv, b_unc, b_cond, guidance, prediction, row, rescale ? records : (const float*)nullptr,
                       (const half_t*)noise, (const half_t*)lat, (half_t*)out, C, F, HW);
    return av_launch_status("cfg_ddim_step_ex");
}
