// FreeU (arXiv 2309.11497) on channels-last token matrices: the decoder's backbone / skip re-weighting in front of the channel
// concat of up_blocks[0] / up_blocks[1] (the reference forwards `enable_freeu` to its UNet, pipeline_i2vgen_xl.py:623-648).
//   backbone: hidden[:, : C / 2] *= b                                  (one fp16 rounding of float(x) * b; the other half is copied)
//   skip:     fftn over (H, W) -> fftshift -> the 2 x 2 box [H/2-1 : H/2+1, W/2-1 : W/2+1] times s -> ifftshift -> ifftn -> real
// The box holds the frequencies Kh x Kw, Kh = {0, -1} (H >= 2) or {0} (H == 1, where the slice wraps), Kw likewise, so the
// filter has a closed form and needs no FFT: with a = 2 pi h / H, b = 2 pi w / W and the seven sums over the plane
//   S0 = sum x,  Ch = sum x cos a,  Sh = sum x sin a,  Cw = sum x cos b,  Sw = sum x sin b,  Cc = sum x cos(a + b),  Sc = sum x sin(a + b)
//   y = x + (s - 1) / (H W) [ S0 + (Ch cos a + Sh sin a) + (Cw cos b + Sw sin b) + (Cc cos(a + b) + Sc sin(a + b)) ]
// (the a / b / a + b terms only where that axis has the frequency -1).  The box is NOT Hermitian-symmetric -- frequency (1, 0)
// is scaled through its partner (-1, 0) only, (1, -1) not at all; that is the definition, not an oversight.
// One block per (image, 64-channel slice): 8 channels (16 bytes) per lane, 32 row lanes striding over the H W rows; the sums are
// reduced across the row lanes by wave shuffles and across the four waves through LDS in a fixed order (no atomics: bit-reproducible,
// and independent of the batch around the image); a second sweep over the slab (<= 32 KB at 16 x 16, L2-hot) applies the correction in
// fp32 and rounds once.  The backbone scale rides in the same launch: further blocks along grid.y.
#include "common.h"

#include <math.h>

#define FU_THREADS 256
#define FU_ROWS (FU_THREADS / 8)   // row lanes of a block
#define FU_SLICE 64                // channels of a block
#define FU_WAVES (FU_THREADS / WAVE)
#define FU_MAX_HW_SUM 4096         // H + W: the cos / sin tables live in LDS

__global__ __launch_bounds__(FU_THREADS) void freeu_kernel(const half_t* __restrict__ Xh, int ldh, half_t* __restrict__ Yh, int ldho,
                                                           int Ch, float b, const half_t* __restrict__ Xs, int lds_,
                                                           half_t* __restrict__ Ys, int ldso, int Cs, float sm1, int H, int W,
                                                           int skip_slices) {
    extern __shared__ __attribute__((aligned(16))) float fu_lds[];
    const int img = blockIdx.x, tid = threadIdx.x;
    const int rl = tid >> 3, v = tid & 7;
    const int HW = H * W;
    if ((int)blockIdx.y >= skip_slices) {   // backbone: first half of the channels times b
        const int c0 = ((int)blockIdx.y - skip_slices) * FU_SLICE + v * 8;
        if (c0 >= Ch) return;
        const int half = Ch >> 1;
        const half_t* src = Xh + (size_t)img * HW * ldh + c0;
        half_t* dst = Yh + (size_t)img * HW * ldho + c0;
        for (int r = rl; r < HW; r += FU_ROWS) {
            h8 x = *(const h8*)(src + (size_t)r * ldh);
#pragma unroll
            for (int e = 0; e < 8; ++e)
                if (c0 + e < half) {
                    // the fp32 product, rounded, THEN the fp16 rounding -- what (x.float() * b).half() computes.  Left alone, hipcc
                    // fuses the multiply and the conversion into v_fma_mixlo_f16, which rounds the exact product once: a different
                    // fp16 value wherever the fp32 rounding lands on an fp16 tie
                    float p = (float)x[e] * b;
                    asm("" : "+v"(p));
                    x[e] = (half_t)p;
                }
            *(h8*)(dst + (size_t)r * ldho) = x;
        }
        return;
    }
    float* cH = fu_lds;                      // cos / sin of 2 pi h / H and 2 pi w / W
    float* sH = cH + H;
    float* cW = sH + H;
    float* sW = cW + W;
    float* red = sW + W;                     // [FU_WAVES][7][FU_SLICE]
    float* tot = red + FU_WAVES * 7 * FU_SLICE;   // [7][FU_SLICE]
    for (int i = tid; i < H; i += FU_THREADS) sincospif((float)(2 * i) / (float)H, &sH[i], &cH[i]);
    for (int i = tid; i < W; i += FU_THREADS) sincospif((float)(2 * i) / (float)W, &sW[i], &cW[i]);
    const int c0 = (int)blockIdx.y * FU_SLICE + v * 8;
    const bool active = c0 < Cs;             // (a last slice of fewer than 64 channels: the lane only takes part in the reduction)
    const half_t* src = Xs + (size_t)img * HW * lds_ + c0;
    half_t* dst = Ys + (size_t)img * HW * ldso + c0;
    float acc[7][8];
#pragma unroll
    for (int q = 0; q < 7; ++q)
#pragma unroll
        for (int e = 0; e < 8; ++e) acc[q][e] = 0.f;
    __syncthreads();
    if (active) {
#pragma unroll 4
        for (int r = rl; r < HW; r += FU_ROWS) {
            const h8 x = *(const h8*)(src + (size_t)r * lds_);
            const int h = r / W, w = r - h * W;
            const float ca = cH[h], sa = sH[h], cb = cW[w], sb = sW[w];
            const float cab = ca * cb - sa * sb, sab = sa * cb + ca * sb;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float f = (float)x[e];
                acc[0][e] += f;
                acc[1][e] += f * ca;
                acc[2][e] += f * sa;
                acc[3][e] += f * cb;
                acc[4][e] += f * sb;
                acc[5][e] += f * cab;
                acc[6][e] += f * sab;
            }
        }
    }
    // row lanes of a wave (lane = 8 row lanes x 8 channel lanes): xor shuffles, every lane ends with the same sum
    const int wave = tid / WAVE, lane = tid % WAVE;
#pragma unroll
    for (int q = 0; q < 7; ++q)
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float a = acc[q][e];
            a += __shfl_xor(a, 8, 64);
            a += __shfl_xor(a, 16, 64);
            a += __shfl_xor(a, 32, 64);
            if (lane < 8) red[(wave * 7 + q) * FU_SLICE + v * 8 + e] = a;
        }
    __syncthreads();
    for (int i = tid; i < 7 * FU_SLICE; i += FU_THREADS) {
        float a = red[i];
#pragma unroll
        for (int k = 1; k < FU_WAVES; ++k) a += red[k * 7 * FU_SLICE + i];
        tot[i] = a;
    }
    __syncthreads();
    if (!active) return;
    // (s - 1) / (H W) times the sums; an axis of size 1 has no frequency -1: its terms (and the mixed one) drop out
    const float scale = sm1 / (float)HW;
    const float fh = H >= 2 ? scale : 0.f, fw = W >= 2 ? scale : 0.f, fhw = (H >= 2 && W >= 2) ? scale : 0.f;
    float t[7][8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const int c = v * 8 + e;
        t[0][e] = tot[0 * FU_SLICE + c] * scale;
        t[1][e] = tot[1 * FU_SLICE + c] * fh;
        t[2][e] = tot[2 * FU_SLICE + c] * fh;
        t[3][e] = tot[3 * FU_SLICE + c] * fw;
        t[4][e] = tot[4 * FU_SLICE + c] * fw;
        t[5][e] = tot[5 * FU_SLICE + c] * fhw;
        t[6][e] = tot[6 * FU_SLICE + c] * fhw;
    }
#pragma unroll 4
    for (int r = rl; r < HW; r += FU_ROWS) {
        const h8 x = *(const h8*)(src + (size_t)r * lds_);
        const int h = r / W, w = r - h * W;
        const float ca = cH[h], sa = sH[h], cb = cW[w], sb = sW[w];
        const float cab = ca * cb - sa * sb, sab = sa * cb + ca * sb;
        h8 y;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float d = t[0][e];
            d += t[1][e] * ca + t[2][e] * sa;
            d += t[3][e] * cb + t[4][e] * sb;
            d += t[5][e] * cab + t[6][e] * sab;
            y[e] = (half_t)((float)x[e] + d);
        }
        *(h8*)(dst + (size_t)r * ldso) = y;
    }
}

extern "C" int anyv2v_freeu_f16(const void* hidden, int32_t ld_hidden, void* hidden_out, int32_t ld_hidden_out, int32_t C_hidden,
                                float b, const void* skip, int32_t ld_skip, void* skip_out, int32_t ld_skip_out, int32_t C_skip,
                                float s, int32_t n_img, int32_t H, int32_t W, void* stream) {
    AV_CHECK(hidden && hidden_out && skip && skip_out, "freeu: null pointer");
    AV_CHECK(n_img >= 1 && H >= 1 && W >= 1, "freeu: n_img = %d, H = %d, W = %d must all be >= 1", n_img, H, W);
    AV_CHECK((int64_t)H + W <= FU_MAX_HW_SUM, "freeu: H = %d, W = %d: H + W > %d (the cos / sin tables live in LDS)", H, W, FU_MAX_HW_SUM);
    AV_CHECK(C_hidden >= 8 && C_hidden % 8 == 0 && C_skip >= 8 && C_skip % 8 == 0,
             "freeu: C_hidden = %d, C_skip = %d must be positive multiples of 8", C_hidden, C_skip);
    AV_CHECK(ld_hidden >= C_hidden && ld_hidden_out >= C_hidden && ld_skip >= C_skip && ld_skip_out >= C_skip,
             "freeu: a leading dimension is smaller than its channel count");
    AV_CHECK(ld_hidden % 8 == 0 && ld_hidden_out % 8 == 0 && ld_skip % 8 == 0 && ld_skip_out % 8 == 0 && av_aligned16(hidden) &&
                 av_aligned16(hidden_out) && av_aligned16(skip) && av_aligned16(skip_out),
             "freeu: rows must be 16-byte aligned");
    AV_CHECK(isfinite(b) && isfinite(s), "freeu: b and s must be finite");
    AV_CHECK(hidden != hidden_out && skip != skip_out, "freeu: out of place only");
    const int skip_slices = (C_skip + FU_SLICE - 1) / FU_SLICE, hidden_slices = (C_hidden + FU_SLICE - 1) / FU_SLICE;
    AV_CHECK(skip_slices + hidden_slices <= 65535, "freeu: too many channels");
    const size_t lds_bytes = (size_t)(2 * H + 2 * W + (FU_WAVES + 1) * 7 * FU_SLICE) * sizeof(float);
    hipLaunchKernelGGL(freeu_kernel, dim3((unsigned)n_img, (unsigned)(skip_slices + hidden_slices)), dim3(FU_THREADS), lds_bytes,
                       (hipStream_t)stream, (const half_t*)hidden, ld_hidden, (half_t*)hidden_out, ld_hidden_out, C_hidden, b,
                       (const half_t*)skip, ld_skip, (half_t*)skip_out, ld_skip_out, C_skip, s - 1.0f, H, W, skip_slices);
    return av_launch_status("freeu");
}
