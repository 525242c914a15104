// GroupNorm (+SiLU) and LayerNorm over channels-last token matrices (HBM-bound kernels, 16-byte vector access).
//
// GroupNorm replaces diffusers GroupNorm(32) as used by ResnetBlock2D.norm1/norm2 (reference restatement
// i2vgen-xl/pnp_utils.py:48,104), Transformer2DModel.norm, TemporalConvLayer / TransformerTemporalModel.norm
// (5-D: statistics over all frames of a clip) and conv_norm_out.  The input may be the channel concat [X0 | X1]
// (skip connection of the up blocks, consisti2v/.../videoldm_unet_blocks.py:721-745) without materialising it.
// Two kernels, no atomics (bit-reproducible): (1) partial sums per (stat group, row chunk, channel group) reduced
// through LDS; (2) normalise + affine (+ SiLU) -> fp16, each block first folding the chunk sums of its stat group into
// (mean, rstd) in a fixed order (a separate 7-us finalize launch per GroupNorm used to cost 2 % of the step; a
// last-arriver finalize would need device-scope fences, which flush the per-XCD L2 on gfx950).
// Algorithmic traffic: 2 reads + 1 write of X.
// The sums are shifted: s = sum(x - K), q = sum((x - K)^2) about one pivot K per (stat group, channel group), the fp16 value at
// the group's first row and first channel; mean = K + s/n, var = q/n - (s/n)^2.  Unshifted one-pass sums cancel catastrophically
// once a group's mean is large against its spread (|mean| = 1000 sigma or near-constant groups: errors of 1e-1); about a member of
// the group, s/n is of the order of the spread.  The shift keeps the sums additive over chunks (and over ranks, for the pivoted
// sharded entry points, which agree on one pivot first).  The ABI-101 sharded pair (anyv2v_groupnorm_partial_f16 / _apply_f16)
// keeps its one-all-reduce contract and therefore the rank-independent pivot K = 0: unshifted sums, as before.
#include "common.h"
#include "norm_plan.h"

// pivot of (stat group sg, channel group g): the caller's agreed value, x[first row of sg][first channel of g] (pivot == nullptr,
// from_data) or 0 (pivot == nullptr, !from_data: the unshifted sums of the one-all-reduce sharded pair)
__device__ __forceinline__ float gn_pivot(const half_t* X0, const half_t* X1, int C0, int C1, const float* pivot, int from_data,
                                          int sg, int rows_per_group, int G, int g) {
    if (pivot) return pivot[(size_t)sg * G + g];
    if (!from_data) return 0.f;
    const int c = g * ((C0 + C1) / G);
    return c < C0 ? (float)X0[(size_t)sg * rows_per_group * C0 + c] : (float)X1[(size_t)sg * rows_per_group * C1 + (c - C0)];
}

// sharded entry points: pivot[sg][g] = this rank's pivot / shards (all-reduced by the caller into the agreed pivot)
__global__ void gn_pivot_kernel(const half_t* __restrict__ X0, const half_t* __restrict__ X1, int C0, int C1,
                                float* __restrict__ pivot, int rows_per_group, int G, float shards) {
    const int sg = blockIdx.x, g = threadIdx.x;
    if (g < G) pivot[(size_t)sg * G + g] = gn_pivot(X0, X1, C0, C1, nullptr, 1, sg, rows_per_group, G, g) / shards;
}

// (1) per-(stat group, row chunk) partial sums, reduced deterministically through LDS (no atomics)
__global__ void gn_partial_kernel(const half_t* __restrict__ X0, const half_t* __restrict__ X1, int C0, int C1,
                                  const float* __restrict__ pivot, int from_data, float* __restrict__ partial,
                                  int rows_per_group, int G, int rows_chunk, int rpb, int nchunks) {
    extern __shared__ __attribute__((aligned(16))) float red[];  // [rpb][C][2]
    const int C = C0 + C1, V = C >> 3, cpg = C / G;
    const int sg = blockIdx.x, chunk = blockIdx.y;
    const int tid = threadIdx.x;
    const int rl = tid / V, v = tid - rl * V;
    if (rl < rpb) {
        const int r_begin = chunk * rows_chunk;
        int r_end = r_begin + rows_chunk;
        if (r_end > rows_per_group) r_end = rows_per_group;
        const int c0 = v * 8;
        const bool from0 = c0 < C0;
        const half_t* base = from0 ? X0 : X1;
        const int ld = from0 ? C0 : C1;
        const int cc = from0 ? c0 : c0 - C0;
        // pivots straight from memory, no barrier (in flight with the first row loads); with >= 8 channels per group the
        // thread's 8 channels span at most two groups: two loads
        float s[8], q[8], k[8];
        if (cpg >= 8) {
            const int g0 = c0 / cpg, split = (g0 + 1) * cpg - c0;
            const float k0 = gn_pivot(X0, X1, C0, C1, pivot, from_data, sg, rows_per_group, G, g0);
            const float k1 = split < 8 ? gn_pivot(X0, X1, C0, C1, pivot, from_data, sg, rows_per_group, G, g0 + 1) : k0;
#pragma unroll
            for (int e = 0; e < 8; ++e) k[e] = e < split ? k0 : k1;
        } else {
#pragma unroll
            for (int e = 0; e < 8; ++e) k[e] = gn_pivot(X0, X1, C0, C1, pivot, from_data, sg, rows_per_group, G, (c0 + e) / cpg);
        }
#pragma unroll
        for (int e = 0; e < 8; ++e) s[e] = q[e] = 0.f;
        const half_t* ptr = base + ((size_t)sg * rows_per_group) * ld + cc;
        int r = r_begin + rl;
        for (; r + 3 * rpb < r_end; r += 4 * rpb) {  // 4 independent 16-byte loads in flight
            h8 x[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) x[u] = *(const h8*)(ptr + (size_t)(r + u * rpb) * ld);
#pragma unroll
            for (int u = 0; u < 4; ++u)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float f = (float)x[u][e] - k[e];
                    s[e] += f;
                    q[e] += f * f;
                }
        }
        for (; r < r_end; r += rpb) {
            const h8 x = *(const h8*)(ptr + (size_t)r * ld);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const float f = (float)x[e] - k[e];
                s[e] += f;
                q[e] += f * f;
            }
        }
        float* dst = red + ((size_t)rl * C + c0) * 2;
#pragma unroll
        for (int e = 0; e < 8; e += 2) *(f4*)(dst + 2 * e) = (f4){s[e], q[e], s[e + 1], q[e + 1]};
    }
    __syncthreads();
    if (tid < G) {
        float as = 0.f, aq = 0.f;
        for (int rr = 0; rr < rpb; ++rr) {
            const float* src = red + ((size_t)rr * C + tid * cpg) * 2;
            for (int c = 0; c < cpg; ++c) {
                as += src[2 * c];
                aq += src[2 * c + 1];
            }
        }
        float* o = partial + (((size_t)sg * nchunks + chunk) * G + tid) * 2;
        o[0] = as;
        o[1] = aq;
    }
}

// (2) normalise + affine (+ SiLU); grid = (row blocks per stat group, stat groups), block = V x rpb threads.
// A thread owns ONE 16-byte channel vector (its 8 channels' mean / rstd / gamma / beta live in registers for the whole
// kernel: no index division, no per-element group stepping, no gamma / beta reloads) and walks the rows of its block
// with U row loads in flight (the previous one-vector-per-iteration grid-stride form had 32 KiB in flight per CU and
// stopped at 3.6 TB/s read + write).
// x * sigmoid(x) on raw v_exp / v_rcp.  The output is fp16: over all 63 488 finite fp16 inputs it is at most 1 fp16 ulp from the exact
// result rounded once, on a handful of inputs, in every apply kernel (tests/gpu_checks.py::check_silu_all_inputs).
__device__ __forceinline__ float gn_silu(float x) {
    return x * __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(-1.4426950408889634f * x));
}

// The streaming part shared by the apply kernels: a thread owns ONE 16-byte channel vector and walks the rows of its block with U
// row loads in flight; smean / srstd: the statistics of this block's statistics group (LDS).
template <int U>
__device__ __forceinline__ void gn_apply_rows(const half_t* __restrict__ X0, const half_t* __restrict__ X1, int C0, int C1,
                                              half_t* __restrict__ Y, const half_t* __restrict__ gamma,
                                              const half_t* __restrict__ beta, const float* smean, const float* srstd,
                                              int rows_per_group, int G, int silu, int rpb, int rows_per_block) {
    const int C = C0 + C1, V = C >> 3, cpg = C / G;
    const int sg = blockIdx.y, tid = threadIdx.x;
    const int rl = tid / V, v = tid - rl * V;
    if (rl >= rpb) return;
    const int c0 = v * 8;
    const bool from0 = c0 < C0;
    const int ld = from0 ? C0 : C1;
    const half_t* src = (from0 ? X0 + c0 : X1 + (c0 - C0)) + (size_t)sg * rows_per_group * ld;
    half_t* dst = Y + (size_t)sg * rows_per_group * C + c0;
    float mean[8], rstd[8], ga[8], be[8];
    {
        const h8 gv = *(const h8*)(gamma + c0);
        const h8 bv = *(const h8*)(beta + c0);
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int ge = (c0 + e) / cpg;
            mean[e] = smean[ge];
            rstd[e] = srstd[ge];
            ga[e] = (float)gv[e];
            be[e] = (float)bv[e];
        }
    }
    const int r_begin = blockIdx.x * rows_per_block;
    int r_end = r_begin + rows_per_block;
    if (r_end > rows_per_group) r_end = rows_per_group;
    auto norm8 = [&](const h8& x) {
        h8 y;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            float f = ((float)x[e] - mean[e]) * rstd[e] * ga[e] + be[e];
            if (silu) f = gn_silu(f);
            y[e] = (half_t)f;
        }
        return y;
    };
    int r = r_begin + rl;
    for (; r + (U - 1) * rpb < r_end; r += U * rpb) {
        h8 x[U];
#pragma unroll
        for (int u = 0; u < U; ++u) x[u] = *(const h8*)(src + (size_t)(r + u * rpb) * ld);
#pragma unroll
        for (int u = 0; u < U; ++u) *(h8*)(dst + (size_t)(r + u * rpb) * C) = norm8(x[u]);
    }
    for (; r < r_end; r += rpb) *(h8*)(dst + (size_t)r * C) = norm8(*(const h8*)(src + (size_t)r * ld));
}

// The statistics prologue shared by the apply kernels.  The first min(blockDim.x, 256) threads are `parts` = that / G rows of G threads;
// thread (part, g) brings the sums (as, aq) of channel group g over its share of the chunks (or records), about the pivot kpiv.  The
// parts are added in ascending order -- the same additions in every block of a statistics group, so identical in all of them -- and
// thread g < G writes smean[g] = kpiv + s / n, srstd[g] = rsqrt(q / n - (s / n)^2 + eps).  Called by every thread of the block.
__device__ __forceinline__ void gn_fold_stats(float as, float aq, float kpiv, int parts, int G, float inv_cnt, float eps, float* smean,
                                              float* srstd) {
    __shared__ float rs[256], rq[256];
    const int tid = threadIdx.x;
    if (tid < 256) {
        rs[tid] = as;
        rq[tid] = aq;
    }
    __syncthreads();
    if (tid < G) {
        float s = 0.f, q = 0.f;
        for (int p2 = 0; p2 < parts; ++p2) {
            s += rs[p2 * G + tid];
            q += rq[p2 * G + tid];
        }
        const float m = s * inv_cnt;  // mean - pivot
        const float var = fmaxf(q * inv_cnt - m * m, 0.f);
        smean[tid] = kpiv + m;
        srstd[tid] = rsqrtf(var + eps);
    }
    __syncthreads();
}

// (as, aq) += the record src = (K_i, s_i, q_i) over n values, moved to the pivot kpiv exactly: s_i + n d, q_i + 2 d s_i + n d^2 with
// d = K_i - kpiv (a difference of two fp16 values: exact)
__device__ __forceinline__ void gn_move_record(const float* src, float kpiv, float n, float& as, float& aq) {
    const float d = src[0] - kpiv, si = src[1], qi = src[2];
    const float nd = n * d;
    as += si + nd;
    aq += qi + (2.f * d * si + nd * d);
}

template <int U>
__global__ __launch_bounds__(1024) void gn_apply_kernel(const half_t* __restrict__ X0, const half_t* __restrict__ X1, int C0,
                                                        int C1, half_t* __restrict__ Y, const half_t* __restrict__ gamma,
                                                        const half_t* __restrict__ beta, const float* __restrict__ pivot,
                                                        int from_data, const float* __restrict__ partial, int nchunks, float inv_cnt,
                                                        float eps, int rows_per_group, int G, int silu, int rpb,
                                                        int rows_per_block) {
    __shared__ float smean[64], srstd[64];
    const int sg = blockIdx.y, tid = threadIdx.x;
    const int nt = blockDim.x < 256 ? blockDim.x : 256;
    const int parts = nt / G;  // G <= 64 <= blockDim.x
    const int g = tid % G, part = tid / G;
    // this group's pivot, loaded before the chunk sums so that its latency overlaps theirs
    const float kpiv = tid < G ? gn_pivot(X0, X1, C0, C1, pivot, from_data, sg, rows_per_group, G, tid) : 0.f;
    float as = 0.f, aq = 0.f;
    if (part < parts)   // thread (part, g) takes chunks part, part + parts, ... in ascending order
        for (int c = part; c < nchunks; c += parts) {
            const float* src = partial + (((size_t)sg * nchunks + c) * G + g) * 2;
            as += src[0];
            aq += src[1];
        }
    gn_fold_stats(as, aq, kpiv, parts, G, inv_cnt, eps, smean, srstd);
    gn_apply_rows<U>(X0, X1, C0, C1, Y, gamma, beta, smean, srstd, rows_per_group, G, silu, rpb, rows_per_block);
}

// GroupNorm from the records a producing GEMM wrote (AnyV2VGemmDesc.gn_stats): gn_apply_kernel with another statistics prologue.
// rec: [statistics group][record][G][3] = (K_i, s_i, q_i), nrec records per (statistics group, channel group), each over n_rec
// values except the last (n_last).  Every block moves them to the pivot of record 0 (gn_move_record), thread (part, g) taking records
// part, part + parts, ... in ascending order.
template <int U>
__global__ __launch_bounds__(1024) void gn_apply_stats_kernel(const half_t* __restrict__ X, half_t* __restrict__ Y,
                                                              const half_t* __restrict__ gamma, const half_t* __restrict__ beta,
                                                              const float* __restrict__ rec, int nrec, float n_rec, float n_last,
                                                              float inv_cnt, float eps, int C, int rows_per_group, int G, int silu,
                                                              int rpb, int rows_per_block) {
    __shared__ float smean[64], srstd[64];
    const int sg = blockIdx.y, tid = threadIdx.x;
    const int nt = blockDim.x < 256 ? blockDim.x : 256;
    const int parts = nt / G;  // G <= 64 <= blockDim.x
    const int g = tid % G, part = tid / G;
    const float* base = rec + ((size_t)sg * nrec * G + g) * 3;
    const float kpiv = base[0];
    float as = 0.f, aq = 0.f;
    if (part < parts)
        for (int c = part; c < nrec; c += parts) gn_move_record(base + (size_t)c * G * 3, kpiv, c + 1 == nrec ? n_last : n_rec, as, aq);
    gn_fold_stats(as, aq, kpiv, parts, G, inv_cnt, eps, smean, srstd);
    // (X twice: the second source is never read with C1 = 0, and a literal nullptr here crashes hipcc 7.2's inliner)
    gn_apply_rows<U>(X, X, C, 0, Y, gamma, beta, smean, srstd, rows_per_group, G, silu, rpb, rows_per_block);
}

// Long statistics groups (the 5-D norms: 16 frames x 4096 pixels = 4096 records per channel group): runs of `run` consecutive
// records are first moved to the pivot of the run's first record and written as one record each, so that the apply blocks fold at
// most GN_MAX_CHUNKS of them.  One thread per (statistics group, run, channel group), ascending order.
__global__ void gn_fold_records_kernel(const float* __restrict__ rec, float* __restrict__ out, int nrec, int run, int nruns, int G,
                                       float n_rec) {
    const int sg = blockIdx.y, j = blockIdx.x, g = threadIdx.x;
    if (g >= G) return;
    const float* base = rec + (((size_t)sg * nrec + (size_t)j * run) * G + g) * 3;
    int cnt = nrec - j * run;
    if (cnt > run) cnt = run;
    const float kpiv = base[0];
    float as = 0.f, aq = 0.f;
    for (int c = 0; c < cnt; ++c) gn_move_record(base + (size_t)c * G * 3, kpiv, n_rec, as, aq);
    float* o = out + (((size_t)sg * nruns + j) * G + g) * 3;
    o[0] = kpiv;
    o[1] = as;
    o[2] = aq;
}

extern "C" int64_t anyv2v_groupnorm_scratch_floats(int32_t M, int32_t rows_per_group, int32_t G) {
    return av_gn_scratch_floats(M, rows_per_group, G);
}

// resident gn_apply blocks on the whole device for a block size (occupancy query, cached per size)
static int gn_apply_slots(int threads) {
    static int cache[1025];
    if (threads < 1 || threads > 1024) return 2048;
    if (cache[threads] == 0) {
        int per_cu = 0, dev = 0, cus = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, gn_apply_kernel<4>, threads, 0) != hipSuccess || per_cu < 1) per_cu = 7;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess ||
            cus < 1)
            cus = 256;
        cache[threads] = per_cu * cus;
    }
    return cache[threads];
}

// launch plan shared by the one-call and the two-phase (sharded) entry points: av_gn_plan under the batch hint in force and this
// device's occupancy.  X0 is not null; a second width needs a second source.
static GnPlan gn_plan(const void* X0, const void* X1, int32_t C0, int32_t C1, int32_t M, int32_t rows_per_group, int32_t G) {
    if (C1 > 0 && !X1) {
        anyv2v_set_error("groupnorm: bad C0/C1");
        return GnPlan{ANYV2V_EINVAL};
    }
    return av_gn_plan(C0, C1, M, rows_per_group, G, av_hint_rows(M), gn_apply_slots(av_gn_threads(C0 + C1, G)),
                      av_aligned16(X0) && av_aligned16(X1));
}

// pivot: [nsg][G] agreed pivots, or nullptr: each stat group's own first element per channel group (from_data) or 0
static int gn_partial(const GnPlan& pl, const void* X0, const void* X1, int32_t C0, int32_t C1, const float* pivot,
                      int from_data, float* stats, int32_t rows_per_group, int32_t G, hipStream_t s) {
    // stats: [nsg][nchunks][G][2]
    hipLaunchKernelGGL(gn_partial_kernel, dim3(pl.nsg, pl.nchunks), dim3(pl.threads), pl.lds, s, (const half_t*)X0,
                       (const half_t*)X1, C0, C1, pivot, from_data, stats, rows_per_group, G, pl.rows_chunk, pl.rpb, pl.nchunks);
    return av_launch_status("groupnorm<partial>");
}

static int gn_apply(const GnPlan& pl, const void* X0, const void* X1, int32_t C0, int32_t C1, void* Y, const void* gamma,
                    const void* beta, const float* pivot, int from_data, const float* stats, int32_t rows_per_group,
                    int32_t G, float eps, int32_t silu, int32_t shards, hipStream_t s) {
    AV_CHECK(av_aligned16(Y) && av_aligned16(gamma) && av_aligned16(beta), "groupnorm: pointers must be 16-byte aligned");
    const float inv_cnt = 1.0f / ((float)rows_per_group * (float)((C0 + C1) / G) * (float)shards);
    hipLaunchKernelGGL(gn_apply_kernel<4>, dim3((unsigned)pl.bps, (unsigned)pl.nsg), dim3(pl.threads), 0, s,
                       (const half_t*)X0, (const half_t*)X1, C0, C1, (half_t*)Y, (const half_t*)gamma, (const half_t*)beta,
                       pivot, from_data, stats, pl.nchunks, inv_cnt, eps, rows_per_group, G, silu, pl.rpb, pl.rows_block);
    return av_launch_status("groupnorm");
}

extern "C" int anyv2v_groupnorm_f16(const void* X0, const void* X1, int32_t C0, int32_t C1, void* Y,
                                    const void* gamma, const void* beta, float* stats, int32_t M,
                                    int32_t rows_per_group, int32_t G, float eps, int32_t silu, void* stream) {
    AV_CHECK(X0 && Y && gamma && beta && stats, "groupnorm: null pointer");
    const GnPlan pl = gn_plan(X0, X1, C0, C1, M, rows_per_group, G);
    if (pl.status) return pl.status;
    if (int rc = gn_partial(pl, X0, X1, C0, C1, nullptr, 1, stats, rows_per_group, G, (hipStream_t)stream)) return rc;
    return gn_apply(pl, X0, X1, C0, C1, Y, gamma, beta, nullptr, 1, stats, rows_per_group, G, eps, silu, 1, (hipStream_t)stream);
}

extern "C" int64_t anyv2v_groupnorm_stats_floats(int32_t M, int32_t rows_per_group, int32_t G) {
    return av_gn_stats_floats(M, rows_per_group, G);
}

extern "C" int anyv2v_groupnorm_apply_stats_f16(const void* X, void* Y, const void* gamma, const void* beta, float* stats,
                                                const int32_t* sizes, float eps, int32_t silu, void* stream) {
    AV_CHECK(X && Y && gamma && beta && stats && sizes, "groupnorm_apply_stats: null pointer");
    const int32_t M = sizes[0], C = sizes[1], rows_per_group = sizes[2], G = sizes[3];
    const GnPlan pl = gn_plan(X, nullptr, C, 0, M, rows_per_group, G);
    if (pl.status) return pl.status;
    AV_CHECK(av_aligned16(Y) && av_aligned16(gamma) && av_aligned16(beta), "groupnorm: pointers must be 16-byte aligned");
    const GnRecordsPlan rp = av_gn_records_plan(M, C, rows_per_group, G);
    if (rp.status) return rp.status;
    AV_CHECK((int64_t)sizes[4] >= av_gn_stats_floats(M, rows_per_group, G),
             "groupnorm_apply_stats: stats holds %d floats, needs anyv2v_groupnorm_stats_floats() = %lld", sizes[4],
             (long long)av_gn_stats_floats(M, rows_per_group, G));
    const float* rec = stats;
    hipStream_t s = (hipStream_t)stream;
    if (rp.fold) {   // runs of records first, into the tail of `stats`
        hipLaunchKernelGGL(gn_fold_records_kernel, dim3(rp.nruns, pl.nsg), dim3(64), 0, s, rec, stats + rp.folded_at, rp.nrec, rp.run,
                           rp.nruns, G, rp.n_gemm);
        if (int rc = av_launch_status("groupnorm<fold records>")) return rc;
        rec = stats + rp.folded_at;
    }
    const float inv_cnt = 1.0f / ((float)rows_per_group * (float)(C / G));
    hipLaunchKernelGGL(gn_apply_stats_kernel<4>, dim3((unsigned)pl.bps, (unsigned)pl.nsg), dim3(pl.threads), 0, s, (const half_t*)X,
                       (half_t*)Y, (const half_t*)gamma, (const half_t*)beta, rec, rp.nruns, rp.n_rec, rp.n_last, inv_cnt, eps, C,
                       rows_per_group, G, silu, pl.rpb, pl.rows_block);
    return av_launch_status("groupnorm<from records>");
}

// Sharded GroupNorm (a clip whose frames or pixels are split over `shards` ranks, every rank holding the same local
// shape).  Pivoted form: phase 0 writes this rank's pivot / shards, which the caller adds over the ranks (all-reduce SUM)
// into the agreed pivot; phase 1 writes this rank's partial sums about it; the caller adds the first
// anyv2v_groupnorm_partial_floats() floats of `stats` over the ranks (all-reduce SUM, RCCL); phase 2 normalises with the
// agreed pivot and shards x the local element count.  The ABI-101 pair (partial_f16 / apply_f16, one all-reduce) is the
// same with pivot 0.
extern "C" int anyv2v_groupnorm_pivot_f16(const void* X0, const void* X1, int32_t C0, int32_t C1, float* pivot, int32_t M,
                                          int32_t rows_per_group, int32_t G, int32_t shards, void* stream) {
    AV_CHECK(X0 && pivot, "groupnorm_pivot: null pointer");
    AV_CHECK(shards >= 1, "groupnorm_pivot: shards must be >= 1");
    const GnPlan pl = gn_plan(X0, X1, C0, C1, M, rows_per_group, G);
    if (pl.status) return pl.status;
    hipLaunchKernelGGL(gn_pivot_kernel, dim3(pl.nsg), dim3(64), 0, (hipStream_t)stream, (const half_t*)X0, (const half_t*)X1, C0,
                       C1, pivot, rows_per_group, G, (float)shards);
    return av_launch_status("groupnorm<pivot>");
}

extern "C" int64_t anyv2v_groupnorm_partial_floats(int32_t M, int32_t rows_per_group, int32_t G, int32_t C) {
    return av_gn_partial_floats(av_gn_plan(C, 0, M, rows_per_group, G, av_hint_rows(M), 1), G);   // (the chunking ignores the occupancy)
}

extern "C" int anyv2v_groupnorm_partial_pivot_f16(const void* X0, const void* X1, int32_t C0, int32_t C1, const float* pivot,
                                                  float* stats, int32_t M, int32_t rows_per_group, int32_t G, void* stream) {
    AV_CHECK(X0 && pivot && stats, "groupnorm_partial: null pointer");
    const GnPlan pl = gn_plan(X0, X1, C0, C1, M, rows_per_group, G);
    if (pl.status) return pl.status;
    return gn_partial(pl, X0, X1, C0, C1, pivot, 0, stats, rows_per_group, G, (hipStream_t)stream);
}

extern "C" int anyv2v_groupnorm_apply_pivot_f16(const void* X0, const void* X1, int32_t C0, int32_t C1, void* Y,
                                                const void* gamma, const void* beta, const float* pivot, const float* stats,
                                                int32_t M, int32_t rows_per_group, int32_t G, float eps, int32_t silu,
                                                int32_t shards, void* stream) {
    AV_CHECK(X0 && Y && gamma && beta && pivot && stats, "groupnorm_apply: null pointer");
    AV_CHECK(shards >= 1, "groupnorm_apply: shards must be >= 1");
    const GnPlan pl = gn_plan(X0, X1, C0, C1, M, rows_per_group, G);
    if (pl.status) return pl.status;
    return gn_apply(pl, X0, X1, C0, C1, Y, gamma, beta, pivot, 0, stats, rows_per_group, G, eps, silu, shards, (hipStream_t)stream);
}

extern "C" int anyv2v_groupnorm_partial_f16(const void* X0, const void* X1, int32_t C0, int32_t C1, float* stats, int32_t M,
                                            int32_t rows_per_group, int32_t G, void* stream) {
    AV_CHECK(X0 && stats, "groupnorm_partial: null pointer");
    const GnPlan pl = gn_plan(X0, X1, C0, C1, M, rows_per_group, G);
    if (pl.status) return pl.status;
    return gn_partial(pl, X0, X1, C0, C1, nullptr, 0, stats, rows_per_group, G, (hipStream_t)stream);
}

extern "C" int anyv2v_groupnorm_apply_f16(const void* X0, const void* X1, int32_t C0, int32_t C1, void* Y,
                                          const void* gamma, const void* beta, const float* stats, int32_t M,
                                          int32_t rows_per_group, int32_t G, float eps, int32_t silu, int32_t shards,
                                          void* stream) {
    AV_CHECK(X0 && Y && gamma && beta && stats, "groupnorm_apply: null pointer");
    AV_CHECK(shards >= 1, "groupnorm_apply: shards must be >= 1");
    const GnPlan pl = gn_plan(X0, X1, C0, C1, M, rows_per_group, G);
    if (pl.status) return pl.status;
    return gn_apply(pl, X0, X1, C0, C1, Y, gamma, beta, nullptr, 0, stats, rows_per_group, G, eps, silu, shards, (hipStream_t)stream);
}

// ---------------------------------------------------------------------------------------------------------
// LayerNorm: one wave per row, row kept in registers (two-pass mean / variance), C % 8 == 0, C <= 2048.
template <int NV>
__global__ __launch_bounds__(256) void layernorm_kernel(const half_t* __restrict__ X, half_t* __restrict__ Y,
                                                        const half_t* __restrict__ gamma,
                                                        const half_t* __restrict__ beta, int M, int C, float eps) {
    const int lane = threadIdx.x & 63;
    const int wpb = blockDim.x >> 6;
    const int V = C >> 3;
    const int stride = gridDim.x * wpb;
    // gamma / beta of this lane's vectors: loaded once per wave, not once per row
    h8 ga[NV], be[NV];
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const int v = lane + 64 * i;
        if (v < V) {
            ga[i] = *(const h8*)(gamma + v * 8);
            be[i] = *(const h8*)(beta + v * 8);
        }
    }
    auto load_row = [&](int row, h8 (&xv)[NV]) {
        const half_t* x = X + (size_t)row * C;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int v = lane + 64 * i;
            if (v < V) xv[i] = *(const h8*)(x + v * 8);
        }
    };
    auto norm_row = [&](int row, const h8 (&xv)[NV]) {
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i)
            if (lane + 64 * i < V) {
#pragma unroll
                for (int e = 0; e < 8; ++e) sum += (float)xv[i][e];
            }
        const float mean = wave_sum(sum) / (float)C;
        float sq = 0.f;
#pragma unroll
        for (int i = 0; i < NV; ++i)
            if (lane + 64 * i < V) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const float d = (float)xv[i][e] - mean;
                    sq += d * d;
                }
            }
        const float rstd = rsqrtf(wave_sum(sq) / (float)C + eps);
        half_t* y = Y + (size_t)row * C;
#pragma unroll
        for (int i = 0; i < NV; ++i) {
            const int v = lane + 64 * i;
            if (v < V) {
                h8 o;
#pragma unroll
                for (int e = 0; e < 8; ++e)
                    o[e] = (half_t)(((float)xv[i][e] - mean) * rstd * (float)ga[i][e] + (float)be[i][e]);
                *(h8*)(y + v * 8) = o;
            }
        }
    };
    // two rows in flight per wave (one row per wave and iteration left ~20 KiB in flight per CU at C = 320)
    int row = blockIdx.x * wpb + (threadIdx.x >> 6);
    for (; row + stride < M; row += 2 * stride) {
        h8 xa[NV], xb[NV];
        load_row(row, xa);
        load_row(row + stride, xb);
        norm_row(row, xa);
        norm_row(row + stride, xb);
    }
    if (row < M) {
        h8 xa[NV];
        load_row(row, xa);
        norm_row(row, xa);
    }
}

// any C (tiny rows, e.g. C = 4 of image_latents_temporal_encoder.norm1): one thread per row
__global__ void layernorm_naive_kernel(const half_t* __restrict__ X, half_t* __restrict__ Y,
                                       const half_t* __restrict__ gamma, const half_t* __restrict__ beta, int M, int C,
                                       float eps) {
    const int row = blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= M) return;
    const half_t* x = X + (size_t)row * C;
    float s = 0.f;
    for (int c = 0; c < C; ++c) s += (float)x[c];
    const float mean = s / (float)C;
    float q = 0.f;
    for (int c = 0; c < C; ++c) {
        const float d = (float)x[c] - mean;
        q += d * d;
    }
    const float rstd = rsqrtf(q / (float)C + eps);
    for (int c = 0; c < C; ++c)
        Y[(size_t)row * C + c] = (half_t)(((float)x[c] - mean) * rstd * (float)gamma[c] + (float)beta[c]);
}

extern "C" int anyv2v_layernorm_f16(const void* X, void* Y, const void* gamma, const void* beta, int32_t M, int32_t C,
                                    float eps, void* stream) {
    AV_CHECK(X && Y && gamma && beta && M > 0 && C > 0, "layernorm: bad arguments");
    hipStream_t s = (hipStream_t)stream;
    const bool fast = C % 8 == 0 && C <= 2048 && av_aligned16(X) && av_aligned16(Y) && av_aligned16(gamma) &&
                      av_aligned16(beta);
    if (!fast) {
        hipLaunchKernelGGL(layernorm_naive_kernel, dim3((M + 255) / 256), dim3(256), 0, s, (const half_t*)X, (half_t*)Y,
                           (const half_t*)gamma, (const half_t*)beta, M, C, eps);
        return av_launch_status("layernorm_naive");
    }
    int blocks = (M + 7) / 8;  // 4 waves per block, two rows in flight per wave
    if (blocks > 8192) blocks = 8192;
    const int V = C / 8;
#define LN_LAUNCH(NV)                                                                                             \
    hipLaunchKernelGGL(layernorm_kernel<NV>, dim3(blocks), dim3(256), 0, s, (const half_t*)X, (half_t*)Y,         \
                       (const half_t*)gamma, (const half_t*)beta, M, C, eps)
    if (V <= 64) LN_LAUNCH(1);
    else if (V <= 128) LN_LAUNCH(2);
    else if (V <= 192) LN_LAUNCH(3);
    else LN_LAUNCH(4);
#undef LN_LAUNCH
    return av_launch_status("layernorm");
}
