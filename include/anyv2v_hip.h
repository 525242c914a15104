/*
 * anyv2v_hip.h -- C ABI of libanyv2v_hip.so: hand-written HIP kernels (gfx950 / MI355X) for the
 * AnyV2V I2VGen-XL DDIM-inversion + PnP-edit hot path.
 *
 * The reference (TIGER-AI-Lab/AnyV2V) is pure Python and has no FFI layer; its hot path sits behind
 * Python protocol seams.  Each entry point below names the reference call it replaces
 * (paths relative to the reference root).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer to fp16 ("half") data unless the name says f32 / i32 / i64;
 *   - activations are channels-last token matrices  X[(b f) (h w), C]  (row-major, leading dim in elements);
 *   - `stream` is a hipStream_t (0 = default stream); kernels are enqueued, never synchronised;
 *   - nothing allocates: the caller owns all memory (PyTorch caching allocator in the Python host);
 *   - return value: 0 = ok, <0 = ANYV2V_E* (message via anyv2v_last_error()), >0 = hipError_t.
 */
#ifndef ANYV2V_HIP_H
#define ANYV2V_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ANYV2V_OK 0
#define ANYV2V_EINVAL (-1)   /* bad shape / alignment / null pointer            */
#define ANYV2V_EUNSUPPORTED (-2) /* shape outside what the fast kernels cover   */

/* ---- gather-GEMM ------------------------------------------------------------------------------
 * C[m, n] = epilogue( sum_{tap} sum_{k<K} A[row(m,tap), k] * W[n, tap*K + k] ),  fp16 in, fp32 acc.
 * A is the channel-concatenation [A0 | A1] (K = C0 + C1) -- the skip `torch.cat` of the up blocks
 * folded into the K loop.
 *   mode 0  LINEAR    : 1 tap, row = m.                     torch Linear / 1x1 conv
 *                       (attn.to_q/to_k/to_v/to_out[0]  i2vgen-xl/pnp_utils.py:175,182-183,216;
 *                        conv_shortcut pnp_utils.py:117-122; time_emb_proj pnp_utils.py:81-88)
 *   mode 1  CONV2D3x3 : 9 taps, pad 1, stride 1|2, optional nearest x2 upsample folded into the gather
 *                       (conv1/conv2 pnp_utils.py:78,107; Upsample2D/Downsample2D pnp_utils.py:51-76);
 *                       asym = 1: zero padding only after the last row / column (F.pad (0,1,0,1) + stride-2
 *                       conv of the AutoencoderKL encoder's Downsample2D, pipeline_i2vgen_xl.py:565-592)
 *   mode 2  TEMPORAL3 : 3 taps along the frame axis, pad 1 (Conv3d (3,1,1) of TemporalConvLayer;
 *                       consisti2v/consisti2v/models/videoldm_unet_blocks.py:316-328)
 * epilogue: + bias[n]; + rowvec[(m / rowvec_div) * ldrv + n] (the temb broadcast pnp_utils.py:91-92);
 *           act: 0 none, 1 SiLU, 2 GELU(erf), 3 GEGLU (W packed [16 x h | 16 x gate] per 32 rows, out N/2),
 *                4 = store the fp32 accumulator (+bias) to C as float (ldc in floats; no rowvec / R): attention
 *                logits of the VAE mid-block's single 512-wide head;
 *           + R[m, n] (residual, pnp_utils.py:124); store fp16.
 */
/* AnyV2VGemmDesc.flags.  All but LDS_DMA are A/B switches and test hooks, off by default; unnamed bits are ignored. */
#define ANYV2V_GEMM_NAIVE (1 << 0)         /* Run the naive reference kernel. */
#define ANYV2V_GEMM_LDS_DMA (1 << 1)       /* Stage operands by LDS-DMA; only the 128-row and naive kernels run without it. */
#define ANYV2V_GEMM_NO_BIG (1 << 2)        /* Never take the persistent 192x320 kernel, nor the weight-stationary one. */
#define ANYV2V_GEMM_FORCE_BIG (1 << 3)     /* Take the persistent kernel whenever the shape allows. */
#define ANYV2V_GEMM_NO_SPLITK (1 << 4)     /* Never split along K. */
#define ANYV2V_GEMM_PROBE_TRACE (1 << 5)   /* Probe build: phase timestamps; ignored by the product library. */
#define ANYV2V_GEMM_PROBE_KO_SHIFT 6       /* Bits 6-8, probe build: K-loop knock-outs; ignored by the product library. */
#define ANYV2V_GEMM_NO_WS (1 << 9)         /* Never take the weight-stationary kernel. */
#define ANYV2V_GEMM_FORCE_WS (1 << 10)     /* Take it wherever it is implemented, also below its M >= 32768 threshold. */
#define ANYV2V_GEMM_NF4 (1 << 11)          /* 128-column tiles in the 128-row kernel whatever the fill heuristic says. */
#define ANYV2V_GEMM_NF5 (1 << 12)          /* 160-column tiles likewise. */
#define ANYV2V_GEMM_RASTER_SHIFT 13        /* Bits 13-15, persistent kernels' tile order: 0 auto, 1 classic, 2..6 super-tiles of
                                              4 / 8 / 16 / 32 / 2 M-tiles per XCD round; same bits in every order. */
#define ANYV2V_GEMM_RASTER_NFAST (1 << 16) /* Walk the super-tiles N-fastest. */
#define ANYV2V_GEMM_PP (1 << 17)           /* Take the ping-pong kernel wherever the shape allows (N % 320 = 0, no GEGLU). */
#define ANYV2V_GEMM_NO_PP (1 << 18)        /* Never take it. */
#define ANYV2V_GEMM_PP_192 (1 << 19)       /* Its 192-row tile. */
#define ANYV2V_GEMM_PP_256 (1 << 20)       /* Its 256-row tile. */
#define ANYV2V_GEMM_SW (1 << 21)           /* Take the one-wave-per-SIMD kernel wherever the shape allows (N % 320 = 0, K >= 128). */
#define ANYV2V_GEMM_NO_SW (1 << 22)        /* Never take it, its stream-K form or the LDS-patch kernel. */
#define ANYV2V_GEMM_PROBE_SW_KO_SHIFT 23   /* Bits 23-25, probe build: its knock-outs / K orders; ignored by the product library. */
#define ANYV2V_GEMM_STREAMK (1 << 26)      /* Allow the stream-K form where it pays (un-hinted, 126 MB workspace; another summation order). */
#define ANYV2V_GEMM_FORCE_STREAMK (1 << 27) /* Take it wherever it can run. */
#define ANYV2V_GEMM_SWH (1 << 28)          /* 3x3 stride-1 "same" convolutions at width 16 / 32 / 64 on the LDS-patch kernel (another order). */
#define ANYV2V_GEMM_PROBE_KORDER_SHIFT 29  /* Bits 29-30, probe patches: K order of the persistent kernel; ignored by the product library. */
typedef struct AnyV2VGemmDesc {
    const void* A0;
    const void* A1;      /* may be NULL when C1 == 0 */
    const void* W;       /* [N][taps*(C0+C1)] */
    void* C;
    const void* bias;    /* [N] or NULL */
    const void* rowvec;  /* [M/rowvec_div][ldrv] or NULL */
    const void* R;       /* [M][ldr] or NULL */
    int32_t M, N;
    int32_t C0, C1;
    int32_t lda0, lda1, ldc, ldr, ldrv, rowvec_div;
    int32_t mode;
    int32_t Hi, Wi, Ho, Wo, stride, up; /* mode 1 */
    int32_t asym;                       /* mode 1: 0 = pad 1 on every side, 1 = pad only right / bottom */
    int32_t F, HW;                      /* mode 2: frames per clip, pixels per frame */
    int32_t act;
    int32_t flags;       /* ANYV2V_GEMM_* above */
    void* workspace;     /* optional fp32 scratch for split-K partial tiles (small-M, long-K launches) or NULL */
    int64_t workspace_bytes;
    /* LayerNorm folded into the projection that consumes it (BasicTransformerBlock.norm1/2/3 -> attn.to_q/k/v / ff.net[0].proj,
     * consisti2v/consisti2v/models/videoldm_transformer_blocks.py:461-564): with ln_c1 != NULL the rows of A0 are the
     * UN-normalised residual stream and
     *     C = act( rstd[m] * (A0 W^T - mean[m] * ln_c1) + bias ),   mean / rstd = LayerNorm statistics of row m over C0, eps = ln_eps,
     * where the caller passes W = W_proj diag(gamma) (fp16), ln_c1[n] = sum_k W[n][k] (fp32, summed over the fp16-rounded W) and
     * bias = b_proj + W_proj beta.  Mode 0, C0 = 320 (N % 160 = 0) or C0 = 512 with GEGLU (N % 128 = 0), no rowvec / R: other
     * shapes return ANYV2V_EUNSUPPORTED (the caller then runs anyv2v_layernorm_f16 + the plain GEMM). */
    const float* ln_c1;
    float ln_eps;
    int32_t reserved0;
    /* GroupNorm statistics from the epilogue (ABI 105; NULL / 0 = off).  With gn_stats != NULL the launch also writes partial
     * GroupNorm statistics of the STORED fp16 output (after bias, rowvec, activation, residual and rounding) for the consumer
     * GroupNorm(gn_groups) over statistics groups of gn_rows_per_group consecutive rows: one record of 3 floats per (16 consecutive
     * rows, channel group),
     *     gn_stats[((m / 16) * gn_groups + g) * 3 + {0, 1, 2}] = (K, sum(x - K), sum((x - K)^2)),   K = C[16 (m / 16)][g * N / gn_groups]
     * over the record's 16 x (N / gn_groups) values -- each record about its own first element, summed in an order that depends only
     * on the position inside the record (not on the tile, the kernel family or the batch hint; no atomics), so a [negative, editing]
     * launch writes bit for bit the records the three-branch launch writes for those rows.  gn_stats_floats: capacity of gn_stats, at
     * least anyv2v_gemm_gn_stats_floats(d).  A launch whose plan cannot emit statistics fails with ANYV2V_EINVAL -- ask first. */
    float* gn_stats;
    int64_t gn_stats_floats;
    int32_t gn_rows_per_group;
    int32_t gn_groups;
} AnyV2VGemmDesc;

int anyv2v_gemm_f16(const AnyV2VGemmDesc* d, void* stream);
/* Floats of gn_stats the launch described by `d` would write (3 * (M / 16) * gn_groups), or 0 when the plan this descriptor gets
 * cannot emit statistics: split-K plans, the naive kernel, the weight-stationary / LayerNorm-fold kernel, GEGLU / fp32-out
 * epilogues, the off-by-default kernels flags bits 17 / 21 / 26-28 select, N not a multiple of 160, N / gn_groups not a divisor of
 * 40 (a channel group must not straddle a 160-column wave tile), M or gn_rows_per_group not a multiple of 16.  Decides exactly as
 * anyv2v_gemm_f16 will (same flags, workspace, alignment and batch hint; gn_stats and C may still be NULL), launches nothing and
 * touches no device.  A descriptor the launch would reject (ANYV2V_EINVAL / ANYV2V_EUNSUPPORTED) answers 0 and leaves the launch's
 * text in anyv2v_last_error(). */
int64_t anyv2v_gemm_gn_stats_floats(const AnyV2VGemmDesc* d);
/* Launches that emitted statistics since the counter was last reset (reset != 0: return the count, then zero it).  Host-side,
 * counted at enqueue time, before the launch status is known (a graph replay does not count; a launch the runtime rejects
 * does).  One process-global integer, NOT thread-safe, like the batch hint.  For tests: a forced path must not pass because it
 * fell back. */
int64_t anyv2v_gemm_gn_launches(int32_t reset);

/* ---- fused feed-forward ----------------------------------------------------------------------
 * Y = GEGLU(X W1^T + b1) W2^T + b2 (+ R): the FeedForward of BasicTransformerBlock (diffusers-0.26.3 `FeedForward(dim,
 * activation_fn="geglu")` behind pipeline_i2vgen_xl.py:1146; in-tree restatement consisti2v/consisti2v/models/
 * videoldm_transformer_blocks.py:545-563) in one kernel -- the [M, H] hidden activation never reaches HBM.  Implemented for
 * C = 320, H = 1280 (the 64x64 level); anything else returns ANYV2V_EUNSUPPORTED and the caller runs the two GEMMs.
 *   W1 [2 H][C], b1 [2 H]: rows interleaved [16 x h | 16 x gate] per 32 (the act = 3 packing of anyv2v_gemm_f16);
 *   W2 [H / 32][C][32]   : slab-major; inside a slab of 32 hidden units, column 8 q + e (q = 0..3) holds hidden unit 4 q + e for
 *                          e < 4 and 16 + 4 q + (e - 4) for e >= 4 (the MFMA K-slot order the kernel produces the hidden values in);
 *   b2 [C]; R [M][ldr] or NULL; X [M][ldx]; Y [M][ldy].  fp32 accumulation, the hidden value rounded to fp16 once, Y = fp16(acc + b2)
 *   then + R in fp16 (the rounding points of the unfused GEGLU GEMM + Linear pair). */
typedef struct AnyV2VFFDesc {
    const void* X;
    const void* W1;
    const void* b1;
    const void* W2;
    const void* b2;
    const void* R;
    void* Y;
    int32_t M, C, H;
    int32_t ldx, ldr, ldy;
    int32_t flags;       /* reserved, 0 */
    int32_t reserved0;
} AnyV2VFFDesc;

int anyv2v_ff_geglu_f16(const AnyV2VFFDesc* d, void* stream);

/* ---- normalisation ---------------------------------------------------------------------------
 * GroupNorm over channels-last tokens, optionally fused SiLU, input = channel concat [X0 | X1].
 * Statistics are taken over `rows_per_group` consecutive rows x (C/G) channels: rows_per_group = H*W
 * gives the 4-D per-frame GroupNorm (ResnetBlock2D.norm1/norm2 pnp_utils.py:48,104; Transformer2DModel.norm),
 * rows_per_group = F*H*W the 5-D per-clip one (TemporalConvLayer, TransformerTemporalModel.norm).
 * `stats` is caller-provided scratch of anyv2v_groupnorm_scratch_floats(M, rows_per_group, G) floats (mean/rstd
 * plus per-chunk partial sums; the reduction uses no atomics, so results are bit-reproducible).
 */
int64_t anyv2v_groupnorm_scratch_floats(int32_t M, int32_t rows_per_group, int32_t G);
int anyv2v_groupnorm_f16(const void* X0, const void* X1, int32_t C0, int32_t C1, void* Y, const void* gamma,
                         const void* beta, float* stats, int32_t M, int32_t rows_per_group, int32_t G, float eps,
                         int32_t silu, void* stream);
/* The same from the records a producing anyv2v_gemm_f16 launch wrote (AnyV2VGemmDesc.gn_stats): normalise + affine (+ SiLU), no
 * partial pass over X.  sizes = {M, C, rows_per_group, G, capacity of stats in floats}; single source (the concat form stays on
 * anyv2v_groupnorm_f16); rows_per_group a multiple of 16.  `stats` holds anyv2v_groupnorm_stats_floats(M, rows_per_group, G)
 * floats: the 3 * (M / 16) * G the GEMM writes, then room in which statistics groups of more than 256 records (the 5-D norms) are
 * first folded in runs (one more small launch).  Records are moved to one pivot per (statistics group, channel group), the first
 * record's, exactly:  s += s_i + n_i d,  q += q_i + 2 d s_i + n_i d^2,  d = K_i - K,  in a fixed order that is the same in every
 * block and depends on rows_per_group only: two runs are bit-equal, and so are a batch-hinted launch and the launch it stands for. */
int64_t anyv2v_groupnorm_stats_floats(int32_t M, int32_t rows_per_group, int32_t G);
int anyv2v_groupnorm_apply_stats_f16(const void* X, void* Y, const void* gamma, const void* beta, float* stats,
                                     const int32_t* sizes, float eps, int32_t silu, void* stream);

/* Sharded 5-D GroupNorm, for a clip whose frames / pixels are split over `shards` ranks (the 128-frame mode,
 * gradio_demo.py:129-131; every rank holds the same local shape).  The statistics are sums about one pivot per
 * (statistics group, channel group), which all ranks must share: phase 0 writes this rank's pivot / shards into `pivot`
 * ((M / rows_per_group) x G floats) and the caller adds them over the ranks (all-reduce SUM); phase 1 writes this rank's
 * partial sums about the agreed pivot into `stats`; the caller adds the first
 * anyv2v_groupnorm_partial_floats(M, rows_per_group, G, C0 + C1) floats over the ranks (all-reduce SUM: RCCL on the
 * node); phase 2 normalises with the agreed pivot and shards x the local element count.
 * pivot(shards = 1) + partial_pivot + apply_pivot(shards = 1) on one rank is exactly anyv2v_groupnorm_f16. */
int64_t anyv2v_groupnorm_partial_floats(int32_t M, int32_t rows_per_group, int32_t G, int32_t C);
int anyv2v_groupnorm_pivot_f16(const void* X0, const void* X1, int32_t C0, int32_t C1, float* pivot, int32_t M,
                               int32_t rows_per_group, int32_t G, int32_t shards, void* stream);
int anyv2v_groupnorm_partial_pivot_f16(const void* X0, const void* X1, int32_t C0, int32_t C1, const float* pivot,
                                       float* stats, int32_t M, int32_t rows_per_group, int32_t G, void* stream);
int anyv2v_groupnorm_apply_pivot_f16(const void* X0, const void* X1, int32_t C0, int32_t C1, void* Y, const void* gamma,
                                     const void* beta, const float* pivot, const float* stats, int32_t M,
                                     int32_t rows_per_group, int32_t G, float eps, int32_t silu, int32_t shards, void* stream);
/* The pre-104 sharded pair, kept for existing callers: ONE all-reduce (of the partial sums), i.e. the pivot fixed at 0 --
 * unshifted sums, which lose precision once a group's |mean| is large against its spread (hundreds of sigma). */
int anyv2v_groupnorm_partial_f16(const void* X0, const void* X1, int32_t C0, int32_t C1, float* stats, int32_t M,
                                 int32_t rows_per_group, int32_t G, void* stream);
int anyv2v_groupnorm_apply_f16(const void* X0, const void* X1, int32_t C0, int32_t C1, void* Y, const void* gamma,
                               const void* beta, const float* stats, int32_t M, int32_t rows_per_group, int32_t G,
                               float eps, int32_t silu, int32_t shards, void* stream);

/* LayerNorm over the last dim (BasicTransformerBlock.norm1/2/3). */
int anyv2v_layernorm_f16(const void* X, void* Y, const void* gamma, const void* beta, int32_t M, int32_t C,
                         float eps, void* stream);

/* ---- attention -------------------------------------------------------------------------------
 * softmax(Q K^T / sqrt(64)) V for head_dim 64, no mask -- F.scaled_dot_product_attention at
 * i2vgen-xl/pnp_utils.py:208-210 (spatial) and :314-316 (temporal).
 * Batch element i (0 <= i < batch), sequence position s, head h address row
 *     row = (i / inner) * outer_stride + (i % inner) * inner_stride + s * seq_stride
 * of a token matrix with leading dim ld; head h occupies columns [64 h, 64 h + 64).
 *   spatial : inner = 1,  outer_stride = S,    seq_stride = 1
 *   temporal: inner = HW, outer_stride = F*HW, inner_stride = 1, seq_stride = HW   (no permute needed)
 * K/V use batch index i / kv_div (cross-attention: all F frames of a clip share one K/V).
 * PnP injection (pnp_utils.py:189-196, :295-302): qk_mod > 0 makes Q and K of batch element i come
 * from element i % qk_mod (the source branch) -- aliasing instead of the reference's copies.
 * Strides are 64-bit and every kernel forms row addresses in 64 bits, with one limit: the flash kernels (Sq or Sk > 16) hold the
 * byte offsets of the 64 key rows of a K / V tile in 32 bits, so they run only while
 *     (63 * kv_seq * max(ldk, ldv) + 64) * 2 < 2^32      (kv_seq * ld below about 34.1 M elements; kv_seq >= 0).
 * A launch beyond that limit is not an error: it runs on the 96-key loop kernel of anyv2v_attention_small_f16 (64-bit addressing
 * throughout, same strides / kv_div / qk_mod; several times slower), or on the one-thread-per-query kernel when batch or heads
 * exceed 65535.  Same result within the kernels' rounding, not bit for bit; flags bit2, bit3 and bit7 select among the flash
 * kernels' forms only and mean nothing there.  Leading dimensions must be positive (ANYV2V_EINVAL otherwise).
 */
typedef struct AnyV2VAttnDesc {
    const void* Q;
    const void* K;
    const void* V;
    void* O;
    int32_t ldq, ldk, ldv, ldo;
    int32_t batch, heads, Sq, Sk;
    int32_t inner;
    int64_t q_outer, q_inner, q_seq;     /* strides in rows */
    int64_t kv_outer, kv_inner, kv_seq;
    int32_t kv_div;
    int32_t qk_mod;
    float scale;
    int32_t flags;      /* bit0: force the naive reference kernel; bit1: no short-sequence kernel; bit2: never use the
                           8-wave (256-query) blocks; bit3: PnP launches (batch == 3 qk_mod) as per-branch aliasing on the
                           plain kernel instead of the shared-softmax kernel; bit7 (128): 8-byte instead of 16-byte epilogue stores in
                           the flash kernels (A/B of the widened epilogue; same bytes, same results).  All other bits are ignored. */
} AnyV2VAttnDesc;

int anyv2v_attention_f16(const AnyV2VAttnDesc* d, void* stream);

/* Attention for any head_dim <= 160, used once per clip (and by the ConsistI2V hook family's temporal attention, head_dim = C / 8): image_latents_temporal_encoder (2 heads x dim 4) and the CLIP towers of
 * encode_prompt / _encode_image (pipeline_i2vgen_xl.py:224-441: text 16 heads x 64 with the causal mask, vision 16 heads x 80).
 * head_dim a multiple of 8 in 40..128 and Sk <= 288, or in 136..160 and Sk <= 96: a whole-sequence MFMA kernel (K and V^T of a
 * head in LDS, exact softmax over the score row block in registers); anything else, or flags bit0: one thread per (batch, head, query).  Same addressing as above
 * with explicit head_dim; flags bit4 (16): causal mask (key j visible to query s iff j <= s). */
int anyv2v_attention_small_f16(const AnyV2VAttnDesc* d, int32_t head_dim, void* stream);
/* The same with an additive score bias: softmax(scale * Q K^T + bias[head]) V, bias fp32 [heads, Sq, Sk] shared by all batch
 * elements -- SEINE's TemporalAttention adds a learned relative-position bias to the temporal scores
 * (seine/models/attention.py:815-817,870-889; seine/pnp_utils.py:386-451 is its hooked form).  Generic kernel, head_dim <= 160. */
int anyv2v_attention_bias_f16(const AnyV2VAttnDesc* d, int32_t head_dim, const float* bias, void* stream);

/* Temporal self-attention with its LayerNorm-folded QKV projection inside (plain form: every batch element attends with its own
 * Q and K): O = attention(QKV) with QKV = rstd (X W^T - mean ln_c1) + bias as anyv2v_gemm_f16 computes it with ln_c1 set, for the token
 * matrix X [(B F) HW][ldx] of TransformerTemporalModel: sequence (b, pixel) is rows b F HW + pixel + f HW, f = 0..F-1.  W [3 C][C] =
 * [Wq; Wk; Wv] diag(gamma) (fp16), bias [3 C] (fp16), ln_c1 [3 C] (fp32) as for AnyV2VGemmDesc; head h reads rows 64 h .. 64 h + 63 of
 * each third and writes columns [64 h, 64 h + 64) of O [(B F) HW][ldo].  The [rows, 3 C] QKV tensor is never written.  Bit for bit the
 * result of anyv2v_gemm_f16 (weight-stationary LayerNorm-fold kernel) followed by anyv2v_attention_f16 (temporal strides) on the same
 * operands; a row's result does not depend on what else is in the launch.  Implemented for F = 16, C = 320, heads = 5 (head_dim 64),
 * even HW; anything else returns ANYV2V_EUNSUPPORTED and the caller runs the two launches.  X, O, W, ln_c1 16-byte aligned, bias
 * 8-byte aligned, ldx and ldo multiples of 8. */
typedef struct AnyV2VTattnDesc {
    const void* X;
    const void* W;
    const void* bias;
    const float* ln_c1;
    void* O;
    int32_t B, F, HW;
    int32_t C, heads;
    int32_t ldx, ldo;
    float ln_eps;
    float scale;         /* softmax scale, 1 / sqrt(64) */
    int32_t flags;       /* reserved, 0 */
} AnyV2VTattnDesc;

int anyv2v_temporal_qkv_attn_f16(const AnyV2VTattnDesc* d, void* stream);

/* ---- elementwise / layout --------------------------------------------------------------------- */
/* y = silu(x) (n elements) */
int anyv2v_silu_f16(const void* X, void* Y, int64_t n, void* stream);
/* y = a + b */
int anyv2v_add_f16(const void* A, const void* B, void* Y, int64_t n, void* stream);
/* sinusoidal timestep embedding, flip_sin_to_cos, freq shift 0: out[b, :] = [cos(t_b w) | sin(t_b w)] */
int anyv2v_timestep_embedding_f16(const float* t, void* out, int32_t B, int32_t dim, void* stream);
/* [B, C, F, H, W] (NCFHW, the pipeline's latent layout) -> tokens [(B F) (H W), ldy] at column col0 */
int anyv2v_ncfhw_to_tokens_f16(const void* X, void* Y, int32_t B, int32_t C, int32_t F, int32_t HW, int32_t ldy,
                               int32_t col0, void* stream);
int anyv2v_tokens_to_ncfhw_f16(const void* X, void* Y, int32_t B, int32_t C, int32_t F, int32_t HW, int32_t ldx,
                               int32_t col0, void* stream);
/* AdaptiveAvgPool2d over channels-last tokens [N, Hi, Wi, C] -> [N, Ho, Wo, C] */
int anyv2v_adaptive_avgpool_f16(const void* X, void* Y, int32_t N, int32_t Hi, int32_t Wi, int32_t Ho, int32_t Wo,
                                int32_t C, void* stream);
/* Row gather with column windows: Y[m, ycol0 : ycol0+C] = X[idx[m], xcol0 : xcol0+C] (idx: int32 on the device; C, ld, col0
 * multiples of 8).  Builds the key / value sequences of ConsistI2V's first-frame-conditioned attention without a second
 * projection: spatial attn1 attends over [own frame ; first frame] (videoldm_transformer_blocks.py:479-489), temporal attn1 over
 * [the pixel's frames ; the 8 neighbours of the pixel in the first frame] (:490-503, videoldm_attention.py:589-599) -- both are
 * rows of the K / V projections that already exist. */
int anyv2v_gather_rows_f16(const void* X, int32_t ldx, int32_t xcol0, const int32_t* idx, void* Y, int32_t ldy, int32_t ycol0,
                           int64_t M, int32_t C, void* stream);
/* Rotary position embedding in place (consisti2v/consisti2v/models/rotary_embedding.py:29-49,143-163 as called by
 * RotaryEmbAttnProcessor2_0 / ModifiedTmpAttnProcessor, videoldm_attention.py:773-777, consisti2v/pnp_utils.py:306-310):
 * columns [col0 + w * window_stride, ... + rot_dim) of row r for w < n_windows, in interleaved pairs (2i, 2i+1), rotated by
 * pos(r) * theta^(-2i/rot_dim) with pos(r) = (r / rows_per_pos) % n_pos -- for token matrices [(b f)(h w), C]: rows_per_pos = HW,
 * n_pos = F.  ConsistI2V rotates ONE window (the first half of the channels, before the head split); SEINE rotates the first 32
 * channels of EVERY head (seine/models/attention.py:880-882, RotaryEmbedding(32) on [b, heads, f, d]): n_windows = heads,
 * window_stride = head_dim.  fp32 angles. */
int anyv2v_rotary_f16(void* X, int32_t ld, int64_t rows, int32_t col0, int32_t rot_dim, int32_t n_windows, int32_t window_stride,
                      int32_t rows_per_pos, int32_t n_pos, float theta, void* stream);
/* rows copy with column window: Y[m, ycol0 : ycol0+C] = X[m, xcol0 : xcol0+C] */
int anyv2v_copy_cols_f16(const void* X, int32_t ldx, int32_t xcol0, void* Y, int32_t ldy, int32_t ycol0, int64_t M,
                         int32_t C, void* stream);

/* FreeU (arXiv 2309.11497; the reference pipeline forwards enable_freeu to its UNet, pipeline_i2vgen_xl.py:623-648) on the pair of
 * token matrices [n_img H W, C] (rows ordered (image, h, w)) that an up block concatenates, out of place:
 *   hidden_out[:, c] = fp16(float(hidden[:, c]) * b) for c < C_hidden / 2, a copy for the other half;
 *   skip_out = per (image, channel) plane [H, W], in fp32, rounded once: fftn -> fftshift -> the 2 x 2 box
 *              [H/2-1 : H/2+1, W/2-1 : W/2+1] times s -> ifftshift -> ifftn -> real.  The box holds the frequencies {0, -1} of each
 *              axis ({0} on an axis of size 1), so the filter is evaluated in closed form -- seven sums per plane and a rank-4
 *              correction, no FFT (DESIGN.md "FreeU").  No atomics: bit-reproducible, and independent of n_img.
 * C_hidden, C_skip and the leading dimensions are multiples of 8, every pointer is 16-byte aligned, H + W <= 4096. */
int anyv2v_freeu_f16(const void* hidden, int32_t ld_hidden, void* hidden_out, int32_t ld_hidden_out, int32_t C_hidden, float b,
                     const void* skip, int32_t ld_skip, void* skip_out, int32_t ld_skip_out, int32_t C_skip, float s,
                     int32_t n_img, int32_t H, int32_t W, void* stream);

/* Stitch of the tiled AutoencoderKL encode / decode (diffusers-0.26.3 tiled_encode / tiled_decode / blend_v / blend_h behind the reference's
 * enable_vae_tiling, pipeline_i2vgen_xl.py:208-221): gathers the planar image out[n_img, C, H, W] (fp16) from the RAW tiles, channels-last
 * token matrices inside `tiles` [tile_rows, ld] (C <= 8 channels used, ld % 8 == 0, 16-byte aligned).  The definition blends in place in
 * row-major tile order (with the tile above, then with the tile on the left, each already blended) and keeps tile[:limit, :limit]; unrolled:
 *   out[n, c, y, x] = wy wx R[py, px] + wy (1 - wx) L[py, qx] + (1 - wy) wx^2 U[qy, px] + (1 - wy)(1 - wx^2) UL[qy, qx]
 * R / L / U / UL = raw tiles (ky, kx), (ky, kx - 1), (ky - 1, kx), (ky - 1, kx - 1) of image n, (ky, py, qy) = row table [y], wy = row
 * weight [y] (p / e' inside a blend band, 1 outside, where the q entry and the tiles it selects are not read), columns likewise.
 * Four products and their sum in fp64, ONE rounding to fp16 (exact, hence bit-equal to the sequential definition, when e' is a power
 * of two); a pixel outside every band is copied.  Every output element is written exactly once.
 *   plan  int32: [nty * ntx][4] tile records {first row of image 0 in `tiles`, height, width, 0} (image n of a tile follows image n - 1),
 *                then [H][3] rows {k, p, q}, then [W][3] columns {k, p, q};      weight  fp64: [H] wy, then [W] wx.
 * Both tables are passed twice: the host copy, which the entry point checks against tile_rows and the tile extents before it launches
 * (ANYV2V_EINVAL), and the device copy of the SAME values, which the kernel reads. */
int anyv2v_tile_blend_f16(const void* tiles, int64_t tile_rows, int32_t ld, int32_t C, const int32_t* plan_host,
                          const double* weight_host, const int32_t* plan_dev, const double* weight_dev, int32_t nty, int32_t ntx,
                          void* out, int32_t n_img, int32_t H, int32_t W, void* stream);

/* Row softmax of fp32 logits (from anyv2v_gemm_f16 with act = 4) into fp16 probabilities:
 * P[r, c] = softmax_c(scale * S[r, c]), cols <= 8192.  AutoencoderKL mid-block attention (single head of width 512,
 * encode_vae_video / decode_latents, pipeline_i2vgen_xl.py:565-592,598-620). */
int anyv2v_softmax_rows_f32_f16(const float* S, int32_t lds, void* P, int32_t ldp, int32_t rows, int32_t cols, float scale,
                                void* stream);

/* Fused classifier-free-guidance combine + DDIM step (eta = 0, v-prediction), reading the UNet's
 * channels-last v-prediction tokens directly and updating NCFHW latents in place:
 *   v = v_unc + g * (v_cond - v_unc)                              pipeline_i2vgen_xl.py:1160-1162
 *   x0 = sa_t x - sb_t v ; eps = sa_t v + sb_t x ; x' = sa_p x0 + sb_p eps   (DDIMScheduler.step, :1173;
 *   inverse: consisti2v/ddim_inverse_scheduler.py:329-369 -- same formula, different alphas)
 * Vtok: [(nb F) HW, ldv] tokens; branch `b_unc` / `b_cond` select the batch slices (b_unc < 0: no CFG).
 * coef: 4 floats on the device {sa_t, sb_t, sa_p, sb_p}.  lat/out: [1, C, F, H, W] fp16; out may alias lat.
 */
int anyv2v_cfg_ddim_step_f16(const void* Vtok, int32_t ldv, int32_t b_unc, int32_t b_cond, float guidance,
                             const float* coef, const void* lat, void* out, int32_t C, int32_t F, int32_t HW,
                             void* stream);

/* Statistics for the guidance rescale (Lin et al. 3.4; rescale_noise_cfg, consisti2v/consisti2v/pipelines/pipeline_video_editing.py:50-61,
 * replaces its two `.std()` reductions, :55-56) of ONE clip's prediction, read from the same tokens anyv2v_cfg_ddim_step_f16 reads:
 * the text branch e_txt = Vtok[b_cond] and the guided prediction g = fp16(e_unc + fp16(G * fp16(e_txt - e_unc))), n = C F HW elements
 * each.  A fixed grid of ANYV2V_GUIDANCE_STATS_BLOCKS blocks x ANYV2V_GUIDANCE_STATS_THREADS threads strides over the F HW pixels;
 * block b writes record b, ANYV2V_GUIDANCE_STATS_RECORD floats {S_txt, Q_txt, S_cfg, Q_cfg, K_txt, K_cfg, 0, 0} with S = sum(x - K),
 * Q = sum((x - K)^2) in fp32 about the pivot K = the tensor's first element.  No atomics, nothing depends on the device: the
 * records are bit-reproducible.  records: ANYV2V_GUIDANCE_STATS_BLOCKS * ANYV2V_GUIDANCE_STATS_RECORD floats, 16-byte aligned; b_unc >= 0. */
#define ANYV2V_GUIDANCE_STATS_BLOCKS 64
#define ANYV2V_GUIDANCE_STATS_THREADS 256
#define ANYV2V_GUIDANCE_STATS_RECORD 8
int anyv2v_guidance_stats_f16(const void* Vtok, int32_t ldv, int32_t b_unc, int32_t b_cond, float guidance, float* records,
                              int32_t C, int32_t F, int32_t HW, void* stream);

/* anyv2v_cfg_ddim_step_f16 with the sampler options of the reference's call (pipeline_i2vgen_xl.py:868,1173 `scheduler.step(noise_pred,
 * t, latents, **extra_step_kwargs)` with eta > 0 -- seine/diffusion/gaussian_diffusion.py:583-599 is the in-tree statement of that
 * step -- and pipeline_video_editing.py:685-688 `rescale_noise_cfg(noise_pred, noise_pred_text, guidance_rescale)`):
 *   g  as above (b_unc < 0: e_txt);   g' = fp16(g * s), s = phi * std_txt / std_cfg + (1 - phi), when phi > 0 and b_unc >= 0, else g
 *   x0 / eps from g' by `prediction` (0 v_prediction, 1 epsilon, 2 sample; as anyv2v_guided_step_f16)
 *   out = fp16(c_x0 * x0 + c_eps * eps + sigma * noise)          one rounding
 * row: 8 floats on the device {sa_t, sb_t, c_x0, c_eps, sigma, phi, n, 0} (n = C F HW), rewritten per step by the host.  Every block
 * folds the records of anyv2v_guidance_stats_f16 in fp64, in record order, into the unbiased standard deviations (n - 1, torch.std).
 * `phi` is the host's copy of row[5], checked here (0 <= phi <= 1; phi > 0 with guidance needs `records` and n >= 2); records may be
 * NULL when phi == 0, noise (planar fp16 like lat) may be NULL when sigma is 0 for the whole run.  The caller keeps epsilon prediction
 * away from sa_t = 0 and sample prediction from sb_t = 0 (the row lives on the device).  With phi = 0 and sigma = 0 and v-prediction
 * the result equals anyv2v_cfg_ddim_step_f16's bit for bit.  lat/out: [1, C, F, H, W] fp16; out may alias lat. */
int anyv2v_cfg_ddim_step_ex_f16(const void* Vtok, int32_t ldv, int32_t b_unc, int32_t b_cond, float guidance, int32_t prediction,
                                const float* row, const float* records, float phi, const void* noise, const void* lat, void* out,
                                int32_t C, int32_t F, int32_t HW, void* stream);

/* Masked PnP editing -- the source clip kept outside an edit mask.  Nothing in the reference does this; the technique is the latent
 * blending of Blended Latent Diffusion (arXiv 2206.02779) and of diffusers' 4-channel inpaint loop, which these two entry points replace:
 *   init_mask = torch.nn.functional.interpolate(mask, size=(height // vae_scale_factor, width // vae_scale_factor))
 *   latents = (1 - init_mask) * init_latents_proper + init_mask * latents       (pipeline_stable_diffusion_inpaint.py, prepare_mask_latents
 *                                                                                and the end of the denoising loop's body)
 * with the inverted latent of the source (the resident trajectory) in the place of the re-noised `init_latents_proper`.
 *
 * anyv2v_latent_mask_f16: pixel mask [mask_frames, H, W] fp16 in [0, 1] (1 = edit, 0 = keep; clamped, NaN counts as 0) -> latent mask
 * out [mask_frames, H / 8, W / 8] fp16.  Three stages in fp32, ONE rounding to fp16 at the end, one launch per stage that is on:
 *   1. pool    the mean over each 8 x 8 block: the 64 values are summed exactly (integers in units of 2^-24) and the sum is rounded to
 *              fp32 once -- the correctly rounded mean; a binary mask gives k / 64 exactly;
 *   2. grow    (grow > 0) the maximum over the (2 grow + 1)^2 window, positions outside the image ignored; 0 <= grow <= ANYV2V_MASK_MAX_GROW;
 *   3. feather (R > 0) separable Gaussian with replicate padding, out[y, x] = sum_j t[j] (sum_i t[i] in[y + j, x + i]) by fmaf in tap
 *              order; taps: 2 R + 1 floats ON THE HOST (exp(-k^2 / (2 sigma^2)) / sum in fp64, rounded to fp32; R = ceil(3 sigma)),
 *              checked here and handed to the kernel by value; 0 <= R <= ANYV2V_MASK_MAX_RADIUS.  A window wider than the image is fine.
 * workspace: 2 * mask_frames * (H / 8) * (W / 8) floats on the device.  No atomics.  Runs once per clip, outside any captured graph.
 *
 * anyv2v_masked_blend_f16: x / src / out [1, C, F, HW] fp16, mask [mask_frames, HW] fp16 (mask_frames 1 or F; broadcast over C, and over
 * F when 1); per element, with m the mask value:
 *   m == 0 -> src      m == 1 -> x      (selects: the dropped operand may hold Inf / NaN)      else fp16(fmaf(m, x - src, src)) in fp32
 * out may alias x (the step engines blend the latent slot in place), nothing else.  16-byte accesses when HW % 8 == 0 and all four
 * pointers are 16-byte aligned, a scalar kernel otherwise -- chosen here, on the host. */
#define ANYV2V_MASK_MAX_GROW 8
#define ANYV2V_MASK_MAX_RADIUS 24
int anyv2v_latent_mask_f16(const void* mask, int32_t mask_frames, int32_t H, int32_t W, int32_t grow, const float* taps, int32_t R,
                           float* workspace, void* out, void* stream);
int anyv2v_masked_blend_f16(const void* x, const void* src, const void* mask, int32_t mask_frames, void* out, int32_t C, int32_t F,
                            int32_t HW, void* stream);

/* Automatic edit masks for the masked edit -- where do the UNet's predictions under the source and under the edit conditioning differ?
 * Nothing in the reference does this; the method is DiffEdit's (Couairon et al., arXiv 2210.11427), these two entry points replace the
 * tail of diffusers' StableDiffusionDiffEditPipeline.generate_mask:
 *   mask_guidance_map = torch.abs(noise_pred_target - noise_pred_source).reshape(b, num_maps_per_mask, *shape).mean([1, 2])
 * followed by its normalisation by the map's mean, the scaling by mask_thresholding_ratio, the clamp to [0, 1] and the threshold -- here as
 *   map = clamp(ratio * map / mean(map), 0, 1);   mask = map > threshold
 * with ONE mean over the whole clip (a frame in which nothing changes comes out empty), for a video UNet's [F, h, w] maps.  The factor
 * 1 / (N C) of the two means cancels in the normalisation, so the accumulator holds plain sums.
 *
 * anyv2v_diff_map_accum_f16: Vtok [2 F HW, ldv] fp16, the UNet's token-layout output of the batch [source, edit]: rows [0, F HW) the
 * source branch, rows [F HW, 2 F HW) the edit branch, the C channels in the first columns of a row (columns C .. ldv - 1 are never read).
 *   s[p] = sum_c |V_tgt[p, c] - V_src[p, c]|    the difference and its absolute value exact in fp32, channels added in the order 0 .. C - 1
 *   acc[p] = first ? s[p] : acc[p] + s[p]       fp32 [F HW]
 * `first` (0 / 1) is the host's flag; first_dev, when not NULL, points at ONE int32 on the device that is read instead -- a captured graph
 * then serves the first map and every further one.  One thread per pixel, no atomics, each element written once per launch.
 *
 * anyv2v_diff_map_finish_f16: acc fp32 [F, h, w] -> map fp16 [F, h, w] and pixel_mask uint8 [F, 8 h, 8 w] (0 / 1: torch.bool's layout).
 *   mean = sum(acc) / (F h w): a fixed grid of ANYV2V_DIFF_MAP_BLOCKS x ANYV2V_DIFF_MAP_THREADS threads writes one fp32 partial sum per
 *          block into `records` (ANYV2V_DIFF_MAP_BLOCKS floats); every consumer folds them in fp64 in record order -- bit-reproducible;
 *   map  = fp16(clamp(acc * fp32(ratio / mean), 0, 1)), one rounding to fp16; mean == 0 (identical conditionings): map = 0, no NaN;
 *   mask = map > fp16(threshold), compared on the ROUNDED map, each latent pixel replicated over its 8 x 8 pixel block.
 * ratio finite and > 0, threshold in (0, 1).  16-byte accesses when w % 8 == 0 and acc / map / pixel_mask are 16-byte aligned, a scalar
 * kernel otherwise -- chosen here, on the host.  Two launches (partial sums, finish), no atomics. */
#define ANYV2V_DIFF_MAP_BLOCKS 64
#define ANYV2V_DIFF_MAP_THREADS 256
int anyv2v_diff_map_accum_f16(const void* Vtok, int32_t ldv, int32_t C, int32_t F, int32_t HW, float* acc, int32_t first,
                              const int32_t* first_dev, void* stream);
int anyv2v_diff_map_finish_f16(const float* acc, int32_t F, int32_t h, int32_t w, float ratio, float threshold, float* records, void* map,
                               void* pixel_mask, void* stream);

/* Pixel-space composite behind the VAE decode of a masked edit: outside the edit region the frames written are the source's bytes, not
 * decode(encode(source)).  Nothing in the reference does this (the pixel-space finish of Blended Latent Diffusion, arXiv 2206.02779;
 * diffusers' apply_overlay).  Three entry points, no atomics, every output element written once by one thread.
 *
 * anyv2v_pixel_alpha_f16: latent mask fp16 [Fm, h, w] (what anyv2v_latent_mask_f16 wrote: alpha follows the region the latent blend
 * used) -> alpha fp32 [Fm, 8 h, 8 w].
 *   base(f, y, x) = lm(f, y / 8, x / 8) > 0     the support: a softly blended latent cell is neither source nor edit, it shows the decode
 *   core = dilate(base, grow_px), wide = dilate(base, grow_px + R)     square-window maxima, positions outside the image ignored
 *   a    = G * wide     separable: the row pass first, then the column pass, each in tap order in fp32 with fmaf, replicate padding
 *   alpha = core ? 1.0f : min(a, 1.0f)
 * so alpha is exactly 1 on the grown support, exactly 0 beyond grow_px + 2 R of it (the taps are >= 0 and the inputs 0 there) and falls
 * off continuously in between.  R == 0: the hard mask, alpha = core.  grow_px in [0, ANYV2V_COMPOSITE_MAX_GROW], R in
 * [0, ANYV2V_COMPOSITE_MAX_RADIUS], taps = 2 R + 1 weights in [0, 1] (NULL when R == 0) on the HOST, copied into the launch.
 * Dilation and feather are separable two-pass kernels, O(grow_px + R) per output.  workspace: 2 * Fm * 8 h * 8 w floats.
 *
 * anyv2v_composite_stats_u8: the statistics of the colour match over the KEPT region (alpha == 0), per channel, per clip (a per-frame gain
 * would flicker).  video fp16 [1, 3, F, H, W] (the decode's output, in [-1, 1]), source uint8 [F, H, W, 3], alpha fp32 [Fm, H, W], Fm 1 or
 * F.  e = the byte vae.to_pil forms from the video value (below), s = the source byte.  A fixed grid of ANYV2V_COMPOSITE_STATS_BLOCKS
 * blocks writes one record of ANYV2V_COMPOSITE_STATS_RECORD int64 each: for channel c at [5 c .. 5 c + 4] count, sum e, sum e^2, sum s,
 * sum s^2, [15] = 0.  Exact integer sums: independent of the order, bit-reproducible.
 *
 * anyv2v_composite_u8: out uint8 [F, H, W, 3].  Per element
 *   e   = the level ((v + 1.0) * 127.5).round().clamp(0, 255) of an fp16 tensor: sum and product each rounded to fp16, round-half-even;
 *         NaN -> 0, +Inf -> 255, -Inf -> 0 (the bytes vae.to_pil writes for the same value)
 *   out = alpha == 0 ? s : alpha == 1 ? e : rint(fmaf(alpha, e - s, s))     selects, never multiplies: a kept pixel is the source's byte
 *         whatever the decode holds, a fully edited pixel is the byte written without the composite
 * records != NULL (the colour match): every block folds the records in record order and forms per channel, in fp64,
 *   mean = sum / count, var = max(sum2 / count - mean^2, 0), gain = clamp(sqrt(var_s) / sqrt(var_e), 0.5, 2), bias = mean_s - gain mean_e,
 * both rounded to fp32; the identity (1, 0) when count < 64 or var_e == 0.  e' = clamp(fmaf(gain, e, bias), 0, 255) stands in for e
 * wherever alpha > 0 and the result is rounded once, by the rint at the end.
 * 4 pixels per thread when H W % 4 == 0 and video / alpha / source / out are 8 / 16 / 4 / 4-byte aligned, a scalar kernel otherwise --
 * chosen here, on the host.  out may not alias an input. */
#define ANYV2V_COMPOSITE_MAX_GROW 64
#define ANYV2V_COMPOSITE_MAX_RADIUS 48
#define ANYV2V_COMPOSITE_STATS_BLOCKS 256
#define ANYV2V_COMPOSITE_STATS_RECORD 16
int anyv2v_pixel_alpha_f16(const void* latent_mask, int32_t mask_frames, int32_t h, int32_t w, int32_t grow_px, const float* taps, int32_t R,
                           float* workspace, float* alpha, void* stream);
int anyv2v_composite_stats_u8(const void* video, const void* source, const float* alpha, int32_t mask_frames, int32_t F, int32_t H, int32_t W,
                              int64_t* records, void* stream);
int anyv2v_composite_u8(const void* video, const void* source, const float* alpha, int32_t mask_frames, const int64_t* records, void* out,
                        int32_t F, int32_t H, int32_t W, void* stream);

/* Mask tracking (track.hip): carry a frame-0 pixel mask through the clip along block-matched motion of the SOURCE frames (full-search
 * block matching; nothing in the reference does this).  All integers, so every result is defined bit for bit.  Frames are uint8
 * [F, H, W, 3] with H % 8 == 0, W % 8 == 0, F >= 1; cells are the 8 x 8 pixel blocks of the latent grid, h = H / 8, w = W / 8; clamp()
 * clamps a pixel coordinate into the frame (replicate border).
 *
 * anyv2v_luma_u8: Y = (77 R + 150 G + 29 B + 128) >> 8, uint8 [F, H, W].
 *
 * anyv2v_block_match_u8: flow int16 [F, h, w, 2], ordered (dy, dx).  For frame k >= 1 and cell (cy, cx) the window is the 16 x 16 pixels
 * centred on the cell (the cell plus 4 pixels on each side).  For every integer d = (dy, dx) in [-radius, radius]^2
 *   cost(d) = sum over p in the window of |Y_k[clamp(p)] - Y_{k-1}[clamp(p + d)]|        (<= 65 280)
 * and D_k[cy, cx] is the d that minimises the tuple (cost, dy^2 + dx^2, dy, dx) in lexicographic order: ties go to the shortest vector, so
 * a flat or periodic region stays at zero displacement.  D_0 = 0; radius in [0, ANYV2V_TRACK_MAX_RADIUS], radius 0 gives all zeros.
 * One block per 4 x 4 cells: Y_{k-1} with its halo staged in LDS already clamped, four pixels per v_sad_u8, an odd dx by byte-align
 * operations on the same five dwords (identically for every dx), the winner by an integer key minimum -- no atomics, no floating point.
 *
 * anyv2v_flow_median_i16: every component replaced by the median of its 3 x 3 cell neighbourhood, replicate border, per frame; out may
 * not alias the input.
 *
 * anyv2v_mask_propagate_u8: mask_0 uint8 [H, W] (non-zero = set) -> out uint8 [F, H, W] of 0 / 1 with
 *   mask_k[p] = mask_{k-1}[clamp(p + D_k[cell(p)])],
 * evaluated in one launch, one thread per output pixel: q = p; for j = k .. 1: q = clamp(q + D_j[cell(q)]); out = mask_0[q] != 0 (equal
 * to the frame-after-frame warp by induction on k).  Any int16 flow is safe: every step is clamped into the frame.
 *
 * anyv2v_first_frame_mask_u8: source, edited uint8 [H, W, 3] -> mask uint8 [H, W] of 0 / 1, constant on cells:
 *   changed[p] = max over c of |edited[p, c] - source[p, c]| > threshold      (strict; threshold in [0, 255])
 *   a cell is set when at least min_count (1 .. 64) of its 64 pixels changed. */
#define ANYV2V_TRACK_MAX_RADIUS 32
int anyv2v_luma_u8(const void* frames, void* luma, int32_t F, int32_t H, int32_t W, void* stream);
int anyv2v_block_match_u8(const void* luma, void* flow, int32_t F, int32_t H, int32_t W, int32_t radius, void* stream);
int anyv2v_flow_median_i16(const void* flow, void* out, int32_t F, int32_t h, int32_t w, void* stream);
int anyv2v_mask_propagate_u8(const void* mask0, const void* flow, void* out, int32_t F, int32_t H, int32_t W, void* stream);
int anyv2v_first_frame_mask_u8(const void* source, const void* edited, void* mask, int32_t H, int32_t W, int32_t threshold,
                               int32_t min_count, void* stream);

/* Resampling of 8-bit frames (resample_plan.cpp, resample.hip): Pillow's `Image.resize` for 8-bit bands (its ImagingResample), which
 * works in fixed point, so every byte is defined and the kernels are tested bit for bit against Pillow itself.  Two separable passes,
 * horizontal first, with a uint8 intermediate image; a pass is skipped when that side's output size equals its input size and its box
 * is the whole side (the caller decides; each entry below is one pass).
 *
 * anyv2v_resample_table: the table of one side.  in_size pixels, box [in0, in1) in source pixels, out_size outputs, a filter with its
 * `support`.  All of this in IEEE double, no fused multiply-add:
 *   scale = (in1 - in0) / out_size;  fs = max(scale, 1.0);  sup = support * fs;  ss = 1.0 / fs;  ksize = (int)ceil(sup) * 2 + 1
 * and for output xx
 *   center = in0 + (xx + 0.5) * scale
 *   xmin = max((int)(center - sup + 0.5), 0);   n = min((int)(center + sup + 0.5), in_size) - xmin
 *   w[x] = filter((x + xmin - center + 0.5) * ss) for x < n;   ww = sum of w[x], left to right;   w[x] /= ww when ww != 0
 *   k[x] = (int)(w[x] * 2^22 + 0.5) for w[x] >= 0, (int)(w[x] * 2^22 - 0.5) otherwise
 * Filters (the numbers are Pillow's `Image.Resampling` values):
 *   ANYV2V_RESAMPLE_BOX       support 0.5: 1 for -0.5 < x <= 0.5
 *   ANYV2V_RESAMPLE_BILINEAR  support 1: 1 - |x|
 *   ANYV2V_RESAMPLE_BICUBIC   support 2: Keys' kernel with a = -0.5, as ((a + 2) |x| - (a + 3)) |x| |x| + 1 below 1 and
 *                             (((|x| - 5) |x| + 8) |x| - 4) a below 2
 *   ANYV2V_RESAMPLE_LANCZOS   support 3: sinc(x) sinc(x / 3) for -3 <= x < 3, sinc(x) = sin(pi x) / (pi x), sinc(0) = 1
 * Returns ksize.  With bounds == NULL or coeffs == NULL it only returns ksize; otherwise it fills bounds[out_size][2] = (xmin, n) and
 * coeffs[out_size][ksize] = k, zero past n.  A negative status (text: anyv2v_last_error()) for sides outside 1 .. ANYV2V_RESAMPLE_MAX_SIDE,
 * a box that is empty or not inside [0, in_size] (in1 may pass in_size by one float ulp, in_size * 2^-23: Pillow forms the width of a
 * float box in float, and in0 + width can land there), an unknown filter, or a table with a row of sum |k[x]| >= 2 * 2^22: below that,
 * 255 * sum |k| + 2^21 < 2^31 and the kernels' int32 accumulator cannot overflow.  Host code only, no GPU is touched.
 *
 * An output sample of either pass, per band:   acc = 2^21 + sum over x < n of in[xmin + x] * k[x]   (int32)
 *                                              out = clamp(acc >> 22, 0, 255)                        (arithmetic shift)
 *
 * anyv2v_resample_h_u8: src uint8 [F, H, W, C] -> dst uint8 [F, rows, out_w, C], the horizontal pass over the input rows
 * [row0, row0 + rows) only (the rows a following vertical pass reads).  anyv2v_resample_v_u8: src [F, H, W, C] -> dst [F, out_h, W, C].
 * C is 1 or 3; bounds int32 [out][2] and coeffs int32 [out][ksize] are DEVICE copies of a table as anyv2v_resample_table writes it (4-byte
 * aligned); a window of the output is a slice of the table's rows.  src and dst need no alignment and may not overlap.  A table entry
 * that points outside the side is cut to it (no read leaves src).  Element offsets are 64-bit; F <= 65535.  No atomics, a fixed grid:
 * every output byte is written once, by one thread. */
#define ANYV2V_RESAMPLE_LANCZOS 1
#define ANYV2V_RESAMPLE_BILINEAR 2
#define ANYV2V_RESAMPLE_BICUBIC 3
#define ANYV2V_RESAMPLE_BOX 4
#define ANYV2V_RESAMPLE_MAX_SIDE 16384
int anyv2v_resample_table(int in_size, double in0, double in1, int out_size, int filter, int* bounds, int* coeffs);
int anyv2v_resample_h_u8(const void* src, void* dst, int32_t F, int32_t H, int32_t W, int32_t C, int32_t row0, int32_t rows, int32_t out_w,
                         const int32_t* bounds, const int32_t* coeffs, int32_t ksize, void* stream);
int anyv2v_resample_v_u8(const void* src, void* dst, int32_t F, int32_t H, int32_t W, int32_t C, int32_t out_h, const int32_t* bounds,
                         const int32_t* coeffs, int32_t ksize, void* stream);

/* The way back to the source clip's own size (restore.hip): per frame, in Pillow's words,
 *   out = S.copy();  out.paste(E.resize(dsize, filter, box), (dx0, dy0), mask = A.resize(dsize, BILINEAR, box))
 * with S the source frame [sh, sw, 3], E the edited frame at the working size, A its alpha (one band) and dsize = (dx1 - dx0, dy1 - dy0).
 * Pillow resizes horizontally first: the caller runs anyv2v_resample_h_u8 on E (3 bands) and on A (1 band) over the input rows the vertical
 * tables read, and this entry does the rest in one launch over the whole output frame.
 *   source   uint8 [F, sh, sw, 3]
 *   edit_h   uint8 [F, e_rows, dw, 3], the horizontal intermediate of the edit, dw = dx1 - dx0
 *   alpha_h  uint8 [mask_frames, a_rows, dw], the horizontal intermediate of alpha, mask_frames = 1 (every frame) or F; or NULL: m = 255
 *            everywhere, a plain paste, and mask_frames / a_* are not looked at
 *   e_bounds int32 [dh][2], e_coeffs int32 [dh][e_ksize], dh = dy1 - dy0: DEVICE copies of the vertical table of the edit's filter as
 *            anyv2v_resample_table writes it, its (ymin, n) re-based to the intermediate's first row; a_bounds / a_coeffs [dh][a_ksize]: the
 *            same for alpha (BILINEAR: another filter, hence another table and another row range).  Where Pillow skips the vertical pass the
 *            caller hands an identity table (ksize 1, (r, 1), coefficient 2^22): the kernel does not branch on it
 *   out      uint8 [F, sh, sw, 3]
 * A byte outside dest = [dx0, dx1) x [dy0, dy1) is the source's.  A byte inside, per band, with d the source's byte:
 *   e = clamp((2^21 + sum over y < n of edit_h[ymin + y] * k[y]) >> 22, 0, 255)        the vertical pass of anyv2v_resample_v_u8
 *   m = the same form over alpha_h at the byte's pixel (255 without alpha)
 *   t = d * (255 - m) + e * m + 128;   out = ((t >> 8) + t) >> 8                       Pillow's paste for 8-bit bands, all in uint32
 * m = 0 returns d and m = 255 returns e exactly.  A negative status (text: anyv2v_last_error()) for a null source / edit_h / out or table,
 * F outside 1 .. 65535, sides outside 1 .. ANYV2V_RESAMPLE_MAX_SIDE, a dest that is empty or not inside the frame, rows or ksize below 1,
 * mask_frames other than 1 or F, tables that are not 4-byte aligned, or an out that overlaps any input.  A table entry that points outside
 * its intermediate is cut to it (no read leaves a buffer).  No operand but the tables needs an alignment.  No atomics, a fixed grid: every
 * output byte is written once, by one thread. */
int anyv2v_restore_paste_u8(const void* source, const void* edit_h, const void* alpha_h, void* out, int32_t F, int32_t sh, int32_t sw,
                            int32_t dx0, int32_t dy0, int32_t dx1, int32_t dy1, int32_t e_rows, const int32_t* e_bounds,
                            const int32_t* e_coeffs, int32_t e_ksize, int32_t mask_frames, int32_t a_rows, const int32_t* a_bounds,
                            const int32_t* a_coeffs, int32_t a_ksize, void* stream);

/* Detail-preserving restore (restore_detail.hip): the way back above, with the fine detail of the source carried into the upscaled edit.
 * With S the source frame and P the prepared source -- the frame the model saw, at the working size like the edit E --, S - up(P) is the
 * detail that the trip down and up destroys; it is added to up(E) wherever a gate says that E stayed close to P.  All 8-bit integers.
 *
 * anyv2v_detail_gate_u8: edit, prepared uint8 [F, h, w, 3] -> gate_out uint8 [F, h, w]; lo, hi integers with 0 <= lo < hi <= 255, radius
 * 0 .. ANYV2V_DETAIL_MAX_RADIUS.  Per pixel:
 *   c[y, x] = max over the 3 bands of |E - P|
 *   b[y, x] = sum of c over the (2 radius + 1)^2 window, coordinates clamped to the frame (replicate edge)
 *   n = (2 radius + 1)^2;   mean = (b + n / 2) / n                                      (integer division)
 *   G = 255 where mean <= lo;   G = 0 where mean >= hi;   otherwise G = (255 * (hi - mean) + (hi - lo) / 2) / (hi - lo)
 * The box is separable: two launches, row sums into scratch (uint16 [F, h, w]: 255 * 33 < 65536; at least 2 F h w bytes, 2-byte aligned),
 * then column sums and the ramp.  Work is O(radius) per pixel.  No other operand needs an alignment; gate_out and scratch may overlap
 * nothing.  No read leaves a buffer.
 *
 * anyv2v_restore_detail_u8: anyv2v_restore_paste_u8's sibling.  The caller runs anyv2v_resample_h_u8 on E and P (3 bands, the edit's
 * filter) and on G and A (1 band, BILINEAR):
 *   prep_h   uint8 [F, e_rows, dw, 3], the horizontal intermediate of P: the same filter, the same box and the same row range as edit_h
 *   gate_h   uint8 [gate_frames, a_rows, dw], the horizontal intermediate of G, gate_frames = 1 (every frame) or F; never NULL, so the
 *            a_* tables (alpha's: BILINEAR) are always read
 *   alpha_h  uint8 [mask_frames, a_rows, dw] or NULL (m = 255), as above
 * A byte outside dest is the source's.  A byte inside, per band, with d the source's byte:
 *   e = the vertical pass over edit_h (as above);   p = the same table over prep_h
 *   g = the vertical pass of the a_* table over gate_h at the byte's pixel;   m = the same over alpha_h, or 255
 *   wt = g + (g >> 7)                                                                   0 .. 256, 255 maps to 256
 *   add = ((d - p) * wt + 128) >> 8                                                     arithmetic shift of a signed int32
 *   e2 = clamp(e + add, 0, 255)
 *   t = d * (255 - m) + e2 * m + 128;   out = ((t >> 8) + t) >> 8                       Pillow's paste, as above
 * g = 0 gives exactly anyv2v_restore_paste_u8 (and so Pillow); g = 255 with e = p gives d; m = 0 gives d.  Hence an edit that changes
 * nothing (E = P, whose gate is 255 everywhere, and a constant 255 resamples to 255) restores the source byte for byte.  Refused, like
 * above: null pointers, sizes out of range, an empty dest or one outside the frame, gate_frames / mask_frames other than 1 or F, tables that
 * are not 4-byte aligned, an out that overlaps any input.  A table entry that points outside its intermediate is cut to it.  No atomics, a
 * fixed grid: every output byte is written once, by one thread. */
#define ANYV2V_DETAIL_MAX_RADIUS 16
int anyv2v_detail_gate_u8(const void* edit, const void* prepared, void* gate_out, int32_t F, int32_t h, int32_t w, int32_t lo, int32_t hi,
                          int32_t radius, void* scratch, int64_t scratch_bytes, void* stream);
int anyv2v_restore_detail_u8(const void* source, const void* edit_h, const void* prep_h, const void* gate_h, const void* alpha_h, void* out,
                             int32_t F, int32_t sh, int32_t sw, int32_t dx0, int32_t dy0, int32_t dx1, int32_t dy1, int32_t e_rows,
                             const int32_t* e_bounds, const int32_t* e_coeffs, int32_t e_ksize, int32_t gate_frames, int32_t mask_frames,
                             int32_t a_rows, const int32_t* a_bounds, const int32_t* a_coeffs, int32_t a_ksize, void* stream);

/* Plain elementwise DDIM / inverse-DDIM step (eta = 0, v-prediction) on same-layout tensors:
 * the generic `scheduler.step(model_output, t, sample).prev_sample` (pipeline_i2vgen_xl.py:868,1173,1418). */
int anyv2v_ddim_step_f16(const void* V, const void* X, void* Y, float sa_t, float sb_t, float sa_p, float sb_p,
                         int64_t n, void* stream);

/* Guidance combine + DDIM / inverse-DDIM step (eta = 0) on same-layout tensors, any prediction type: the loop body of the
 * ConsistI2V pipeline (consisti2v/consisti2v/pipelines/pipeline_video_editing.py:921-937 invert, :1539-1555 sample_with_pnp, :676-692
 * __call__; scheduler arithmetic consisti2v/ddim_inverse_scheduler.py:329-369).  E: the UNet's prediction of every branch, `n`
 * contiguous elements per branch; branch indices b_unc / b_img / b_txt:
 *   e = e[b_unc] + g_img (e[b_img] - e[b_unc]) + g_txt (e[b_txt] - e[b_img])    "both";   b_img < 0: e[b_unc] + g_txt (e[b_txt] - e[b_unc]);
 *   b_unc < 0: e[b_txt] (no guidance).   prediction: 0 v_prediction, 1 epsilon, 2 sample.   X / Y: `n` elements; Y may alias X. */
int anyv2v_guided_step_f16(const void* E, int64_t n, int32_t b_unc, int32_t b_img, int32_t b_txt, float g_img, float g_txt,
                           int32_t prediction, float sa_t, float sb_t, float sa_p, float sb_p, const void* X, void* Y, void* stream);

/* The same with general coefficients and an additive noise term -- the ancestral (DDPM) step of SEINE's edit loop
 * (seine/run_pnp_edit.py:205 `self.scheduler.step(noise_pred, t, x)` with sample_method "ddpm"):
 *   y = c_x0 * x0 + c_eps * eps + sigma * noise[i]      x0 / eps from the guided prediction as above (sa_t, sb_t).
 * DDPM without sample clipping: c_x0 = coeff_x0 + coeff_xt * sa_t, c_eps = coeff_xt * sb_t (x = sa_t x0 + sb_t eps).  noise may be NULL
 * when sigma is 0 (the last step). */
int anyv2v_guided_step_noise_f16(const void* E, int64_t n, int32_t b_unc, int32_t b_img, int32_t b_txt, float g_img, float g_txt,
                                 int32_t prediction, float sa_t, float sb_t, float c_x0, float c_eps, const void* X, void* Y,
                                 const void* noise, float sigma, void* stream);

/* ---- misc ------------------------------------------------------------------------------------- */
/* Launch heuristics (kernel family, split-K factor, GroupNorm chunking) see rows * num / den from now on; grids and bounds keep the true
 * row counts.  The PnP edit runs some steps on [negative, editing] only (steps outside every injection schedule; steps whose source
 * features are replayed from a multi-edit cache, pipeline_i2vgen_xl.py:1136-1162): with the hint 3 / 2 those launches choose what the
 * three-branch launch chooses, so every fp32 summation order -- and the result, bit for bit -- is the same.  (1, 1) resets.
 * PROCESS-GLOBAL and NOT thread-safe: one host-side pair of integers read by every launch at enqueue (= graph capture) time, like the
 * single-threaded reference loop it serves.  A host that enqueues from several threads must serialise "set hint .. launches ..
 * reset" itself (anyv2v_last_error(), by contrast, is thread-local). */
int anyv2v_set_batch_hint(int32_t num, int32_t den);
const char* anyv2v_last_error(void);
/* ABI version = major * 100 + minor.  Descriptors carry no size field: a caller MUST be compiled against the header of the
 * library it loads (check anyv2v_version() >= the ANYV2V_ABI_VERSION it was built with) and MUST zero-initialise every
 * descriptor (new fields are appended with 0 = "off").  101: AnyV2VGemmDesc grew ln_c1 / ln_eps / reserved0 (round 3), flags
 * bits 13-16 select the persistent kernel's tile order (round 4).  102: anyv2v_ff_geglu_f16.  103: anyv2v_guided_step_f16, anyv2v_guided_step_noise_f16.
 * 104: GroupNorm sums about a pivot; pivoted sharded entry points anyv2v_groupnorm_pivot_f16 / _partial_pivot_f16 /
 * _apply_pivot_f16 (the earlier pair is unchanged).  105: AnyV2VGemmDesc grew gn_stats / gn_stats_floats / gn_rows_per_group /
 * gn_groups (GroupNorm statistics from the GEMM epilogue), anyv2v_gemm_gn_stats_floats, anyv2v_gemm_gn_launches,
 * anyv2v_groupnorm_stats_floats, anyv2v_groupnorm_apply_stats_f16; nothing earlier changed (a 104 caller that zero-initialises its descriptors, as required,
 * must still be recompiled against this header because the structure grew).  anyv2v_freeu_f16, anyv2v_tile_blend_f16, anyv2v_latent_mask_f16,
 * anyv2v_masked_blend_f16, anyv2v_diff_map_accum_f16, anyv2v_diff_map_finish_f16, anyv2v_pixel_alpha_f16, anyv2v_composite_stats_u8,
 * anyv2v_composite_u8, anyv2v_luma_u8, anyv2v_block_match_u8, anyv2v_flow_median_i16, anyv2v_mask_propagate_u8,
 * anyv2v_first_frame_mask_u8, anyv2v_resample_table, anyv2v_resample_h_u8, anyv2v_resample_v_u8 and anyv2v_restore_paste_u8 were added under 105, and anyv2v_detail_gate_u8 and anyv2v_restore_detail_u8 after them: new entry
 * points, no structure changed
 * (a binding that needs them finds out when it resolves the symbol). */
#define ANYV2V_ABI_VERSION 105
int anyv2v_version(void);
/* MFMA / LDS layout self-test used by the gpu test-suite (returns 0 when the layouts the kernels assume hold) */
int anyv2v_selftest(void* scratch, int64_t scratch_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ANYV2V_HIP_H */
