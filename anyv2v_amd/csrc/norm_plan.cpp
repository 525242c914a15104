// Launch planning of the GroupNorm entry points (norm_plan.h).  Host code only.
#include "norm_plan.h"

#define PLAN_CHECK(cond, ...) do { if (!(cond)) { anyv2v_set_error(__VA_ARGS__); p.status = ANYV2V_EINVAL; return p; } } while (0)

static long long ceil_div(long long a, long long b) { return (a + b - 1) / b; }

int av_gn_threads(int C, int G) {
    const int V = C / 8;
    if (V < 1) return 0;
    const int rpb = 256 / V < 1 ? 1 : 256 / V;
    int threads = V * rpb;
    if (threads < 64) threads = 64;
    if (threads < G) threads = G;
    return threads;
}

GnPlan av_gn_plan(int32_t C0, int32_t C1, int32_t M, int32_t rows_per_group, int32_t G, int hinted_rows, int apply_slots, bool aligned) {
    GnPlan p = {};
    PLAN_CHECK(C0 > 0 && C1 >= 0, "groupnorm: bad C0/C1");
    const int C = C0 + C1;
    PLAN_CHECK(C0 % 8 == 0 && C1 % 8 == 0, "groupnorm: C0/C1 must be multiples of 8 (%d,%d)", C0, C1);
    PLAN_CHECK(G > 0 && G <= 64 && C % G == 0, "groupnorm: bad group count %d for C=%d", G, C);
    PLAN_CHECK(rows_per_group > 0 && M % rows_per_group == 0, "groupnorm: M %% rows_per_group != 0");
    PLAN_CHECK(aligned, "groupnorm: pointers must be 16-byte aligned");
    p.nsg = M / rows_per_group;
    p.V = C / 8;
    PLAN_CHECK(p.V <= 1024, "groupnorm: C too large (%d)", C);
    p.rpb = 256 / p.V < 1 ? 1 : 256 / p.V;
    p.threads = av_gn_threads(C, G);
    // Chunking, decided on the hinted number of statistics groups (anyv2v_set_batch_hint: a two-branch step sums its chunks in the
    // order the three-branch step does): about 1536 blocks in all, each thread at least 8 row iterations, at most GN_MAX_CHUNKS.
    const long long nsg_h = hinted_rows / rows_per_group > 0 ? hinted_rows / rows_per_group : 1;
    const long long min_rows = ceil_div(rows_per_group, p.rpb * 8);   // chunks, or apply blocks, of >= 8 row iterations per thread
    long long nchunks = ceil_div(1536, nsg_h);
    if (nchunks > min_rows) nchunks = min_rows;
    if (nchunks > GN_MAX_CHUNKS) nchunks = GN_MAX_CHUNKS;
    p.rows_chunk = (int)ceil_div(rows_per_group, nchunks);
    p.nchunks = (int)ceil_div(rows_per_group, p.rows_chunk);
    p.lds = (size_t)p.rpb * C * 2 * sizeof(float);
    PLAN_CHECK(p.lds <= 64 * 1024, "groupnorm: LDS reduction buffer too large");
    // Apply blocks: as many as the chip holds at once (CUs x resident blocks of this size), not more -- 2064 blocks on 1792 slots
    // ran a second, 15 %-full round (the 64x64-level launches, profiles/r03_bench_kernel_summary.md); each block at least 8
    // row iterations per thread where the statistics group is large enough.
    const long long vec_sg = (long long)rows_per_group * p.V;
    PLAN_CHECK(vec_sg < (1ll << 31), "groupnorm: stat group too large (%lld vectors)", vec_sg);
    p.bps = p.nsg != 0 ? apply_slots / p.nsg : 1;   // (M = 0: an empty grid, which the launch reports)
    if (p.bps > min_rows) p.bps = min_rows;
    if (p.bps < 1) p.bps = 1;
    p.rows_block = (int)ceil_div(rows_per_group, p.bps);
    p.bps = ceil_div(rows_per_group, p.rows_block);
    return p;
}

GnRecordsPlan av_gn_records_plan(int32_t M, int32_t C, int32_t rows_per_group, int32_t G) {
    GnRecordsPlan p = {};
    PLAN_CHECK(G > 0 && C % G == 0, "groupnorm: bad group count %d for C=%d", G, C);
    PLAN_CHECK(rows_per_group > 0 && rows_per_group % 16 == 0, "groupnorm_apply_stats: rows_per_group must be a multiple of 16 (%d)",
               rows_per_group);
    p.nrec = rows_per_group / 16;
    p.fold = p.nrec > GN_MAX_CHUNKS;
    p.run = (p.nrec + GN_MAX_CHUNKS - 1) / GN_MAX_CHUNKS;
    p.nruns = (p.nrec + p.run - 1) / p.run;
    p.n_gemm = 16.f * (float)(C / G);
    p.n_rec = p.n_gemm * (float)p.run;
    p.n_last = p.n_gemm * (float)(p.nrec - (p.nruns - 1) * p.run);
    p.folded_at = (int64_t)3 * (M / 16) * G;
    return p;
}

int64_t av_gn_scratch_floats(int32_t M, int32_t rows_per_group, int32_t G) {
    const int64_t nsg = rows_per_group > 0 ? M / rows_per_group : 0;
    return nsg * G * 2 * (int64_t)(1 + GN_MAX_CHUNKS);
}

int64_t av_gn_stats_floats(int32_t M, int32_t rows_per_group, int32_t G) {
    if (M <= 0 || rows_per_group <= 0 || G <= 0 || rows_per_group % 16 != 0 || M % rows_per_group != 0) return 0;
    return (int64_t)3 * (M / 16) * G + (int64_t)3 * (M / rows_per_group) * GN_MAX_CHUNKS * G;
}

int64_t av_gn_partial_floats(const GnPlan& pl, int32_t G) { return pl.status == ANYV2V_OK ? (int64_t)pl.nsg * pl.nchunks * G * 2 : -1; }
