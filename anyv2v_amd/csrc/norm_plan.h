// Launch plan of the GroupNorm entry points (norm.hip): block size, chunking of the statistics pass, row partition of the apply pass,
// folding of GEMM-written records, and the sizes of the three float buffers the ABI speaks of.  Pure functions of the shape, the hinted
// row count and the occupancy (no HIP, no globals): plain C++17, built for the host alone by tests/test_norm_plan_host.py.
// norm.hip checks its pointers for null, plans, then launches what the plan says.
#pragma once
#include <stddef.h>

#include "../../include/anyv2v_hip.h"   // (and stdint.h)

#define AV_PLAN_LOCAL __attribute__((visibility("hidden")))   // shared between the library's objects, never exported

#define GN_MAX_CHUNKS 256   // partial sums (or records) an apply block folds per (statistics group, channel group), at most

void anyv2v_set_error(const char* fmt, ...);   // errors.hip (the planner test brings its own): the text behind a failed status

struct GnPlan {
    int status;   // ANYV2V_OK / ANYV2V_EINVAL (text: anyv2v_last_error())
    int nsg;      // statistics groups: M / rows_per_group
    int V;        // 16-byte vectors per row: C / 8
    // These three fix the order of the floating-point additions and so the bits of the result.  They depend on the shape and on
    // hinted_rows alone, never on apply_slots.
    int rpb;          // rows a block walks side by side; a thread adds rows rl, rl + rpb, ... of its chunk
    int nchunks;      // partial sums per (statistics group, channel group): grid.y of the statistics pass
    int rows_chunk;   // rows per chunk (the last one may be shorter)
    // These only partition work: any value gives the same result.
    long long bps;    // apply blocks per statistics group: grid.x of the apply pass
    int rows_block;   // rows per apply block (the last one may be shorter)
    int threads;      // block size of both passes: av_gn_threads(C, G)
    size_t lds;       // dynamic LDS of the statistics pass: [rpb][C][2] floats
};

// V x rpb threads with rpb = 256 / V (at least one row), not below one wave nor below G (thread g < G folds channel group g);
// 0 for a C that has no block (C < 8).  norm.hip asks the occupancy of this block size before it plans.
AV_PLAN_LOCAL int av_gn_threads(int C, int G);

// hinted_rows: av_hint_rows(M), the row count the chunking should see (anyv2v_set_batch_hint); apply_slots: resident apply blocks of
// `threads` threads on the whole device; aligned: the sources are 16-byte aligned (checked where norm.hip used to check it, between
// the shape checks).
AV_PLAN_LOCAL GnPlan av_gn_plan(int32_t C0, int32_t C1, int32_t M, int32_t rows_per_group, int32_t G, int hinted_rows, int apply_slots,
                                bool aligned = true);

// GroupNorm from the records of a producing GEMM (anyv2v_groupnorm_apply_stats_f16): one record per (16 rows, channel group).  More
// than GN_MAX_CHUNKS of them per statistics group are first folded in runs of `run` consecutive records.
struct GnRecordsPlan {
    int status;
    int nrec;           // records per (statistics group, channel group) as the GEMM wrote them: rows_per_group / 16
    bool fold;          // nrec > GN_MAX_CHUNKS: a fold launch of (nruns, nsg) blocks comes first
    int run, nruns;     // records per run (the last run may be shorter), runs; 1, nrec without a fold
    float n_gemm;       // values behind one record as the GEMM wrote it: 16 rows of a channel group
    float n_rec;        // values behind each record the apply kernel reads, except the last:
    float n_last;       // values behind that one
    int64_t folded_at;  // float offset in `stats` of the folded records (behind the GEMM's)
};
AV_PLAN_LOCAL GnRecordsPlan av_gn_records_plan(int32_t M, int32_t C, int32_t rows_per_group, int32_t G);

// anyv2v_groupnorm_scratch_floats / _stats_floats / _partial_floats
AV_PLAN_LOCAL int64_t av_gn_scratch_floats(int32_t M, int32_t rows_per_group, int32_t G);   // [nsg][1 + GN_MAX_CHUNKS][G][2]: any plan's partial sums, and the pivots
AV_PLAN_LOCAL int64_t av_gn_stats_floats(int32_t M, int32_t rows_per_group, int32_t G);     // the GEMM's records, and GN_MAX_CHUNKS folded ones per group; 0: no such buffer
AV_PLAN_LOCAL int64_t av_gn_partial_floats(const GnPlan& pl, int32_t G);                    // [nsg][nchunks][G][2], what a sharded caller all-reduces; -1: no plan
