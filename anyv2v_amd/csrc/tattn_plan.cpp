// Host-side plan of the fused temporal QKV + attention kernel: see tattn_plan.h.  No device code, no HIP headers.
#include "tattn_plan.h"

TattnPlan av_tattn_plan(int64_t rows_per_branch, int B, int C, int heads, int F, int HW) {
    TattnPlan p = {};
    p.lds_bytes = TATTN_LDS_BYTES;
    if (B <= 0 || HW <= 0 || F != TATTN_F || C != TATTN_C || heads != TATTN_HEADS || (HW & 1)) return p;
    if (rows_per_branch != (int64_t)F * HW) return p;
    const int64_t nstrips = (int64_t)B * HW / 2;
    if (nstrips * 32 > INT32_MAX) return p;   // row indices of the launch stay below 2^31 (byte offsets are formed in 64 bits)
    p.supported = 1;
    p.pays = rows_per_branch >= TATTN_MIN_ROWS;
    p.nstrips = (int)nstrips;
    p.px = 32 / heads;                        // 32 CUs per XCD: 6 ranges x 5 heads
    const int nranges = 8 * p.px;
    p.spr = (p.nstrips + nranges - 1) / nranges;
    p.grid = 8 * p.px * heads;
    return p;
}
