// Stand-alone driver of the fused temporal attention kernel's plan (anyv2v_amd/csrc/tattn_plan.cpp) for tests/test_tattn_fused_host.py:
// one case per input line "rows_per_branch B C heads F HW", one JSON line out.  `covered`: walking every block's range as the
// kernel does (av_tattn_block, then waves striding by TATTN_WAVES), each (head, strip) is visited exactly once.
#include <cstdio>
#include <vector>

#include "../anyv2v_amd/csrc/tattn_plan.h"

int main() {
    long long rows;
    int B, C, heads, F, HW;
    while (std::scanf("%lld %d %d %d %d %d", &rows, &B, &C, &heads, &F, &HW) == 6) {
        const TattnPlan p = av_tattn_plan(rows, B, C, heads, F, HW);
        int covered = 0;
        if (p.supported) {
            std::vector<int> seen((size_t)heads * p.nstrips, 0);
            bool ok = true;
            for (int blk = 0; blk < p.grid; ++blk) {
                int head, begin, end;
                av_tattn_block(p, blk, heads, &head, &begin, &end);
                ok = ok && head >= 0 && head < heads && begin >= 0 && begin <= end && end <= p.nstrips;
                if (!ok) break;
                for (int w = 0; w < TATTN_WAVES; ++w)
                    for (int s = begin + w; s < end; s += TATTN_WAVES) ++seen[(size_t)head * p.nstrips + s];
            }
            for (int v : seen) ok = ok && v == 1;
            covered = ok ? 1 : 0;
        }
        std::printf("{\"supported\": %d, \"pays\": %d, \"nstrips\": %d, \"px\": %d, \"spr\": %d, \"grid\": %d, \"lds_bytes\": %d, \"covered\": %d}\n",
                    p.supported, p.pays, p.nstrips, p.px, p.spr, p.grid, p.lds_bytes, covered);
    }
    return 0;
}
