// Stand-alone driver of the GroupNorm launch planner (anyv2v_amd/csrc/norm_plan.cpp) for tests/test_norm_plan_host.py: reads one shape per
// line from stdin as key=value words, prints one JSON object per line.  No GPU, no HIP: the test builds this file and the planner with the
// host compiler (address + undefined-behaviour sanitizers) and runs it as its own process.
//
// C0, C1 (default 0), rows (rows_per_group), nsg (statistics groups, default 1), M (default nsg * rows), G (default 32), num / den (the
// batch hint, default 1 / 1: the planner sees M * num / den hinted rows, as av_hint_rows of errors.hip gives them), slots (resident apply
// blocks, default 1792), aligned (default 1).  Each object holds the launch plan, the three buffer sizes and, under "rec", the records plan
// of the same shape (C = C0, a single source).
#include <stdarg.h>
#include <stdio.h>

#include <map>
#include <sstream>
#include <string>

#include "../anyv2v_amd/csrc/norm_plan.h"

static char g_message[512];   // what the library's anyv2v_set_error (errors.hip) would keep for anyv2v_last_error()
void anyv2v_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_message, sizeof(g_message), fmt, ap);
    va_end(ap);
}

int main() {
    char line[1024];
    while (fgets(line, sizeof(line), stdin)) {
        std::map<std::string, long long> v;
        std::istringstream in(line);
        std::string word;
        while (in >> word) {
            const size_t eq = word.find('=');
            if (eq == std::string::npos) {
                fprintf(stderr, "bad word '%s'\n", word.c_str());
                return 2;
            }
            v[word.substr(0, eq)] = std::stoll(word.substr(eq + 1), nullptr, 0);
        }
        if (v.empty()) continue;
        auto get = [&](const char* key, long long dflt) { return v.count(key) ? v[key] : dflt; };
        const int32_t C0 = (int32_t)get("C0", 0), C1 = (int32_t)get("C1", 0), rows = (int32_t)get("rows", 0), G = (int32_t)get("G", 32);
        const int32_t M = (int32_t)get("M", get("nsg", 1) * rows);
        const int hinted = (int)((long long)M * get("num", 1) / get("den", 1));
        g_message[0] = 0;
        const GnPlan p = av_gn_plan(C0, C1, M, rows, G, hinted, (int)get("slots", 1792), get("aligned", 1) != 0);
        printf("{\"status\": %d, \"message\": \"%s\", \"nsg\": %d, \"V\": %d, \"rpb\": %d, \"threads\": %d, \"nchunks\": %d, \"rows_chunk\": %d, "
               "\"rows_block\": %d, \"bps\": %lld, \"lds\": %zu, \"gn_threads\": %d, \"partial_floats\": %lld, \"scratch_floats\": %lld, "
               "\"stats_floats\": %lld, ",
               p.status, g_message, p.nsg, p.V, p.rpb, p.threads, p.nchunks, p.rows_chunk, p.rows_block, p.bps, p.lds, av_gn_threads(C0 + C1, G),
               (long long)av_gn_partial_floats(p, G), (long long)av_gn_scratch_floats(M, rows, G), (long long)av_gn_stats_floats(M, rows, G));
        g_message[0] = 0;
        const GnRecordsPlan r = av_gn_records_plan(M, C0, rows, G);
        printf("\"rec\": {\"status\": %d, \"message\": \"%s\", \"nrec\": %d, \"fold\": %s, \"run\": %d, \"nruns\": %d, \"n_gemm\": %.1f, "
               "\"n_rec\": %.1f, \"n_last\": %.1f, \"folded_at\": %lld}}\n",
               r.status, g_message, r.nrec, r.fold ? "true" : "false", r.run, r.nruns, r.n_gemm, r.n_rec, r.n_last, (long long)r.folded_at);
    }
    return 0;
}
