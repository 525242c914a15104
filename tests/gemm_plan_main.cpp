// Stand-alone driver of the GEMM launch planner (anyv2v_amd/csrc/gemm_plan.cpp) for tests/test_gemm_plan_host.py: reads one
// descriptor per line from stdin as key=value words, prints one JSON object per plan.  No GPU, no HIP: the test builds this file and
// the planner with the host compiler (address + undefined-behaviour sanitizers) and runs it as its own process.
//
// Integer fields of AnyV2VGemmDesc go by their names; unset leading dimensions default to the dense ones (lda0 = C0, lda1 = C1,
// ldc = ldr = ldrv = N), rowvec_div to 1.  Operand pointers are fake, 16-byte aligned addresses: A0, W and C always, A1 when C1 > 0,
// and bias=1 / rowvec=1 / R=1 / ln=1 / gn=1 (gn_stats) switch the optional ones on.  ws_mib (default 128; ws_null=1: no buffer) is the
// workspace, hint the batch-hinted row count (default M).
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <sstream>
#include <string>

#include "../anyv2v_amd/csrc/gemm_plan.h"

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
        auto ptr = [&](const char* key, uintptr_t addr, bool dflt) { return get(key, dflt) ? (void*)addr : nullptr; };
        AnyV2VGemmDesc d;
        memset(&d, 0, sizeof(d));
        d.M = (int32_t)get("M", 0); d.N = (int32_t)get("N", 0); d.C0 = (int32_t)get("C0", 0); d.C1 = (int32_t)get("C1", 0);
        d.A0 = ptr("A0", 0x10000, true);
        d.A1 = ptr("A1", 0x20000, d.C1 > 0);
        d.W = ptr("W", 0x30000, true);
        d.C = ptr("C", 0x40000, true);
        d.bias = ptr("bias", 0x50000, false);
        d.rowvec = ptr("rowvec", 0x60000, false);
        d.R = ptr("R", 0x70000, false);
        d.ln_c1 = (const float*)ptr("ln", 0x80000, false);
        d.gn_stats = (float*)ptr("gn", 0x90000, false);
        d.workspace = ptr("ws", 0xa0000, !get("ws_null", 0));
        d.workspace_bytes = get("ws_mib", 128) << 20;
        d.lda0 = (int32_t)get("lda0", d.C0); d.lda1 = (int32_t)get("lda1", d.C1);
        d.ldc = (int32_t)get("ldc", d.N); d.ldr = (int32_t)get("ldr", d.N); d.ldrv = (int32_t)get("ldrv", d.N);
        d.rowvec_div = (int32_t)get("rowvec_div", 1);
        d.mode = (int32_t)get("mode", 0);
        d.Hi = (int32_t)get("Hi", 0); d.Wi = (int32_t)get("Wi", 0); d.Ho = (int32_t)get("Ho", 0); d.Wo = (int32_t)get("Wo", 0);
        d.stride = (int32_t)get("stride", 0); d.up = (int32_t)get("up", 0); d.asym = (int32_t)get("asym", 0);
        d.F = (int32_t)get("F", 0); d.HW = (int32_t)get("HW", 0);
        d.act = (int32_t)get("act", 0);
        d.flags = (int32_t)get("flags", 0);
        d.gn_groups = (int32_t)get("gn_groups", 0); d.gn_rows_per_group = (int32_t)get("gn_rpg", 0);
        d.gn_stats_floats = get("gn_floats", 0);
        g_message[0] = 0;
        const GemmPlan p = av_gemm_plan(d, (int)get("hint", d.M));
        printf("{\"status\": %d, \"message\": \"%s\", \"family\": \"%s\", \"nf\": %d, \"splits\": %d, \"tilesN\": %d, \"tiles\": %d, "
               "\"grid\": %d, \"raster\": [%d, %d, %d, %d, %d], \"pp_mf\": %d, \"sk_blocks\": %d, \"gn_records\": %s, \"gn_decline\": \"%s\"}\n",
               p.status, g_message, av_gemm_family_name(p.family), p.nf, p.splits, p.tilesN, p.tiles, p.grid, p.rast_gm, p.rast_gn,
               p.rast_sm, p.rast_sn, p.rast_nfast, p.pp_mf, p.sk_blocks, p.gn_records ? "true" : "false",
               p.gn_decline != nullptr ? p.gn_decline : "");
    }
    return 0;
}
