// Stand-alone driver of the attention launch planner (anyv2v_amd/csrc/attention_plan.cpp) for tests/test_attention_plan_host.py: reads one
// launch per line from stdin as key=value words, prints one JSON object per plan.  No GPU, no HIP: the test builds this file and the
// planner with the host compiler (address + undefined-behaviour sanitizers) and runs it as its own process.
//
// entry = 0 | 1 | 2 (anyv2v_attention_f16 / _small_f16 / _bias_f16), head_dim (default 64), bias = 1: a bias pointer.  Integer fields of
// AnyV2VAttnDesc go by their names; unset: batch = heads = 1, inner = kv_div = 1, qk_mod = 0, q_outer = Sq, kv_outer = Sk, q_seq = kv_seq = 1,
// the inner strides 0, ldq = ldk = ldv = ldo = heads * head_dim, flags = 0.  scale_milli = 1000 x scale (default 125).  Q / K / V / O = the
// operand's address modulo 16 (fake addresses, never dereferenced), -1: a null pointer.  null_desc = 1 plans a null descriptor.
// The line "instantiations" prints the table of av_attn_instantiation().
#include <stdarg.h>
#include <stdio.h>
#include <string.h>

#include <map>
#include <sstream>
#include <string>

#include "../anyv2v_amd/csrc/attention_plan.h"

static char g_message[512];   // what the library's anyv2v_set_error (errors.hip) would keep for anyv2v_last_error()
void anyv2v_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_message, sizeof(g_message), fmt, ap);
    va_end(ap);
}

static const char* const KERNELS[] = {"naive", "short", "flash", "small", "loop"};
static_assert(sizeof(KERNELS) / sizeof(KERNELS[0]) == ATTN_KERNEL_COUNT, "one name per kernel");

int main() {
    char line[1024];
    while (fgets(line, sizeof(line), stdin)) {
        if (strncmp(line, "instantiations", 14) == 0) {
            printf("{\"instantiations\": [");
            for (int i = 0; i < av_attn_instantiation_count(); ++i) printf("%s\"%s\"", i ? ", " : "", av_attn_kernel_name(av_attn_instantiation(i)));
            printf("]}\n");
            continue;
        }
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
        auto ptr = [&](const char* key, uintptr_t addr) { const long long r = get(key, 0); return r < 0 ? (void*)nullptr : (void*)(addr + (uintptr_t)r); };
        const int head_dim = (int)get("head_dim", 64);
        AnyV2VAttnDesc d;
        memset(&d, 0, sizeof(d));
        d.Q = ptr("Q", 0x10000); d.K = ptr("K", 0x20000); d.V = ptr("V", 0x30000); d.O = ptr("O", 0x40000);
        d.batch = (int32_t)get("batch", 1); d.heads = (int32_t)get("heads", 1); d.Sq = (int32_t)get("Sq", 0); d.Sk = (int32_t)get("Sk", 0);
        const long long C = (long long)d.heads * head_dim;
        d.ldq = (int32_t)get("ldq", C); d.ldk = (int32_t)get("ldk", C); d.ldv = (int32_t)get("ldv", C); d.ldo = (int32_t)get("ldo", C);
        d.inner = (int32_t)get("inner", 1);
        d.q_outer = get("q_outer", d.Sq); d.q_inner = get("q_inner", 0); d.q_seq = get("q_seq", 1);
        d.kv_outer = get("kv_outer", d.Sk); d.kv_inner = get("kv_inner", 0); d.kv_seq = get("kv_seq", 1);
        d.kv_div = (int32_t)get("kv_div", 1); d.qk_mod = (int32_t)get("qk_mod", 0);
        d.scale = (float)get("scale_milli", 125) / 1000.0f;
        d.flags = (int32_t)get("flags", 0);
        g_message[0] = 0;
        const AttnPlan p = av_attn_plan(get("null_desc", 0) ? nullptr : &d, (AttnEntry)get("entry", 0), head_dim, get("bias", 0) != 0);
        printf("{\"status\": %d, \"message\": \"%s\", \"kernel\": \"%s\", \"name\": \"%s\", \"stages\": %d, \"streams\": %d, \"waves\": %d, \"ds\": %d, "
               "\"nkb\": %d, \"bias\": %s, \"causal\": %d, \"q_tiles\": %d, \"grid\": [%u, %u, %u], \"block\": %d, \"lds\": %zu, \"wide\": \"%s\"}\n",
               p.status, g_message, KERNELS[p.kernel], p.status == ANYV2V_OK ? av_attn_kernel_name(p) : "", p.stages, p.streams, p.waves, p.ds,
               p.nkb, p.bias ? "true" : "false", p.causal, p.q_tiles, p.grid_x, p.grid_y, p.grid_z, p.block, p.lds_bytes,
               p.wide_reason != nullptr ? p.wide_reason : "");
    }
    return 0;
}
