// Stand-alone driver of the resampling-table planner (anyv2v_amd/csrc/resample_plan.cpp) for tests/test_resample_host.py: reads one side
// per line from stdin as "in_size in0 in1 out_size filter fill" (fill = 0: the query with null pointers), prints one JSON object per line:
// the status or ksize, the error text, and for fill = 1 the two tables flattened.  No GPU, no HIP: the test builds this file and the planner
// with the host compiler (address + undefined-behaviour sanitizers, no floating-point contraction) and runs it as its own process.  The
// tables are allocated at exactly out_size * 2 and out_size * ksize ints, so a write past either end is the sanitizer's to report.
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../anyv2v_amd/csrc/resample_plan.h"

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
        int in_size = 0, out_size = 0, filter = 0, fill = 0;
        char a[128], b[128];
        if (sscanf(line, "%d %127s %127s %d %d %d", &in_size, a, b, &out_size, &filter, &fill) != 6) {
            fprintf(stderr, "bad line '%s'\n", line);
            return 2;
        }
        const double in0 = strtod(a, nullptr), in1 = strtod(b, nullptr);
        g_message[0] = 0;
        const int ksize = anyv2v_resample_table(in_size, in0, in1, out_size, filter, nullptr, nullptr);
        if (!fill || ksize <= 0) {
            printf("{\"ksize\": %d, \"message\": \"%s\"}\n", ksize, g_message);
            continue;
        }
        std::vector<int> bounds((size_t)out_size * 2, -7), coeffs((size_t)out_size * ksize, -7);
        g_message[0] = 0;
        const int rc = anyv2v_resample_table(in_size, in0, in1, out_size, filter, bounds.data(), coeffs.data());
        printf("{\"ksize\": %d, \"message\": \"%s\", \"bounds\": [", rc, g_message);
        for (size_t i = 0; i < bounds.size(); ++i) printf("%s%d", i ? ", " : "", bounds[i]);
        printf("], \"coeffs\": [");
        for (size_t i = 0; i < coeffs.size(); ++i) printf("%s%d", i ? ", " : "", coeffs[i]);
        printf("]}\n");
    }
    return 0;
}
