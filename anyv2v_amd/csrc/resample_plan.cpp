// Coefficient tables of the 8-bit resampling passes (resample_plan.h).  Host code only.
#include "resample_plan.h"

#include <math.h>

#include <vector>

#define TABLE_CHECK(cond, ...) do { if (!(cond)) { anyv2v_set_error(__VA_ARGS__); return ANYV2V_EINVAL; } } while (0)

static double box_filter(double x) { return x > -0.5 && x <= 0.5 ? 1.0 : 0.0; }

static double bilinear_filter(double x) {
    if (x < 0.0) x = -x;
    return x < 1.0 ? 1.0 - x : 0.0;
}

static double bicubic_filter(double x) {
    const double a = -0.5;
    if (x < 0.0) x = -x;
    if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
    if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
    return 0.0;
}

static double sinc_filter(double x) {
    if (x == 0.0) return 1.0;
    x = x * M_PI;
    return sin(x) / x;
}

static double lanczos_filter(double x) { return -3.0 <= x && x < 3.0 ? sinc_filter(x) * sinc_filter(x / 3) : 0.0; }

extern "C" int anyv2v_resample_table(int in_size, double in0, double in1, int out_size, int filter, int* bounds, int* coeffs) {
    TABLE_CHECK(in_size >= 1 && in_size <= ANYV2V_RESAMPLE_MAX_SIDE, "resample_table: in_size = %d must lie in [1, %d]", in_size,
                ANYV2V_RESAMPLE_MAX_SIDE);
    TABLE_CHECK(out_size >= 1 && out_size <= ANYV2V_RESAMPLE_MAX_SIDE, "resample_table: out_size = %d must lie in [1, %d]", out_size,
                ANYV2V_RESAMPLE_MAX_SIDE);
    // (written so that a NaN fails).  One float ulp of slack at the far end: Pillow checks a box given as C floats, then forms the width
    // in1 - in0 in float, so that in0 + width -- what a caller who restates that hands over -- can pass in_size by a rounding; the taps are
    // cut to the side below whatever the box says
    TABLE_CHECK(in0 >= 0.0 && in1 <= (double)in_size * (1.0 + 1.0 / (1 << 23)) && in0 < in1, "resample_table: box [%g, %g) must be non-empty and inside [0, %d]", in0, in1,
                in_size);
    double (*f)(double) = nullptr;
    double filter_support = 0.0;
    switch (filter) {
        case ANYV2V_RESAMPLE_BOX: f = box_filter; filter_support = 0.5; break;
        case ANYV2V_RESAMPLE_BILINEAR: f = bilinear_filter; filter_support = 1.0; break;
        case ANYV2V_RESAMPLE_BICUBIC: f = bicubic_filter; filter_support = 2.0; break;
        case ANYV2V_RESAMPLE_LANCZOS: f = lanczos_filter; filter_support = 3.0; break;
        default: TABLE_CHECK(false, "resample_table: unknown filter %d", filter);
    }
    const double scale = (in1 - in0) / out_size;
    const double fs = scale < 1.0 ? 1.0 : scale;
    const double sup = filter_support * fs;
    const double ss = 1.0 / fs;
    const int ksize = (int)ceil(sup) * 2 + 1;
    if (!bounds || !coeffs) return ksize;
    std::vector<double> w((size_t)ksize);
    for (int xx = 0; xx < out_size; ++xx) {
        const double center = in0 + (xx + 0.5) * scale;
        int xmin = (int)(center - sup + 0.5);
        if (xmin < 0) xmin = 0;
        int xmax = (int)(center + sup + 0.5);
        if (xmax > in_size) xmax = in_size;
        const int n = xmax - xmin;
        TABLE_CHECK(n >= 0 && n <= ksize, "resample_table: output %d has %d taps, the table has room for %d", xx, n, ksize);
        double ww = 0.0;
        for (int x = 0; x < n; ++x) {
            w[x] = f((x + xmin - center + 0.5) * ss);
            ww += w[x];
        }
        int* k = coeffs + (size_t)xx * ksize;
        long long sum_abs = 0;
        for (int x = 0; x < n; ++x) {
            if (ww != 0.0) w[x] /= ww;
            // (weights that nearly cancel: refused here, before the conversion could leave an int)
            TABLE_CHECK(w[x] > -2.0 && w[x] < 2.0, "resample_table: weight %g of output %d does not leave the int32 accumulator room", w[x], xx);
            k[x] = w[x] < 0 ? (int)(-0.5 + w[x] * (1 << RS_PRECISION_BITS)) : (int)(0.5 + w[x] * (1 << RS_PRECISION_BITS));
            sum_abs += k[x] < 0 ? -(long long)k[x] : k[x];
        }
        for (int x = n; x < ksize; ++x) k[x] = 0;
        TABLE_CHECK(sum_abs < (2ll << RS_PRECISION_BITS), "resample_table: sum |k| = %lld of output %d does not leave the int32 accumulator room",
                    sum_abs, xx);
        bounds[2 * xx] = xmin;
        bounds[2 * xx + 1] = n;
    }
    return ksize;
}
