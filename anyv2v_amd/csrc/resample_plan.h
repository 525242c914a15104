// The coefficient tables of the 8-bit resampling passes (resample.hip): Pillow's precompute_coeffs + normalize_coeffs_8bpc, restated in
// include/anyv2v_hip.h.  A pure function of its arguments in IEEE double (no HIP, no globals): plain C++17, built for the host alone by
// tests/test_resample_host.py.  The file is compiled with floating-point contraction off: a fused multiply-add in the weight arithmetic
// can move a coefficient by one.
#pragma once
#include "../../include/anyv2v_hip.h"   // anyv2v_resample_table, ANYV2V_RESAMPLE_* (and stdint.h)

#define RS_PRECISION_BITS 22   // 32 - 8 - 2: an 8-bit sample times a coefficient, and a factor 2 of room for the negative lobes

void anyv2v_set_error(const char* fmt, ...);   // errors.hip (the planner test brings its own): the text behind a failed status
