// pd_keys.h -- the perturbed simplex keys of an edge, perturb_filter_function (accelerated_PD.py:16-22), for pd_pipeline.hip,
// pd_tiny.hip and pd_wide.hip.  This one expression decides bit parity with the reference: it is evaluated in exactly this
// association with two roundings each, never a fused multiply-add, so the including unit must be built with -ffp-contract=off
// (the Makefile's default; the three users are).
#pragma once
#include "tlc_common.h"

__device__ __forceinline__ double tlc_key_asc(double fa, double fb) {
    const double hi = fa > fb ? fa : fb, lo = fa < fb ? fa : fb;
    return hi + (lo + 1.0) * 1e-6;
}
__device__ __forceinline__ double tlc_key_desc(double fa, double fb) {
    const double hi = fa > fb ? fa : fb, lo = fa < fb ? fa : fb;
    return lo - (101.0 - hi) * 1e-6;
}
