// What cgs_temporal_smooth (csrc/temporal.hip) and cgs_temporal_smooth_mc (csrc/temporal_motion.hip) have in common: the tap of the filter and
// the host side's argument check and coefficients.  The two kernels differ in where a tap's cell lies, not in what a tap does.
#pragma once
#include "pixel_common.h"

// One tap: the cell of colour l and mask value zl of frame f + k against the centre cell of colour c0 (cc = c0.c0), kk = (float)(k k) and
// e the spatial term of the exponent (+inf for a cell outside the grid: the weight is then +0 exactly).
//   w = exp2(-(d2 cr + (kk ct + e))),  num = fma(w, zl, num),  den = den + w
// with both sums of the exponent fused multiply-adds, written out: what the compiler may contract does not decide the rounding.  Both
// kernels form every tap here and nowhere else, so on an all-zero motion field, where their taps are the same cells in the same order,
// cgs_temporal_smooth_mc gives cgs_temporal_smooth's output bit for bit (tests/test_gpu_temporal_motion.py asserts it).
__device__ __forceinline__ void ts_tap(uint32_t cc, uint32_t c0, uint32_t l, float zl, float cr, float kk, float ct, float e, float& num,
                                       float& den) {
    const uint32_t d2 = cc + px_dot3(l, l) - 2u * px_dot3(c0, l);
    const float arg = fmaf((float)d2, cr, fmaf(kk, ct, e));
    const float w = __builtin_amdgcn_exp2f(-arg);
    num = fmaf(w, zl, num);
    den += w;
}

struct TsCoef {
    float cr, ct, cs;                                         // log2(e) / (2 sigma_r^2), log2(e) / (2 sigma_t^2) with sigma_t = radius / 2, log2(e) / 2
};

// The arguments that both entries take, and the coefficients.  `more_bad`: an argument error of the caller's own; like every argument error
// it comes before CGS_ERR_UNSUPPORTED.
inline int ts_prepare(const float* z, const uint8_t* low, const float* out, int32_t n, int32_t f0, int32_t f1, int32_t radius, float sigma_r,
                      bool more_bad, TsCoef* c) {
    if (!z || !low || !out || n < 1 || f0 < 0 || f1 <= f0 || f1 > n || radius < 1 || !(sigma_r > 0.0f) || sigma_r > 3.0e38f ||
        ((uintptr_t)z & 3u) || ((uintptr_t)out & 3u) || more_bad)
        return CGS_ERR_BADARG;
    if (radius > CGS_TEMPORAL_MAX_RADIUS) return CGS_ERR_UNSUPPORTED;
    const double log2e = 1.4426950408889634, sigma_t = 0.5 * (double)radius;
    c->cr = (float)(log2e / (2.0 * (double)sigma_r * (double)sigma_r));
    c->ct = (float)(log2e / (2.0 * sigma_t * sigma_t));
    c->cs = (float)(log2e / 2.0);
    return CGS_OK;
}
