// Small device helpers that the pixel kernels (video, vis, overlay, fit, temporal, objects, boundary) share: each is defined here once.
#pragma once
#include "cgs_common.h"

// a.b over the three colour bytes of two packed colours r | g << 8 | b << 16 (the fourth byte is 0)
__device__ __forceinline__ uint32_t px_dot3(uint32_t a, uint32_t b) {
#if __has_builtin(__builtin_amdgcn_udot4)
    return __builtin_amdgcn_udot4(a, b, 0u, false);
#else
    return (a & 255u) * (b & 255u) + ((a >> 8) & 255u) * ((b >> 8) & 255u) + ((a >> 16) & 255u) * ((b >> 16) & 255u);
#endif
}

// cell `cell` of a stack of RGB bytes as r | g << 8 | b << 16
__device__ __forceinline__ uint32_t px_colour(const uint8_t* __restrict__ low, int64_t cell) {
    return (uint32_t)low[3 * cell] | ((uint32_t)low[3 * cell + 1] << 8) | ((uint32_t)low[3 * cell + 2] << 16);
}

// the maximum of v over the wave, in every lane
__device__ __forceinline__ int px_wave_max(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = max(v, __shfl_xor(v, m, CGS_WAVE));
    return v;
}

// a store that, with NT, does not stay in the caches: for output that the GPU does not read again
template <bool NT, typename T>
__device__ __forceinline__ void px_put(T* p, const T& v) {
    if (NT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}
