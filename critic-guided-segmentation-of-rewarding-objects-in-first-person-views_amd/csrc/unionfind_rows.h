// The run-based union-find over the bit rows of one frame of at most 64 x 64 pixels in LDS, shared by csrc/objects.hip (labelling) and
// csrc/clean.hip (hysteresis, hole filling).  A lane is a column, a row is one 64-bit mask whose bits at and beyond w are clear, and the
// LDS index of a pixel is its raster index y w + x.  L[p] is p's parent: it starts as the first pixel of p's horizontal run and only
// ever decreases, so every loop below ends, whatever the other lanes do meanwhile, and after a barrier the forest is exact: there is
// no sweep count that a winding region could exceed.
#pragma once
#include "cgs_common.h"

__device__ __forceinline__ int lds_get(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
__device__ __forceinline__ void lds_put(int* p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ __forceinline__ int find_root(int* L, int a) {
    int p;
    while ((p = lds_get(&L[a])) != a) a = p;
    return a;
}

// the root of a; a itself is pointed at it on the way out (it is no root, so this cannot undo a union; parents only decrease)
__device__ __forceinline__ int find_compress(int* L, int a) {
    const int r = find_root(L, a);
    if (r != a) atomicMin(&L[a], r);
    return r;
}

__device__ __forceinline__ void unite(int* L, int a, int b) {
    for (;;) {
        const int ra = find_compress(L, a), rb = find_compress(L, b);
        if (ra == rb) return;
        const int hi = max(ra, rb), lo = min(ra, rb);
        const int old = atomicMin(&L[hi], lo);
        if (old == hi) return;                         // hi was still a root: it hangs below lo now
        a = old;                                       // hi had got a parent meanwhile; hi points at min(old, lo), and what is left to
        b = lo;                                        // join is the tree of that parent with lo's
    }
}

// start column of the run of on-pixels that holds column `lane` of the row with on-mask m (lane is on); lt = bits below lane
__device__ __forceinline__ int run_start(unsigned long long m, unsigned long long lt) {
    const unsigned long long zeros = ~m & lt;
    return zeros ? 64 - __clzll((long long)zeros) : 0;
}

// One pixel's part of the merge with the row above: (y, x) is on in `cur`, `up` is the row above; a pair of touching runs is united
// once, by the leftmost pixel of the contact.
__device__ __forceinline__ void unite_with_row_above(int* L, unsigned long long cur, unsigned long long up, int y, int x, int w, bool conn8) {
    const bool U = (up >> x) & 1ull;
    const bool UL = x > 0 && ((up >> (x - 1)) & 1ull), UR = x < 63 && ((up >> (x + 1)) & 1ull);
    const bool Lf = x > 0 && ((cur >> (x - 1)) & 1ull), Rt = x < 63 && ((cur >> (x + 1)) & 1ull);
    const int p = y * w + x;
    if (U) {
        if (!(Lf && UL)) unite(L, p, p - w);                               // else the pixel to the left joined the same two runs
    } else if (conn8) {
        if (UL && !Lf) unite(L, p, p - w - 1);                             // Lf: the left pixel has this run straight above it
        if (UR && !Rt) unite(L, p, p - w + 1);                             // Rt: so has the right pixel
    }
}
