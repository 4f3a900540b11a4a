// How well a mask's outline follows the truth's outline: per frame of at most 64 x 64 pixels the two inner 4-neighbour boundaries, the
// exact squared Euclidean distance from every pixel to each of them, and from those the boundary F counts, the boundary-IoU band counts
// and the two directed Hausdorff distances (cgs_boundary_score, include/cgs_hip.h).  One workgroup of four waves takes one frame,
// everything lives in LDS and is integer, there are no atomics at all, and no result depends on the order of anything below.
//
//   1. bit rows   a lane is a column and a wave takes the rows wave, wave + 4, ... (as objects.hip): one __ballot per row and side gives
//                 the row's on-mask, 64 bits, columns at and beyond w clear.  The rows sit between two zero rows (index r + 1).
//   2. boundary   b[r] = m[r] & ~(m[r-1] & m[r+1] & (m[r] << 1) & (m[r] >> 1)): on, and one of the four neighbours off.  The shifts move
//                 zeros in and the guard rows are zero, so everything outside the frame is off; rows from h on are zero.
//   3. vertical   wave -> (side, upper or lower 32 rows), lane -> column.  A lane collects its column of b as one 64-bit word; the
//                 nearest boundary pixel above row r is the highest set bit at or below r, the nearest below the lowest at or above r
//                 (clz / ctz).  g2[side][r][c] = the squared vertical distance, BD_NONE when the column holds no boundary pixel.
//   4. horizontal the plain 64-candidate scan, NOT a lower envelope: d2[r][c] = min over c' of (c - c')^2 + g2[r][c'], int32.  A lane
//                 keeps its 64 values (c - c')^2 in registers for all rows and both sides; the row of g2 is read 4 words at a time
//                 and every lane reads the same address (a broadcast, no bank conflict).  The wave that owns row r is the only reader
//                 and writer of that row, and its LDS operations complete in order, so d2 replaces g2 where it is.  dist2 goes out
//                 here, straight from the registers.
//                 BD_NONE = 2^20: the largest real value is 2 x 63^2 = 7938, BD_NONE + 63^2 is far from wrapping, and a pixel's d2
//                 is >= BD_NONE exactly when that side has no boundary pixel at all -- the kernel's only test for "empty".
//   5. counts     the last wave adds up the boundary pixels (popcount per row) and the two directed Hausdorff maxima (a lane's maximum
//                 over the rows, then a wave maximum); wave k mod 4 takes tolerance k: per row two __ballots (d2_pred <= q,
//                 d2_truth <= q) and-ed with the row's boundary and mask words give the four counts by popcount.  One lane writes them.
//
// Cost per frame: 2 x 4096 x 64 add-min pairs in step 4 (about 2 k VALU operations and 512 16-byte LDS reads per lane); step 3 is some
// 500 operations per lane, the rest is small.
// LDS: 2 x 16 KiB (g2 / d2 of both sides) + 2 x 66 + 2 x 64 rows of 8 bytes = 34 KiB, four workgroups (16 waves) per CU: LDS, not the
// 32-wave limit, bounds occupancy.
#include "pixel_common.h"

namespace {

constexpr int BD_THREADS = 256;
constexpr int BD_WAVES = BD_THREADS / CGS_WAVE;
constexpr int BD_SIDE = CGS_OBJ_MAX_SIDE;             // a row is one wave-wide ballot
constexpr int BD_NONE = 1 << 20;                      // "no boundary pixel in this column"; see step 4 above
static_assert(BD_SIDE == CGS_WAVE && BD_WAVES == 4, "one lane per column; step 3 splits (side, half) over four waves");
static_assert(BD_NONE > 2 * (BD_SIDE - 1) * (BD_SIDE - 1) && BD_NONE > CGS_BOUNDARY_MAX_TOL_PX * CGS_BOUNDARY_MAX_TOL_PX, "BD_NONE");

__global__ void __launch_bounds__(BD_THREADS)
boundary_kernel(const void* __restrict__ pred, int kind, float thresh, const uint8_t* __restrict__ truth, int h, int w,
                const int32_t* __restrict__ tol2, int T, int32_t* __restrict__ counts, int32_t* __restrict__ dist2) {
    __shared__ __attribute__((aligned(16))) int s_d[2][BD_SIDE][BD_SIDE];     // g2, then d2
    __shared__ unsigned long long s_m[2][BD_SIDE + 2];                         // on-masks, row r at r + 1
    __shared__ unsigned long long s_b[2][BD_SIDE];                             // boundary rows
    const int x = threadIdx.x & (CGS_WAVE - 1), wave = threadIdx.x / CGS_WAVE;
    const bool live = x < w;
    const int64_t frame = (int64_t)blockIdx.x * h * w;

    // 1. bit rows (every row up to 63 is written: zero from h on), and the two guard rows
    for (int y = wave; y < BD_SIDE; y += BD_WAVES) {
        bool p = false, t = false;
        if (live && y < h) {
            const int64_t i = frame + y * w + x;
            if (kind == CGS_OBJ_U8) {
                p = static_cast<const uint8_t*>(pred)[i] != 0;
            } else {
                const float v = static_cast<const float*>(pred)[i];
                p = kind == CGS_OBJ_F32_GT ? (v > thresh) : (v >= thresh);    // a NaN compares false
            }
            t = truth[i] != 0;
        }
        const unsigned long long mp = __ballot(p), mt = __ballot(t);
        if (x == 0) {
            s_m[0][y + 1] = mp;
            s_m[1][y + 1] = mt;
        }
    }
    if (threadIdx.x < 4) s_m[threadIdx.x & 1][(threadIdx.x >> 1) * (BD_SIDE + 1)] = 0ull;
    __syncthreads();

    // 2. boundary rows
    if (threadIdx.x < 2 * BD_SIDE) {
        const int side = threadIdx.x / BD_SIDE, r = threadIdx.x & (BD_SIDE - 1);
        const unsigned long long m = s_m[side][r + 1];
        s_b[side][r] = m & ~(s_m[side][r] & s_m[side][r + 2] & (m << 1) & (m >> 1));
    }
    __syncthreads();

    // 3. vertical distances
    {
        const int side = wave & 1, r0 = (wave >> 1) * (BD_SIDE / 2);
        unsigned long long col = 0ull;
        for (int r = 0; r < h; ++r) col |= ((s_b[side][r] >> x) & 1ull) << r;
        for (int r = r0; r < min(r0 + BD_SIDE / 2, h); ++r) {
            const unsigned long long up = col & ((2ull << r) - 1ull), down = col >> r;
            int g2 = BD_NONE;
            if (up) {
                const int g = r - (63 - __clzll((long long)up));
                g2 = g * g;
            }
            if (down) {
                const int g = __ffsll((long long)down) - 1;
                g2 = min(g2, g * g);
            }
            s_d[side][r][x] = g2;
        }
    }
    __syncthreads();

    // 4. horizontal scan, in place
    {
        int sq[BD_SIDE];
#pragma unroll
        for (int c = 0; c < BD_SIDE; ++c) sq[c] = (x - c) * (x - c);
        for (int y = wave; y < h; y += BD_WAVES) {
#pragma unroll
            for (int side = 0; side < 2; ++side) {
                const int4* row = reinterpret_cast<const int4*>(&s_d[side][y][0]);
                int a0 = 2 * BD_NONE, a1 = 2 * BD_NONE;
#pragma unroll
                for (int j = 0; j < BD_SIDE / 4; ++j) {
                    const int4 g = row[j];
                    a0 = min(a0, min(g.x + sq[4 * j], g.y + sq[4 * j + 1]));
                    a1 = min(a1, min(g.z + sq[4 * j + 2], g.w + sq[4 * j + 3]));
                }
                const int d = min(a0, a1);
                s_d[side][y][x] = d;
                if (dist2 && live) dist2[(((int64_t)blockIdx.x * 2 + side) * h + y) * w + x] = d < BD_NONE ? d : -1;
            }
        }
    }
    __syncthreads();

    // 5. counts
    int32_t* cnt = counts + (int64_t)blockIdx.x * (4 + 4 * T);
    if (wave == BD_WAVES - 1) {
        int n_p = 0, n_t = 0, far_p = -1, far_t = -1;
        for (int y = 0; y < h; ++y) {
            const unsigned long long bp = s_b[0][y], bt = s_b[1][y];
            n_p += __popcll(bp);
            n_t += __popcll(bt);
            if ((bp >> x) & 1ull) far_p = max(far_p, s_d[1][y][x]);             // from a predicted boundary pixel to the truth's
            if ((bt >> x) & 1ull) far_t = max(far_t, s_d[0][y][x]);
        }
        far_p = px_wave_max(far_p);
        far_t = px_wave_max(far_t);
        if (x == 0) {
            const bool both = n_p > 0 && n_t > 0;
            cnt[0] = n_p;
            cnt[1] = n_t;
            cnt[2] = both ? far_p : -1;
            cnt[3] = both ? far_t : -1;
        }
    }
    for (int k = wave; k < T; k += BD_WAVES) {
        const int q = min(tol2[k], BD_NONE - 1);                                // an empty side's d2 is >= BD_NONE: within no tolerance
        int hit_p = 0, hit_t = 0, inter = 0, uni = 0;
        for (int y = 0; y < h; ++y) {
            const unsigned long long near_p = __ballot(s_d[0][y][x] <= q), near_t = __ballot(s_d[1][y][x] <= q);
            const unsigned long long P = s_m[0][y + 1] & near_p, G = s_m[1][y + 1] & near_t;
            hit_p += __popcll(s_b[0][y] & near_t);
            hit_t += __popcll(s_b[1][y] & near_p);
            inter += __popcll(P & G);
            uni += __popcll(P | G);
        }
        if (x == 0) {
            cnt[4 + 4 * k] = hit_p;
            cnt[5 + 4 * k] = hit_t;
            cnt[6 + 4 * k] = inter;
            cnt[7 + 4 * k] = uni;
        }
    }
}

}  // namespace

extern "C" int cgs_boundary_score(const void* pred, int32_t pred_kind, float thresh, const uint8_t* truth, int32_t n, int32_t h, int32_t w,
                                  const int32_t* tol2, int32_t T, int32_t* counts, int32_t* dist2, cgs_stream_t stream_) {
    if (!pred || !truth || !tol2 || !counts || n < 1 || h < 1 || w < 1 || pred_kind < CGS_OBJ_U8 || pred_kind > CGS_OBJ_F32_GE || T < 1 ||
        T > CGS_BOUNDARY_MAX_TOL || (pred_kind != CGS_OBJ_U8 && ((uintptr_t)pred & 3u)) || ((uintptr_t)tol2 & 3u) ||
        ((uintptr_t)counts & 3u) || ((uintptr_t)dist2 & 3u))
        return CGS_ERR_BADARG;
    if (h > BD_SIDE || w > BD_SIDE) return CGS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(boundary_kernel, dim3((unsigned)n), dim3(BD_THREADS), 0, (hipStream_t)stream_, pred, (int)pred_kind, thresh, truth,
                       (int)h, (int)w, tol2, (int)T, counts, dist2);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}
