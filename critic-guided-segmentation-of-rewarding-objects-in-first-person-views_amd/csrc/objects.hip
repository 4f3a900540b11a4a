// From masks to objects: connected-component labelling of a stack of frames of at most 64 x 64 pixels, the area filter, the numbering
// of scipy.ndimage.label (kept components 1..K in raster order of their first pixel) and the per-object table (cgs_objects_label,
// include/cgs_hip.h).  One workgroup of four waves labels one frame in LDS; everything is integer, so the result does not depend on the
// order in which anything below happens.
//
// A lane is a column and a wave takes the rows wave, wave + 4, ...: one __ballot gives the row's on-mask, and every question about a
// pixel's neighbours is a bit of that mask or of the mask of the row above (s_row).  Bits at and beyond w are clear and a shift moves
// zeros in, so the end of one row and the start of the next are never neighbours; the LDS index of a pixel is its raster index y w + x.
//
//   1. load      on-mask per row; L[p] = raster index of the start of p's horizontal run (a run is connected whatever happens elsewhere)
//   2. merge     union-find over L: a pixel whose run touches a run of the row above unites the two (once per pair of touching runs,
//                by the leftmost pixel of the contact).  unite() follows parents to the two roots and hangs the larger root below the
//                smaller one with an LDS atomic min; when another lane got there first it goes on from what it displaced.  Parents only
//                ever decrease, so every loop ends, and after the barrier the forest is exact: there is no sweep count that a long path
//                (the 2111-pixel spiral) could exceed, and no iteration cap.
//   3. flatten   L[p] = root of p = the smallest raster index of p's component = its first pixel
//   4. area      one LDS atomic add per RUN (its length) to A[root]
//   5. rank      a root is kept when its area reaches min_area; kept and found roots are counted per row (ballot + popcount), wave 0
//                turns the 64 row counts into exclusive bases, and a kept root's number is base[y] + #kept roots to its left + 1.
//                The number replaces the area in A[root]
//   6. output    labels = A[L[p]], kept_mask = labels != 0, count = (kept, found)
//   7. table     rows of the first min(kept, max_objects) objects, 256 objects at a time through one LDS block of accumulators
//                (again one atomic per run and field); the rows after them are zeroed
//
// LDS: 2 x 16 KiB (L, A) + 8 KiB of accumulators + 1.3 KiB of row data = 41.3 KiB, three workgroups per CU.
#include <algorithm>

#include "cgs_common.h"
#include "unionfind_rows.h"

namespace {

constexpr int OBJ_THREADS = 256;
constexpr int OBJ_WAVES = OBJ_THREADS / CGS_WAVE;
constexpr int OBJ_MAX_SIDE = 64;                      // a row is one wave-wide ballot
constexpr int OBJ_MAX_PX = OBJ_MAX_SIDE * OBJ_MAX_SIDE;
constexpr int OBJ_CHUNK = 256;                        // objects per pass of the table
constexpr int OBJ_FIELDS = 8;                         // area, x0, y0, x1, y1, sum_x, sum_y, first

__global__ void __launch_bounds__(OBJ_THREADS)
objects_kernel(const void* __restrict__ src, int kind, float thresh, int h, int w, int conn8, int min_area, int max_objects,
               int32_t* __restrict__ labels, uint8_t* __restrict__ kept_mask, int32_t* __restrict__ count, int32_t* __restrict__ table) {
    __shared__ int s_L[OBJ_MAX_PX];
    __shared__ int s_A[OBJ_MAX_PX];
    __shared__ int s_acc[OBJ_CHUNK * OBJ_FIELDS];
    __shared__ unsigned long long s_row[OBJ_MAX_SIDE];
    __shared__ int s_cnt[2][OBJ_MAX_SIDE];            // per row: kept roots (then their exclusive base), found roots
    __shared__ int s_tot[2];
    const int x = threadIdx.x & (CGS_WAVE - 1), wave = threadIdx.x / CGS_WAVE;
    const unsigned long long lt = (1ull << x) - 1ull;
    const bool live = x < w;
    const int64_t frame = (int64_t)blockIdx.x * h * w;

    // 1. load
    for (int y = wave; y < h; y += OBJ_WAVES) {
        const int p = y * w + x;
        bool on = false;
        if (live) {
            if (kind == 0) {
                on = static_cast<const uint8_t*>(src)[frame + p] != 0;
            } else {
                const float v = static_cast<const float*>(src)[frame + p];
                on = kind == 1 ? (v > thresh) : (v >= thresh);            // a NaN compares false
            }
        }
        const unsigned long long m = __ballot(on);
        if (x == 0) s_row[y] = m;
        if (live) {
            s_L[p] = on ? y * w + run_start(m, lt) : -1;
            s_A[p] = 0;
        }
    }
    __syncthreads();

    // 2. merge with the row above
    for (int y = wave; y < h; y += OBJ_WAVES) {
        if (y == 0) continue;
        const unsigned long long cur = s_row[y], up = s_row[y - 1];
        if ((cur >> x) & 1ull) unite_with_row_above(s_L, cur, up, y, x, w, conn8 != 0);
    }
    __syncthreads();

    // 3. flatten (a parent read here is the old one or already the root: both lead to the root)
    for (int y = wave; y < h; y += OBJ_WAVES) {
        if ((s_row[y] >> x) & 1ull) {
            const int p = y * w + x;
            lds_put(&s_L[p], find_root(s_L, p));
        }
    }
    __syncthreads();

    // 4. area, one add per run
    for (int y = wave; y < h; y += OBJ_WAVES) {
        const unsigned long long cur = s_row[y];
        const bool on = (cur >> x) & 1ull, end = on && (x == 63 || !((cur >> (x + 1)) & 1ull));
        if (end) atomicAdd(&s_A[s_L[y * w + x]], x - run_start(cur, lt) + 1);
    }
    __syncthreads();

    // 5. roots per row, in raster order
    for (int y = wave; y < h; y += OBJ_WAVES) {
        const int p = y * w + x;
        const bool root = ((s_row[y] >> x) & 1ull) && s_L[p] == p;
        const bool keep = root && s_A[p] >= min_area;
        const unsigned long long mk = __ballot(keep), mf = __ballot(root);
        if (x == 0) {
            s_cnt[0][y] = __popcll(mk);
            s_cnt[1][y] = __popcll(mf);
        }
    }
    __syncthreads();
    if (wave == 0) {
        const int ck = x < h ? s_cnt[0][x] : 0, cf = x < h ? s_cnt[1][x] : 0;
        int vk = ck, vf = cf;
#pragma unroll
        for (int d = 1; d < CGS_WAVE; d <<= 1) {
            const int tk = __shfl_up(vk, d, CGS_WAVE), tf = __shfl_up(vf, d, CGS_WAVE);
            if (x >= d) {
                vk += tk;
                vf += tf;
            }
        }
        s_cnt[0][x] = vk - ck;
        if (x == CGS_WAVE - 1) {
            s_tot[0] = vk;
            s_tot[1] = vf;
            count[2 * (int64_t)blockIdx.x] = vk;
            count[2 * (int64_t)blockIdx.x + 1] = vf;
        }
    }
    __syncthreads();
    for (int y = wave; y < h; y += OBJ_WAVES) {
        const int p = y * w + x;
        const bool root = ((s_row[y] >> x) & 1ull) && s_L[p] == p;      // s_A[p] of a root is read and written by its own lane only
        const bool keep = root && s_A[p] >= min_area;
        const unsigned long long mk = __ballot(keep);
        if (root) s_A[p] = keep ? s_cnt[0][y] + __popcll(mk & lt) + 1 : 0;
    }
    __syncthreads();

    // 6. output
    if (labels || kept_mask) {
        for (int y = wave; y < h; y += OBJ_WAVES) {
            if (!live) continue;
            const int p = y * w + x;
            const int lab = ((s_row[y] >> x) & 1ull) ? s_A[s_L[p]] : 0;
            if (labels) labels[frame + p] = lab;
            if (kept_mask) kept_mask[frame + p] = lab != 0;
        }
    }

    // 7. table
    if (!table) return;
    const int limit = min(s_tot[0], max_objects);
    int32_t* tab = table + (int64_t)blockIdx.x * max_objects * OBJ_FIELDS;
    for (int64_t j = (int64_t)limit * OBJ_FIELDS + threadIdx.x; j < (int64_t)max_objects * OBJ_FIELDS; j += OBJ_THREADS) tab[j] = 0;
    for (int c0 = 0; c0 < limit; c0 += OBJ_CHUNK) {
        const int rows = min(OBJ_CHUNK, limit - c0);
        for (int j = threadIdx.x; j < OBJ_CHUNK * OBJ_FIELDS; j += OBJ_THREADS) {
            const int field = j & (OBJ_FIELDS - 1);
            s_acc[j] = (field == 1 || field == 2) ? 0x7FFFFFFF : 0;          // the two minima
        }
        __syncthreads();
        for (int y = wave; y < h; y += OBJ_WAVES) {
            const unsigned long long cur = s_row[y];
            if (!((cur >> x) & 1ull)) continue;
            const int p = y * w + x, r = s_L[p];
            const int k = s_A[r] - 1 - c0;                                   // -1 - c0 for a removed component
            if (k < 0 || k >= rows) continue;
            int* a = s_acc + k * OBJ_FIELDS;
            if (r == p) a[7] = p;
            if (x == 63 || !((cur >> (x + 1)) & 1ull)) {                     // the run's last pixel speaks for the run
                const int s = run_start(cur, lt), len = x - s + 1;
                atomicAdd(&a[0], len);
                atomicMin(&a[1], s);
                atomicMin(&a[2], y);
                atomicMax(&a[3], x);
                atomicMax(&a[4], y);
                atomicAdd(&a[5], (s + x) * len / 2);
                atomicAdd(&a[6], y * len);
            }
        }
        __syncthreads();
        for (int j = threadIdx.x; j < rows * OBJ_FIELDS; j += OBJ_THREADS) tab[(int64_t)c0 * OBJ_FIELDS + j] = s_acc[j];
        __syncthreads();
    }
}

}  // namespace

extern "C" int cgs_objects_label(const void* src, int32_t src_kind, float thresh, int32_t n, int32_t h, int32_t w, int32_t connectivity,
                                 int32_t min_area, int32_t max_objects, int32_t* labels, uint8_t* kept_mask, int32_t* count,
                                 int32_t* table, cgs_stream_t stream_) {
    if (!src || !count || n < 1 || h < 1 || w < 1 || src_kind < 0 || src_kind > 2 || (connectivity != 4 && connectivity != 8) ||
        min_area < 1 || max_objects < 1 || (src_kind != 0 && ((uintptr_t)src & 3u)) || ((uintptr_t)labels & 3u) ||
        ((uintptr_t)count & 3u) || ((uintptr_t)table & 3u))
        return CGS_ERR_BADARG;
    if (h > OBJ_MAX_SIDE || w > OBJ_MAX_SIDE) return CGS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(objects_kernel, dim3((unsigned)n), dim3(OBJ_THREADS), 0, (hipStream_t)stream_, src, (int)src_kind, thresh, (int)h,
                       (int)w, (int)(connectivity == 8), (int)min_area, (int)max_objects, labels, kept_mask, count, table);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}
