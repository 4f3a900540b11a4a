// Mask clean-up between "probabilities" and "objects": threshold, hysteresis, morphological opening and closing, filling of small holes
// (cgs_mask_clean, include/cgs_hip.h), for a stack of frames of at most 64 x 64 pixels.  One workgroup of four waves per frame; the
// frame is 64 bit rows in LDS (s_row, bits at and beyond w clear).  Everything is integer or selection, so the result does not depend
// on the order in which anything below happens.
//
//   1. on      a lane is a column, a wave takes the rows wave, wave + 4, ...: one __ballot gives a row's on-mask, a second one the mask
//              of its strong pixels (hysteresis only)
//   2. hyst    the on pixels are labelled with the run-based union-find of unionfind_rows.h (as csrc/objects.hip labels them); a run
//              that holds a strong pixel sets its root's flag, and a pixel stays when its root's flag is set
//   3. morph   wave 0 alone, in registers: lane y holds row y.  A dilation step is the row shifted left and right, and the rows of the
//              lanes y - 1 and y + 1 (two shuffles), ORed; lanes at and beyond h hold 0 and a shift moves zeros in, so outside the
//              frame is off.  An erosion step is the dilation of the complement inside the frame, complemented: outside is on.  The
//              two structuring elements are symmetric, so this is the erosion.  At most 4 x 4 steps, no LDS traffic, no barrier
//   4. fill    the OFF pixels are labelled at the complementary connectivity; a run adds its length to its root, and 2^16 when it
//              touches the first or last row or column (areas stay below 2^13, at most 2^12 runs: no carry, no overflow).  A root whose
//              sum is below 2^16 is a hole; its pixels are turned on when the sum is at most fill_area
//   5. output  out, gated (the source is read a second time: selection only), counts
//
// Pixel counts are taken by wave 0 from the rows (one popcount per lane, one wave sum); root counts per row by ballot and popcount.
// LDS: 2 x 16 KiB (L, A) + 1.5 KiB of rows and counts = 33.5 KiB, four workgroups per CU.
#include "cgs_common.h"
#include "unionfind_rows.h"

namespace {

constexpr int CLN_THREADS = 256;
constexpr int CLN_WAVES = CLN_THREADS / CGS_WAVE;
constexpr int CLN_MAX_SIDE = 64;                      // a row is one wave-wide ballot
constexpr int CLN_MAX_PX = CLN_MAX_SIDE * CLN_MAX_SIDE;
constexpr int CLN_EDGE = 1 << 16;                     // added to a root's area by a run on the frame's edge

typedef unsigned long long row_t;

__device__ __forceinline__ int wave_sum_int(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, CGS_WAVE);
    return v;
}

// The forest of the set pixels of rows[0..h) in L (flattened: L[p] is p's root, the first pixel of its component; -1 where the pixel
// is clear) and A = 0 everywhere.  Every thread of the workgroup calls this; on return the forest is complete and visible.
__device__ __forceinline__ void label_rows(int* L, int* A, const row_t* rows, int h, int w, bool conn8, int x, int wave, row_t lt) {
    for (int y = wave; y < h; y += CLN_WAVES) {
        if (x >= w) continue;
        const row_t m = rows[y];
        const int p = y * w + x;
        L[p] = ((m >> x) & 1ull) ? y * w + run_start(m, lt) : -1;
        A[p] = 0;
    }
    __syncthreads();
    for (int y = wave; y < h; y += CLN_WAVES) {
        if (y == 0) continue;
        const row_t cur = rows[y], up = rows[y - 1];
        if ((cur >> x) & 1ull) unite_with_row_above(L, cur, up, y, x, w, conn8);
    }
    __syncthreads();
    for (int y = wave; y < h; y += CLN_WAVES) {           // (a parent read here is the old one or already the root: both lead to the root)
        if ((rows[y] >> x) & 1ull) {
            const int p = y * w + x;
            lds_put(&L[p], find_root(L, p));
        }
    }
    __syncthreads();
}

// one step of the dilation over the lanes of wave 0 (lane y = row y); m is 0 in the lanes at and beyond h
__device__ __forceinline__ row_t dilate_step(row_t m, bool cross, int lane, row_t wmask) {
    const row_t hor = (m | (m << 1) | (m >> 1)) & wmask;
    const row_t v = cross ? m : hor;
    const row_t a = __shfl_up(v, 1, CGS_WAVE), b = __shfl_down(v, 1, CGS_WAVE);
    return hor | (lane > 0 ? a : 0ull) | (lane < CGS_WAVE - 1 ? b : 0ull);
}

__device__ __forceinline__ row_t dilate(row_t m, int r, bool cross, int lane, bool inside, row_t wmask) {
    for (int i = 0; i < r; ++i) {                         // (every lane shuffles; the lanes below the frame then drop what they got)
        m = dilate_step(m, cross, lane, wmask);
        if (!inside) m = 0ull;
    }
    return m;
}

__device__ __forceinline__ row_t erode(row_t m, int r, bool cross, int lane, bool inside, row_t wmask) {
    const row_t c = dilate(inside ? ~m & wmask : 0ull, r, cross, lane, inside, wmask);
    return inside ? ~c & wmask : 0ull;
}

__global__ void __launch_bounds__(CLN_THREADS)
clean_kernel(const void* __restrict__ src, int kind, float thresh, int hyst, float strong, int h, int w, int conn8, int cross, int open_r,
             int close_r, int fill_area, uint8_t* __restrict__ out, float* __restrict__ gated, int32_t* __restrict__ counts) {
    __shared__ int s_L[CLN_MAX_PX];
    __shared__ int s_A[CLN_MAX_PX];
    __shared__ row_t s_row[CLN_MAX_SIDE];             // the mask
    __shared__ row_t s_aux[CLN_MAX_SIDE];             // the strong pixels (hyst), then the off pixels (fill)
    __shared__ int s_cnt[2][CLN_MAX_SIDE];            // per row: two root counts of the stage at hand
    __shared__ int s_out[8];
    const int x = threadIdx.x & (CGS_WAVE - 1), wave = threadIdx.x / CGS_WAVE;
    const row_t lt = (1ull << x) - 1ull;
    const row_t wmask = w == 64 ? ~0ull : (1ull << w) - 1ull;
    const bool live = x < w;
    const int64_t frame = (int64_t)blockIdx.x * h * w;

    // 1. on
    for (int y = wave; y < h; y += CLN_WAVES) {
        bool on = false, st = false;
        if (live) {
            const int p = y * w + x;
            if (kind == 0) {
                on = static_cast<const uint8_t*>(src)[frame + p] != 0;
            } else {
                const float v = static_cast<const float*>(src)[frame + p];
                on = kind == 1 ? (v > thresh) : (v >= thresh);            // a NaN compares false
                st = kind == 1 ? (v > strong) : (v >= strong);
            }
        }
        const row_t m = __ballot(on), ms = __ballot(st);
        if (x == 0) {
            s_row[y] = m;
            s_aux[y] = ms;
        }
    }
    if (threadIdx.x < 8) s_out[threadIdx.x] = 0;
    __syncthreads();
    if (wave == 0) {
        const int c = wave_sum_int(x < h ? __popcll(s_row[x]) : 0);
        if (x == 0) s_out[0] = s_out[1] = c;
    }

    // 2. hyst
    if (hyst) {
        label_rows(s_L, s_A, s_row, h, w, conn8 != 0, x, wave, lt);
        for (int y = wave; y < h; y += CLN_WAVES) {                       // a run with a strong pixel flags its root
            const row_t cur = s_row[y];
            const bool on = (cur >> x) & 1ull, end = on && (x == 63 || !((cur >> (x + 1)) & 1ull));
            if (end) {
                const int s = run_start(cur, lt);
                const row_t run = (x == 63 ? ~0ull : (1ull << (x + 1)) - 1ull) & ~((1ull << s) - 1ull);
                if (s_aux[y] & run) lds_put(&s_A[s_L[y * w + x]], 1);
            }
        }
        __syncthreads();
        for (int y = wave; y < h; y += CLN_WAVES) {
            const row_t cur = s_row[y];
            const bool on = (cur >> x) & 1ull;
            const int p = y * w + x;
            const bool keep = on && s_A[s_L[p]] != 0;
            const bool dropped_root = on && s_L[p] == p && s_A[p] == 0;
            const row_t mk = __ballot(keep), md = __ballot(dropped_root);
            if (x == 0) {
                s_row[y] = mk;                                            // (a wave reads no rows but its own in this loop)
                s_cnt[0][y] = __popcll(md);
            }
        }
        __syncthreads();
        if (wave == 0) {
            const int c = wave_sum_int(x < h ? __popcll(s_row[x]) : 0), d = wave_sum_int(x < h ? s_cnt[0][x] : 0);
            if (x == 0) {
                s_out[1] = c;
                s_out[5] = d;
            }
        }
        __syncthreads();
    }

    // 3. open, close
    if (wave == 0) {
        const bool inside = x < h;
        row_t m = inside ? s_row[x] : 0ull;
        if (open_r) m = dilate(erode(m, open_r, cross != 0, x, inside, wmask), open_r, cross != 0, x, inside, wmask);
        const int c2 = wave_sum_int(__popcll(m));
        if (close_r) m = erode(dilate(m, close_r, cross != 0, x, inside, wmask), close_r, cross != 0, x, inside, wmask);
        const int c3 = wave_sum_int(__popcll(m));
        if (inside) {
            s_row[x] = m;
            s_aux[x] = ~m & wmask;
        }
        if (x == 0) {
            s_out[2] = c2;
            s_out[3] = s_out[4] = c3;
        }
    }
    __syncthreads();

    // 4. fill
    if (fill_area) {
        label_rows(s_L, s_A, s_aux, h, w, conn8 == 0, x, wave, lt);
        for (int y = wave; y < h; y += CLN_WAVES) {
            const row_t off = s_aux[y];
            const bool is = (off >> x) & 1ull, end = is && (x == 63 || !((off >> (x + 1)) & 1ull));
            if (end) {
                const int s = run_start(off, lt);
                const bool edge = y == 0 || y == h - 1 || s == 0 || x == w - 1;
                atomicAdd(&s_A[s_L[y * w + x]], x - s + 1 + (edge ? CLN_EDGE : 0));
            }
        }
        __syncthreads();
        for (int y = wave; y < h; y += CLN_WAVES) {
            const row_t off = s_aux[y];
            const bool is = (off >> x) & 1ull;
            const int p = y * w + x;
            const int a = is ? s_A[s_L[p]] : CLN_EDGE;
            const bool root = is && s_L[p] == p;
            const row_t mfill = __ballot(a <= fill_area), mh = __ballot(root && a < CLN_EDGE), mf = __ballot(root && a <= fill_area);
            if (x == 0) {
                s_row[y] |= mfill;
                s_cnt[0][y] = __popcll(mh);
                s_cnt[1][y] = __popcll(mf);
            }
        }
        __syncthreads();
        if (wave == 0) {
            const int c = wave_sum_int(x < h ? __popcll(s_row[x]) : 0);
            const int nh = wave_sum_int(x < h ? s_cnt[0][x] : 0), nf = wave_sum_int(x < h ? s_cnt[1][x] : 0);
            if (x == 0) {
                s_out[4] = c;
                s_out[6] = nh;
                s_out[7] = nf;
            }
        }
        __syncthreads();
    }

    // 5. output
    for (int y = wave; y < h; y += CLN_WAVES) {
        if (!live) continue;
        const int p = y * w + x;
        const bool on = (s_row[y] >> x) & 1ull;
        out[frame + p] = on;
        if (gated) {
            const float v = static_cast<const float*>(src)[frame + p];
            const bool pass = kind == 1 ? (v > thresh) : (v >= thresh);
            gated[frame + p] = on ? (pass ? v : thresh) : 0.f;
        }
    }
    if (threadIdx.x < 8) counts[8 * (int64_t)blockIdx.x + threadIdx.x] = s_out[threadIdx.x];
}

}  // namespace

extern "C" int cgs_mask_clean(const void* src, int32_t src_kind, float thresh, int32_t hyst, float strong, int32_t n, int32_t h, int32_t w,
                              int32_t connectivity, int32_t shape, int32_t open_r, int32_t close_r, int32_t fill_area, uint8_t* out,
                              float* gated, int32_t* counts, cgs_stream_t stream_) {
    if (!src || !out || !counts || n < 1 || src_kind < 0 || src_kind > 2 || (connectivity != 4 && connectivity != 8) ||
        (shape != CGS_CLEAN_SQUARE && shape != CGS_CLEAN_CROSS) || open_r < 0 || open_r > CGS_CLEAN_MAX_RADIUS || close_r < 0 ||
        close_r > CGS_CLEAN_MAX_RADIUS || fill_area < 0 || fill_area > CLN_MAX_PX)
        return CGS_ERR_BADARG;
    if (hyst && (src_kind == CGS_OBJ_U8 || !(strong - strong == 0.f) || strong < thresh)) return CGS_ERR_BADARG;      // (inf - inf is a NaN)
    if (gated && (src_kind == CGS_OBJ_U8 || !(thresh > 0.f))) return CGS_ERR_BADARG;
    if ((src_kind != CGS_OBJ_U8 && ((uintptr_t)src & 3u)) || ((uintptr_t)gated & 3u) || ((uintptr_t)counts & 3u)) return CGS_ERR_BADARG;
    if (h < 1 || w < 1 || h > CLN_MAX_SIDE || w > CLN_MAX_SIDE) return CGS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(clean_kernel, dim3((unsigned)n), dim3(CLN_THREADS), 0, (hipStream_t)stream_, src, (int)src_kind, thresh, (int)(hyst != 0),
                       strong, (int)h, (int)w, (int)(connectivity == 8), (int)(shape == CGS_CLEAN_CROSS), (int)open_r, (int)close_r,
                       (int)fill_area, out, gated, counts);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}
