// From per-frame objects to tracks across the frames of one label stack (cgs_objects_track, cgs_objects_track_switches,
// include/cgs_hip.h).  Everything is integer; the only global atomics are integer add / min / max, so nothing depends on an order.
//
//   pairs     cgs_objects_match (objects_match.hip, called, not copied) on frames (f, f + 1) of the same stack gives every object's
//             best partner in the next frame from both sides, and one self-pair of the last frame gives its areas: slot f of `best`
//             in scratch is pair (f, f + 1), slot n - 1 the self-pair, so best[f][0][l - 1][2] is the area of object l of frame f.
//   link      a lane is one (f, l): its side-1 row of pair f - 1 names the partner p, p's side-0 row must name l back, and the
//             threshold must hold; prev and the root pointer ((f - 1) K + p - 1, or itself) are written, the frame's heads are one
//             ballot (kept as a 64-bit mask: a head's rank among them is a popcount below its lane).
//   resolve   pointer doubling root'[i] = root[root[i]] between two buffers, R rounds with 2^R >= n - 1: one launch per round.
//             (A chunked form in LDS was not built: see DESIGN.md.)
//   number    one workgroup scans the per-frame head counts; track number = base[frame of the root] + rank of the root + 1.
//   heads     every head fills the constant fields of its row (first_frame, first_label) and area_min with its own area, in a
//             launch of its own, so that the atomics of the next one start from initialised rows.
//   table     every object adds itself to its track's row: length, area_sum, area_min, area_max, and its backward link's inter and
//             union; the longest length is max(f - first_frame + 1), reduced per workgroup and then one atomic max.
//   paint     one lane per pixel: track_labels and / or rgb.
//
// Launches: init, match (n > 1), self-match, link, R x resolve, number, heads, table, paint: 7 + R + (n > 1), a function of n alone
// (paint is launched also when both its outputs are NULL and then returns at once).
#include "pixel_common.h"

namespace {

constexpr int OT_THREADS = 256;
constexpr int OT_WAVES = OT_THREADS / CGS_WAVE;
constexpr int OT_MAX_K = CGS_OBJ_MATCH_MAX_OBJECTS;
constexpr int OT_SCAN_THREADS = 1024;
static_assert(OT_MAX_K == CGS_WAVE, "one lane per object of a frame");
static_assert((int64_t)CGS_OBJ_TRACK_MAX_FRAMES * OT_MAX_K < (1ll << 31), "root pointers are int32");
static_assert((int64_t)CGS_OBJ_TRACK_MAX_FRAMES * 8191 < (1ll << 31), "area_sum and union_sum stay inside int32");

// scratch, in 32-bit words (the head masks are 64-bit: their offset is even for every n and K)
struct Layout {
    int64_t milli, counts, best, root_a, root_b, heads, base, words;
};
__host__ __device__ inline Layout layout(int64_t n, int64_t K) {
    Layout o;
    o.milli = 0;
    o.counts = 4;
    o.best = o.counts + 4 * n;
    o.root_a = o.best + 8 * n * K;
    o.root_b = o.root_a + n * K;
    o.heads = o.root_b + n * K;
    o.base = o.heads + 2 * n;
    o.words = o.base + n;
    return o;
}

__global__ void __launch_bounds__(OT_THREADS)
track_init_kernel(int32_t* __restrict__ tracks, int64_t words, int32_t* __restrict__ totals, int32_t* __restrict__ milli, int iou) {
    const int64_t step = (int64_t)gridDim.x * OT_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * OT_THREADS + threadIdx.x; i < words; i += step) tracks[i] = 0;
    if (blockIdx.x == 0 && threadIdx.x < 4) {
        totals[threadIdx.x] = 0;
        milli[threadIdx.x] = iou;
    }
}

__global__ void __launch_bounds__(OT_THREADS)
track_link_kernel(const int32_t* __restrict__ best, int n, int K, int iou, int32_t* __restrict__ prev, int32_t* __restrict__ root,
                  unsigned long long* __restrict__ heads, int32_t* __restrict__ totals) {
    __shared__ int s_cnt[2];
    const int lane = threadIdx.x & (CGS_WAVE - 1), wave = threadIdx.x / CGS_WAVE;
    const int f = blockIdx.x * OT_WAVES + wave;
    const bool in = f < n && lane < K;
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int area = in ? best[(((int64_t)f * 2 + 0) * K + lane) * 4 + 2] : 0;
    const bool obj = area > 0;
    int p = 0;
    if (obj && f > 0) {
        const int32_t* row = best + (((int64_t)(f - 1) * 2 + 1) * K + lane) * 4;      // (partner, inter, own area, partner's area)
        const int q = row[0], inter = row[1], uni = row[2] + row[3] - row[1];
        if (q >= 1 && q <= K && inter > 0 && 1000 * inter >= iou * uni &&
            best[(((int64_t)(f - 1) * 2 + 0) * K + q - 1) * 4] == lane + 1)
            p = q;
    }
    if (in) {
        prev[(int64_t)f * K + lane] = p;
        root[(int64_t)f * K + lane] = p ? (f - 1) * K + p - 1 : f * K + lane;
    }
    const unsigned long long head = __ballot(obj && p == 0), objs = __ballot(obj), links = __ballot(p > 0);
    if (lane == 0 && f < n) {
        heads[f] = head;
        if (links) atomicAdd(&s_cnt[0], __popcll(links));
        if (objs) atomicAdd(&s_cnt[1], __popcll(objs));
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&totals[1 + threadIdx.x], s_cnt[threadIdx.x]);
}

__global__ void __launch_bounds__(OT_THREADS)
track_resolve_kernel(const int32_t* __restrict__ src, int32_t* __restrict__ dst, int total) {
    const int i = blockIdx.x * OT_THREADS + threadIdx.x;
    if (i < total) dst[i] = src[src[i]];
}

// exclusive scan of the head counts over the frames, one workgroup: a thread sums a run of frames, the runs' sums are scanned in LDS
__global__ void __launch_bounds__(OT_SCAN_THREADS)
track_number_kernel(const unsigned long long* __restrict__ heads, int n, int32_t* __restrict__ base, int32_t* __restrict__ totals) {
    __shared__ int s_sum[OT_SCAN_THREADS];
    const int t = threadIdx.x, chunk = (n + OT_SCAN_THREADS - 1) / OT_SCAN_THREADS;
    const int lo = min(t * chunk, n), hi = min(lo + chunk, n);
    int sum = 0;
    for (int f = lo; f < hi; ++f) sum += __popcll(heads[f]);
    s_sum[t] = sum;
    __syncthreads();
    for (int d = 1; d < OT_SCAN_THREADS; d <<= 1) {
        const int add = t >= d ? s_sum[t - d] : 0;
        __syncthreads();
        s_sum[t] += add;
        __syncthreads();
    }
    int run = s_sum[t] - sum;
    for (int f = lo; f < hi; ++f) {
        base[f] = run;
        run += __popcll(heads[f]);
    }
    if (t == OT_SCAN_THREADS - 1) totals[0] = s_sum[t];
}

__device__ __forceinline__ int track_number(const unsigned long long* heads, const int32_t* base, int fr, int lr) {
    return base[fr] + __popcll(heads[fr] & ((1ull << lr) - 1ull)) + 1;
}

__global__ void __launch_bounds__(OT_THREADS)
track_heads_kernel(const int32_t* __restrict__ best, const unsigned long long* __restrict__ heads, const int32_t* __restrict__ base,
                   int n, int K, int32_t* __restrict__ tracks, int max_tracks) {
    const int lane = threadIdx.x & (CGS_WAVE - 1);
    const int f = blockIdx.x * OT_WAVES + threadIdx.x / CGS_WAVE;
    if (f >= n || lane >= K || !((heads[f] >> lane) & 1ull)) return;
    const int t = track_number(heads, base, f, lane);
    if (t > max_tracks) return;
    int32_t* row = tracks + (int64_t)(t - 1) * CGS_OBJ_TRACK_FIELDS;
    row[0] = f;
    row[1] = lane + 1;
    row[4] = best[(((int64_t)f * 2 + 0) * K + lane) * 4 + 2];
}

__global__ void __launch_bounds__(OT_THREADS)
track_table_kernel(const int32_t* __restrict__ best, const int32_t* __restrict__ root, const unsigned long long* __restrict__ heads,
                   const int32_t* __restrict__ base, const int32_t* __restrict__ prev, int n, int K, int32_t* __restrict__ track,
                   int32_t* __restrict__ tracks, int max_tracks, int32_t* __restrict__ totals) {
    __shared__ int s_len[OT_WAVES];
    const int lane = threadIdx.x & (CGS_WAVE - 1), wave = threadIdx.x / CGS_WAVE;
    const int f = blockIdx.x * OT_WAVES + wave;
    const bool in = f < n && lane < K;
    const int area = in ? best[(((int64_t)f * 2 + 0) * K + lane) * 4 + 2] : 0;
    int t = 0, len = 0;
    if (area > 0) {
        const int r = root[(int64_t)f * K + lane], fr = r / K, lr = r - fr * K;
        t = track_number(heads, base, fr, lr);
        len = f - fr + 1;
        if (tracks && t <= max_tracks) {
            int32_t* row = tracks + (int64_t)(t - 1) * CGS_OBJ_TRACK_FIELDS;
            atomicAdd(row + 2, 1);
            atomicAdd(row + 3, area);
            atomicMin(row + 4, area);
            atomicMax(row + 5, area);
            if (prev[(int64_t)f * K + lane] > 0) {
                const int32_t* link = best + (((int64_t)(f - 1) * 2 + 1) * K + lane) * 4;
                atomicAdd(row + 6, link[1]);
                atomicAdd(row + 7, link[2] + link[3] - link[1]);
            }
        }
    }
    if (in) track[(int64_t)f * K + lane] = t;
    len = px_wave_max(len);
    if (lane == 0) s_len[wave] = len;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int longest = max(max(s_len[0], s_len[1]), max(s_len[2], s_len[3]));
        if (longest > 0) atomicMax(totals + 3, longest);
    }
}

__global__ void __launch_bounds__(OT_THREADS)
track_paint_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ track, int64_t total, int hw, int K,
                   int32_t* __restrict__ track_labels, uint8_t* __restrict__ rgb) {
    const int64_t i = (int64_t)blockIdx.x * OT_THREADS + threadIdx.x;
    if (i >= total || (!track_labels && !rgb)) return;
    const int l = labels[i];
    const int t = (l >= 1 && l <= K) ? track[(i / hw) * K + l - 1] : 0;
    if (track_labels) track_labels[i] = t;
    if (rgb) {
        const uint32_t hsh = (uint32_t)t * 2654435761u;
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[3 * i + c] = t ? (uint8_t)(64u + ((hsh >> (8 * c)) & 255u) * 191u / 255u) : (uint8_t)0;
    }
}

// Identity switches of a prediction's tracks against the truth's: a lane is one truth object (f, q).  Gaps are not bridged.
__global__ void __launch_bounds__(OT_THREADS)
track_switches_kernel(const int32_t* __restrict__ truth_prev, const int32_t* __restrict__ pred_track, const int32_t* __restrict__ mb,
                      const int32_t* __restrict__ iou_milli, int T, int n, int K, int32_t* __restrict__ counts) {
    __shared__ int s_cnt[CGS_OBJ_MATCH_MAX_IOU * 3];
    const int lane = threadIdx.x & (CGS_WAVE - 1);
    const int f = blockIdx.x * OT_WAVES + threadIdx.x / CGS_WAVE;
    const bool in = f < n && lane < K;
    if (threadIdx.x < 3 * T) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    int inter = 0, uni = 1, trk = 0, inter0 = 0, uni0 = 1, trk0 = -1;
    bool linked = false;
    if (in) {
        const int32_t* row = mb + (((int64_t)f * 2 + 1) * K + lane) * 4;                // (pred partner, inter, area_t, area_p)
        const int p = row[0];
        inter = row[1];
        uni = row[2] + row[3] - row[1];
        if (p >= 1 && p <= K) trk = pred_track[(int64_t)f * K + p - 1];
        const int q0 = f > 0 ? truth_prev[(int64_t)f * K + lane] : 0;
        if (q0 >= 1 && q0 <= K) {
            linked = true;
            const int32_t* row0 = mb + (((int64_t)(f - 1) * 2 + 1) * K + q0 - 1) * 4;
            const int p0 = row0[0];
            inter0 = row0[1];
            uni0 = row0[2] + row0[3] - row0[1];
            if (p0 >= 1 && p0 <= K) trk0 = pred_track[(int64_t)(f - 1) * K + p0 - 1];
        }
    }
    for (int k = 0; k < T; ++k) {
        const int m = iou_milli[k];
        const bool cov = in && inter > 0 && 1000 * inter >= m * uni;
        const bool cont = cov && linked && inter0 > 0 && 1000 * inter0 >= m * uni0;
        const unsigned long long b0 = __ballot(cov), b1 = __ballot(cont), b2 = __ballot(cont && trk != trk0);
        if (lane == 0) {
            if (b0) atomicAdd(&s_cnt[3 * k + 0], __popcll(b0));
            if (b1) atomicAdd(&s_cnt[3 * k + 1], __popcll(b1));
            if (b2) atomicAdd(&s_cnt[3 * k + 2], __popcll(b2));
        }
    }
    __syncthreads();
    if (threadIdx.x < 3 * T && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], s_cnt[threadIdx.x]);
}

inline unsigned blocks_for(int64_t items, int per) { return (unsigned)((items + per - 1) / per); }

}  // namespace

extern "C" int64_t cgs_objects_track_scratch_bytes(int32_t n, int32_t max_objects) {
    if (n < 1 || max_objects < 1) return 0;
    const unsigned __int128 words = (unsigned __int128)n * (7u + 10u * (unsigned __int128)max_objects) + 4u;       // layout().words
    return words * 4u > (unsigned __int128)INT64_MAX ? INT64_MAX : (int64_t)(words * 4u);        // saturates: no buffer is that large
}

extern "C" int cgs_objects_track(const int32_t* labels, int32_t n, int32_t h, int32_t w, int32_t max_objects, int32_t iou_milli,
                                 int32_t max_tracks, int32_t* prev, int32_t* track, int32_t* totals, int32_t* tracks,
                                 int32_t* track_labels, uint8_t* rgb, void* scratch, int64_t scratch_bytes, cgs_stream_t stream_) {
    if (!labels || !prev || !track || !totals || !scratch || n < 1 || h < 1 || w < 1 || max_objects < 1 || max_tracks < 1 ||
        iou_milli < 1 || iou_milli > 1000 || ((uintptr_t)labels & 3u) || ((uintptr_t)prev & 3u) || ((uintptr_t)track & 3u) ||
        ((uintptr_t)totals & 3u) || ((uintptr_t)tracks & 3u) || ((uintptr_t)track_labels & 3u) || ((uintptr_t)scratch & 7u) ||
        scratch_bytes < cgs_objects_track_scratch_bytes(n, max_objects))
        return CGS_ERR_BADARG;
    if (h > CGS_OBJ_MAX_SIDE || w > CGS_OBJ_MAX_SIDE || max_objects > OT_MAX_K || n > CGS_OBJ_TRACK_MAX_FRAMES) return CGS_ERR_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    const int K = max_objects, hw = h * w;
    const Layout o = layout(n, K);
    int32_t* s = static_cast<int32_t*>(scratch);
    int32_t *milli = s + o.milli, *counts = s + o.counts, *best = s + o.best, *root_a = s + o.root_a, *root_b = s + o.root_b,
            *base = s + o.base;
    unsigned long long* heads = reinterpret_cast<unsigned long long*>(s + o.heads);
    const unsigned frames4 = blocks_for(n, OT_WAVES);

    const int64_t words = tracks ? (int64_t)max_tracks * CGS_OBJ_TRACK_FIELDS : 0;
    const int64_t want_blocks = (words + OT_THREADS - 1) / OT_THREADS;
    const unsigned init_blocks = (unsigned)(want_blocks < 1 ? 1 : want_blocks > 4096 ? 4096 : want_blocks);
    hipLaunchKernelGGL(track_init_kernel, dim3(init_blocks), dim3(OT_THREADS), 0, stream, tracks, words, totals, milli, (int)iou_milli);
    CGS_HIP_CHECK_LAUNCH();
    if (n > 1) {
        const int rc = cgs_objects_match(labels, labels + hw, n - 1, h, w, K, milli, 1, counts, best, stream_);
        if (rc != CGS_OK) return rc;
    }
    const int32_t* last = labels + (int64_t)(n - 1) * hw;
    const int rc = cgs_objects_match(last, last, 1, h, w, K, milli, 1, counts + 4 * (int64_t)(n - 1), best + 8 * (int64_t)(n - 1) * K, stream_);
    if (rc != CGS_OK) return rc;
    hipLaunchKernelGGL(track_link_kernel, dim3(frames4), dim3(OT_THREADS), 0, stream, best, (int)n, K, (int)iou_milli, prev, root_a, heads,
                       totals);
    CGS_HIP_CHECK_LAUNCH();
    const int total = n * K;
    for (int reach = 1; reach < n - 1; reach <<= 1) {                     // R rounds, 2^R >= n - 1
        hipLaunchKernelGGL(track_resolve_kernel, dim3(blocks_for(total, OT_THREADS)), dim3(OT_THREADS), 0, stream, root_a, root_b, total);
        CGS_HIP_CHECK_LAUNCH();
        int32_t* swap = root_a;
        root_a = root_b;
        root_b = swap;
    }
    hipLaunchKernelGGL(track_number_kernel, dim3(1), dim3(OT_SCAN_THREADS), 0, stream, heads, (int)n, base, totals);
    CGS_HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(track_heads_kernel, dim3(frames4), dim3(OT_THREADS), 0, stream, best, heads, base, (int)n, K,
                       tracks, tracks ? (int)max_tracks : 0);
    CGS_HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(track_table_kernel, dim3(frames4), dim3(OT_THREADS), 0, stream, best, root_a, heads, base, prev, (int)n, K, track,
                       tracks, (int)max_tracks, totals);
    CGS_HIP_CHECK_LAUNCH();
    const int64_t pixels = (int64_t)n * hw;
    hipLaunchKernelGGL(track_paint_kernel, dim3(blocks_for(pixels, OT_THREADS)), dim3(OT_THREADS), 0, stream, labels, track, pixels, hw, K,
                       track_labels, rgb);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}

extern "C" int cgs_objects_track_switches(const int32_t* truth_prev, const int32_t* pred_track, const int32_t* match_best,
                                          const int32_t* iou_milli, int32_t T, int32_t n, int32_t max_objects, int32_t* counts,
                                          cgs_stream_t stream_) {
    if (!truth_prev || !pred_track || !match_best || !iou_milli || !counts || T < 1 || T > CGS_OBJ_MATCH_MAX_IOU || n < 1 ||
        max_objects < 1 || ((uintptr_t)truth_prev & 3u) || ((uintptr_t)pred_track & 3u) || ((uintptr_t)match_best & 3u) ||
        ((uintptr_t)iou_milli & 3u) || ((uintptr_t)counts & 3u))
        return CGS_ERR_BADARG;
    if (max_objects > OT_MAX_K || n > CGS_OBJ_TRACK_MAX_FRAMES) return CGS_ERR_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    const hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * 3 * (size_t)T, stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(track_switches_kernel, dim3(blocks_for(n, OT_WAVES)), dim3(OT_THREADS), 0, stream, truth_prev, pred_track,
                       match_best, iou_milli, (int)T, (int)n, (int)max_objects, counts);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}
