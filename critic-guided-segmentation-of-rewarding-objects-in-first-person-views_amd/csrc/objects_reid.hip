// From tracks to identities: a colour histogram per track and the chaining of tracks that do not overlap in time, lie at most W frames
// apart and have the same histogram (cgs_objects_appearance, cgs_objects_reid; the rule is their header comment in include/cgs_hip.h).
// Everything is integer; the global atomics are int32 add / max and one unsigned 64-bit max, so nothing depends on an order.
//
//   appearance  one workgroup of four waves per frame, the K x 64 histogram in LDS (16 KiB at K = 64).  A lane is a column and a wave
//               takes the rows wave, wave + 4, ... as objects_match.hip does; a pixel's key is (label, bin), one __ballot gives the row's
//               run boundaries and the last lane of a run adds the run's length once -- an object of one colour is one LDS add per row,
//               not one per pixel on one address.  Flush: H row by row as it lies; for S a wave takes a label, a lane a bin, and the
//               non-zero bins go to S[t - 1] as int32 atomic adds, one contiguous 256-byte row per wave instruction.
//   signature   one wave per track, a lane per bin: A by a wave sum, Q = floor(S 4096 / A) (32-bit when S 4096 < 2^32, which A < 2^20
//               guarantees for the whole wave, else 64-bit), D by a second wave sum; F, L, D go to scratch.  The same launch builds
//               start[f], f = 0 .. n: the first track whose first frame is >= f, a binary search over the table's monotone first column
//               bounded by the device-side n_tracks.
//   pair        one wave per track t, a lane per candidate u of start[L + 1] .. start[L + W + 1]: Q_t is staged in LDS and read back as
//               eight 16-byte broadcasts that stay in registers, Q_u is eight 16-byte loads of the lane's own row, and the 64 minima
//               and their sum are 32 packed 16-bit min and 32 packed 16-bit add (a half's sum is at most 4096).  No cross-lane traffic
//               until the one wave-wide max at the end that gives succ[t]; pred[u] is an unsigned 64-bit atomic max of
//               (s << 32) | (0xFFFFFFFF - t), issued for admissible pairs only: the largest s, then the smallest t.
//   link        a lane per track: the link backwards when pred[u] = t and succ[t] = u, the link forwards likewise; root pointer and
//               depth (0 / 1) for the doubling.
//   resolve     root'[i] = root[root[i]], depth'[i] = depth[i] + depth[root[i]] between two buffers, one launch per round, R rounds
//               with 2^R >= min(n, max_tracks) - 1: the members of a chain do not overlap in time, so a chain has at most n of them.
//   number      one workgroup scans the tracks without a link backwards; an identity's number is its first track's rank among them.
//   finish      identity[i] = rank[root[i]], the longest chain is max(depth) + 1: one atomic max per workgroup.
//
// Launches: two memsets, signature, pair, link, R x resolve, number, finish: a function of n and max_tracks alone.
#include "pixel_common.h"

namespace {

constexpr int OR_THREADS = 256;
constexpr int OR_WAVES = OR_THREADS / CGS_WAVE;
constexpr int OR_BINS = CGS_OBJ_REID_BINS;
constexpr int OR_MAX_K = CGS_OBJ_MATCH_MAX_OBJECTS;
constexpr int OR_SCAN_THREADS = 1024;
constexpr int OR_SCALE = 4096;
static_assert(OR_BINS == CGS_WAVE && CGS_OBJ_MAX_SIDE == CGS_WAVE, "one lane per bin, one lane per column");
static_assert((int64_t)CGS_OBJ_REID_MAX_FRAMES * CGS_OBJ_MAX_SIDE * CGS_OBJ_MAX_SIDE < (1ll << 31), "a track's pixel count is int32");
static_assert(1000 * OR_SCALE < (1ll << 31) && CGS_OBJ_REID_MAX_WINDOW < (1 << 20), "the threshold compare and L + W stay inside int32");

typedef short or_s2 __attribute__((ext_vector_type(2)));

__device__ __forceinline__ int or_wave_sum(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, CGS_WAVE);
    return v;
}

__device__ __forceinline__ int or_tracks(const int32_t* n_tracks, int max_tracks) { return min(max(*n_tracks, 0), max_tracks); }

__global__ void __launch_bounds__(OR_THREADS)
appearance_kernel(const uint8_t* __restrict__ frames, const int32_t* __restrict__ labels, const int32_t* __restrict__ track, int h, int w,
                  int K, int max_tracks, int32_t* __restrict__ S, int32_t* __restrict__ H) {
    __shared__ __attribute__((aligned(16))) int s_H[OR_MAX_K * OR_BINS];      // [label - 1][bin]
    const int x = threadIdx.x & (CGS_WAVE - 1), wave = threadIdx.x / CGS_WAVE;
    const bool live = x < w;
    const int64_t frame = (int64_t)blockIdx.x * h * w;
    const unsigned long long upto = (2ull << x) - 1ull;                 // bits 0..x

    for (int j = threadIdx.x; j < K * OR_BINS / 4; j += OR_THREADS) reinterpret_cast<int4*>(s_H)[j] = make_int4(0, 0, 0, 0);
    __syncthreads();

    int ln = 0;
    uint32_t cn = 0;
    if (live && wave < h) {
        ln = labels[frame + wave * w + x];
        cn = px_colour(frames, frame + wave * w + x);
    }
    for (int y = wave; y < h; y += OR_WAVES) {
        const int l = ln;
        const uint32_t c = cn;
        if (live && y + OR_WAVES < h) {
            ln = labels[frame + (y + OR_WAVES) * w + x];
            cn = px_colour(frames, frame + (y + OR_WAVES) * w + x);
        }
        const int lc = (l >= 1 && l <= K) ? l : 0;
        const int bin = (int)((((c & 255u) >> 6) << 4) | ((((c >> 8) & 255u) >> 6) << 2) | (((c >> 16) & 255u) >> 6));
        const int key = live ? (lc ? ((lc << 6) | bin) : 0) : -1;
        const int left = __shfl_up(key, 1, CGS_WAVE);
        const unsigned long long starts = __ballot(x == 0 || key != left);      // bit 0 is always set
        const bool last = x == CGS_WAVE - 1 || ((starts >> (x + 1)) & 1ull);
        if (live && last && key > 0) atomicAdd(&s_H[(lc - 1) * OR_BINS + bin], x - (63 - __clzll((long long)(starts & upto))) + 1);
    }
    __syncthreads();

    if (H) {
        int32_t* out = H + (int64_t)blockIdx.x * K * OR_BINS;
        for (int j = threadIdx.x; j < K * OR_BINS; j += OR_THREADS) out[j] = s_H[j];
    }
    if (track) {
        for (int l = wave; l < K; l += OR_WAVES) {                       // a wave is one label, a lane one bin: a 256-byte row of S
            const int t = track[(int64_t)blockIdx.x * K + l];
            const int v = s_H[l * OR_BINS + x];
            if (t >= 1 && t <= max_tracks && v) atomicAdd(&S[(int64_t)(t - 1) * OR_BINS + x], v);
        }
    }
}

__global__ void __launch_bounds__(OR_THREADS)
reid_signature_kernel(const int32_t* __restrict__ S, const int32_t* __restrict__ table, const int32_t* __restrict__ extra,
                      const int32_t* __restrict__ n_tracks, int n, int max_tracks, int min_area, int16_t* __restrict__ Q,
                      int32_t* __restrict__ F, int32_t* __restrict__ L, int32_t* __restrict__ D, int32_t* __restrict__ start,
                      int32_t* __restrict__ totals) {
    __shared__ int s_cnt;
    const int N = or_tracks(n_tracks, max_tracks);
    const int lane = threadIdx.x & (CGS_WAVE - 1), wave = threadIdx.x / CGS_WAVE;
    const int64_t i = (int64_t)blockIdx.x * OR_WAVES + wave;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    const int64_t step = (int64_t)gridDim.x * OR_THREADS;
    for (int64_t f = (int64_t)blockIdx.x * OR_THREADS + threadIdx.x; f <= n; f += step) {
        int lo = 0, hi = N;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (table[(int64_t)mid * CGS_OBJ_TRACK_FIELDS] >= f)
                hi = mid;
            else
                lo = mid + 1;
        }
        start[f] = lo;
    }
    if (i < max_tracks) {
        const bool in = i < N;
        const int s = in ? S[i * OR_BINS + lane] : 0;
        const int A = or_wave_sum(s);
        const bool elig = in && A >= min_area;                           // uniform over the wave
        int q = 0;
        if (elig) q = A < (1 << 20) ? (int)((uint32_t)s * (uint32_t)OR_SCALE / (uint32_t)A) : (int)((int64_t)s * OR_SCALE / A);
        Q[i * OR_BINS + lane] = (int16_t)q;
        const int d = or_wave_sum(q);
        if (lane == 0) {
            const int32_t* row = table + i * CGS_OBJ_TRACK_FIELDS;
            const int first = in ? row[0] : 0;
            int64_t end = in ? (int64_t)first + row[2] + (extra ? extra[2 * i + 1] : 0) - 1 : 0;
            end = end < -(1ll << 30) ? -(1ll << 30) : end > (1ll << 30) ? (1ll << 30) : end;
            F[i] = first;
            L[i] = (int)end;
            D[i] = elig ? d : 0;
            if (elig) atomicAdd(&s_cnt, 1);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(totals + 2, s_cnt);
}

__device__ __forceinline__ or_s2 or_pair(int v) {
    return __builtin_bit_cast(or_s2, v);
}

// the sum of the minima of the 8 signature values in a and in b, added to acc half by half
__device__ __forceinline__ or_s2 or_min_add(or_s2 acc, const int4& a, const int4& b) {
    acc += __builtin_elementwise_min(or_pair(a.x), or_pair(b.x));
    acc += __builtin_elementwise_min(or_pair(a.y), or_pair(b.y));
    acc += __builtin_elementwise_min(or_pair(a.z), or_pair(b.z));
    acc += __builtin_elementwise_min(or_pair(a.w), or_pair(b.w));
    return acc;
}

__global__ void __launch_bounds__(OR_THREADS)
reid_pair_kernel(const int16_t* __restrict__ Q, const int32_t* __restrict__ F, const int32_t* __restrict__ L, const int32_t* __restrict__ D,
                 const int32_t* __restrict__ start, const int32_t* __restrict__ n_tracks, int n, int max_tracks, int milli, int W,
                 int32_t* __restrict__ succ, unsigned long long* __restrict__ pred) {
    __shared__ __attribute__((aligned(16))) int16_t s_q[OR_WAVES][OR_BINS];
    const int N = or_tracks(n_tracks, max_tracks);
    const int lane = threadIdx.x & (CGS_WAVE - 1), wave = threadIdx.x / CGS_WAVE;
    const int64_t t = (int64_t)blockIdx.x * OR_WAVES + wave;             // the track's index, number t + 1
    const int Dt = t < N ? D[t] : 0;
    const bool active = Dt > 0;                                          // uniform over the wave
    if (active) s_q[wave][lane] = Q[t * OR_BINS + lane];
    __syncthreads();
    if (!active) return;                                                 // (succ was zeroed by the entry)
    const int Lt = L[t];
    int lo = start[min(max(Lt + 1, 0), n)];
    const int hi = start[min(max(Lt + W + 1, 0), n)];
    lo = max(lo, (int)t + 1);                                            // a link runs forward in the numbers whatever the table holds
    int4 qt[OR_BINS / 8];
#pragma unroll
    for (int k = 0; k < OR_BINS / 8; ++k) qt[k] = reinterpret_cast<const int4*>(s_q[wave])[k];
    unsigned long long best = 0ull;
    for (int u = lo + lane; u < hi; u += CGS_WAVE) {
        const int Du = D[u], Fu = F[u];
        if (Du > 0 && Fu > Lt && Fu <= Lt + W) {
            const int4* row = reinterpret_cast<const int4*>(Q + (int64_t)u * OR_BINS);
            int4 qu[OR_BINS / 8];
#pragma unroll
            for (int k = 0; k < OR_BINS / 8; ++k) qu[k] = row[k];
            or_s2 acc = or_pair(0);
#pragma unroll
            for (int k = 0; k < OR_BINS / 8; ++k) acc = or_min_add(acc, qt[k], qu[k]);
            const int s = (int)acc.x + (int)acc.y;
            if (1000 * s >= milli * min(Dt, Du)) {
                const unsigned long long hi32 = (unsigned long long)(uint32_t)s << 32;
                best = max(best, hi32 | (unsigned long long)(0xFFFFFFFFu - (uint32_t)(u + 1)));
                atomicMax(&pred[u], hi32 | (unsigned long long)(0xFFFFFFFFu - (uint32_t)(t + 1)));
            }
        }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) best = max(best, (unsigned long long)__shfl_xor((long long)best, m, CGS_WAVE));
    if (lane == 0) succ[t] = best ? (int)(0xFFFFFFFFu - (uint32_t)best) : 0;
}

__global__ void __launch_bounds__(OR_THREADS)
reid_link_kernel(const int32_t* __restrict__ succ, const unsigned long long* __restrict__ pred, const int32_t* __restrict__ n_tracks,
                 int max_tracks, int32_t* __restrict__ reid_prev, int32_t* __restrict__ reid_next, int32_t* __restrict__ reid_sim,
                 int32_t* __restrict__ identity, int32_t* __restrict__ root, int32_t* __restrict__ depth, int32_t* __restrict__ totals) {
    __shared__ int s_cnt;
    const int N = or_tracks(n_tracks, max_tracks);
    const int64_t i = (int64_t)blockIdx.x * OR_THREADS + threadIdx.x;
    if (threadIdx.x == 0) s_cnt = 0;
    __syncthreads();
    bool linked = false;
    if (i < max_tracks) {
        int p = 0, q = 0, s = 0;
        if (i < N) {
            const int u = succ[i];                                       // 0, or a number in i + 2 .. N
            if (u > 0 && u <= N && pred[u - 1] && (int64_t)(0xFFFFFFFFu - (uint32_t)pred[u - 1]) == i + 1) q = u;
            const unsigned long long key = pred[i];
            const int64_t t = key ? (int64_t)(0xFFFFFFFFu - (uint32_t)key) : 0;      // 0, or a number in 1 .. i
            if (t >= 1 && t <= i && succ[t - 1] == i + 1) {
                p = (int)t;
                s = (int)(key >> 32);
            }
        }
        linked = p > 0;
        reid_prev[i] = p;
        reid_next[i] = q;
        reid_sim[i] = s;
        identity[i] = 0;
        root[i] = linked ? p - 1 : (int)i;
        depth[i] = linked ? 1 : 0;
    }
    const unsigned long long links = __ballot(linked);
    if ((threadIdx.x & (CGS_WAVE - 1)) == 0 && links) atomicAdd(&s_cnt, __popcll(links));
    __syncthreads();
    if (threadIdx.x == 0 && s_cnt) atomicAdd(totals + 1, s_cnt);
}

__global__ void __launch_bounds__(OR_THREADS)
reid_resolve_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ depth, int32_t* __restrict__ root_out,
                    int32_t* __restrict__ depth_out, int max_tracks) {
    const int64_t i = (int64_t)blockIdx.x * OR_THREADS + threadIdx.x;
    if (i >= max_tracks) return;
    const int r = root[i];
    root_out[i] = root[r];
    depth_out[i] = depth[i] + depth[r];
}

// exclusive scan of "has no link backwards" over the tracks, one workgroup (track_number_kernel's shape): rank[i] is the number of the
// identity that track i heads
__global__ void __launch_bounds__(OR_SCAN_THREADS)
reid_number_kernel(const int32_t* __restrict__ reid_prev, const int32_t* __restrict__ n_tracks, int max_tracks, int32_t* __restrict__ rank,
                   int32_t* __restrict__ totals) {
    __shared__ int s_sum[OR_SCAN_THREADS];
    const int N = or_tracks(n_tracks, max_tracks);
    const int t = threadIdx.x, chunk = (N + OR_SCAN_THREADS - 1) / OR_SCAN_THREADS;
    const int lo = (int)min((int64_t)t * chunk, (int64_t)N), hi = (int)min((int64_t)lo + chunk, (int64_t)N);
    int sum = 0;
    for (int i = lo; i < hi; ++i) sum += reid_prev[i] == 0;
    s_sum[t] = sum;
    __syncthreads();
    for (int d = 1; d < OR_SCAN_THREADS; d <<= 1) {
        const int add = t >= d ? s_sum[t - d] : 0;
        __syncthreads();
        s_sum[t] += add;
        __syncthreads();
    }
    int run = s_sum[t] - sum;
    for (int i = lo; i < hi; ++i) {
        run += reid_prev[i] == 0;
        rank[i] = run;
    }
    if (t == OR_SCAN_THREADS - 1) totals[0] = s_sum[t];
}

__global__ void __launch_bounds__(OR_THREADS)
reid_finish_kernel(const int32_t* __restrict__ root, const int32_t* __restrict__ depth, const int32_t* __restrict__ rank,
                   const int32_t* __restrict__ n_tracks, int max_tracks, int32_t* __restrict__ identity, int32_t* __restrict__ totals) {
    __shared__ int s_len[OR_WAVES];
    const int N = or_tracks(n_tracks, max_tracks);
    const int64_t i = (int64_t)blockIdx.x * OR_THREADS + threadIdx.x;
    int len = 0;
    if (i < N) {
        identity[i] = rank[root[i]];
        len = depth[i] + 1;
    }
    len = px_wave_max(len);
    if ((threadIdx.x & (CGS_WAVE - 1)) == 0) s_len[threadIdx.x / CGS_WAVE] = len;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int longest = max(max(s_len[0], s_len[1]), max(s_len[2], s_len[3]));
        if (longest > 0) atomicMax(totals + 3, longest);
    }
}

// scratch, in 32-bit words; the 64-bit keys come first
struct ReidLayout {
    int64_t pred, succ, F, L, D, root_a, root_b, depth_a, depth_b, rank, start, words;
};
inline ReidLayout reid_layout(int64_t n, int64_t M) {
    ReidLayout o;
    o.pred = 0;
    o.succ = 2 * M;
    o.F = o.succ + M;
    o.L = o.F + M;
    o.D = o.L + M;
    o.root_a = o.D + M;
    o.root_b = o.root_a + M;
    o.depth_a = o.root_b + M;
    o.depth_b = o.depth_a + M;
    o.rank = o.depth_b + M;
    o.start = o.rank + M;
    o.words = (o.start + n + 1 + 1) & ~(int64_t)1;
    return o;
}

inline unsigned blocks_for(int64_t items, int per) { return (unsigned)((items + per - 1) / per); }

}  // namespace

extern "C" int cgs_objects_appearance(const uint8_t* frames, const int32_t* labels, const int32_t* track, int32_t n, int32_t h, int32_t w,
                                      int32_t max_objects, int32_t max_tracks, int32_t* track_hist, int32_t* object_hist,
                                      cgs_stream_t stream_) {
    if (!frames || !labels || (!track) != (!track_hist) || (!track_hist && !object_hist) || n < 1 || h < 1 || w < 1 || max_objects < 1 ||
        (track && max_tracks < 1) || ((uintptr_t)labels & 3u) || ((uintptr_t)track & 3u) || ((uintptr_t)track_hist & 3u) ||
        ((uintptr_t)object_hist & 3u))
        return CGS_ERR_BADARG;
    if (h > CGS_OBJ_MAX_SIDE || w > CGS_OBJ_MAX_SIDE || max_objects > OR_MAX_K || n > CGS_OBJ_REID_MAX_FRAMES) return CGS_ERR_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    if (track_hist) {
        const hipError_t e = hipMemsetAsync(track_hist, 0, sizeof(int32_t) * OR_BINS * (size_t)max_tracks, stream);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(appearance_kernel, dim3((unsigned)n), dim3(OR_THREADS), 0, stream, frames, labels, track, (int)h, (int)w,
                       (int)max_objects, (int)max_tracks, track_hist, object_hist);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}

extern "C" int64_t cgs_objects_reid_scratch_bytes(int32_t n, int32_t max_tracks) {
    if (n < 1 || max_tracks < 1) return 0;
    return reid_layout(n, max_tracks).words * 4;                         // 11 max_tracks + n + 1 words: far inside int64
}

extern "C" int cgs_objects_reid(const int32_t* track_hist, const int32_t* tracks, const int32_t* tracks_extra, const int32_t* n_tracks,
                                int32_t n, int32_t max_tracks, int32_t sim_milli, int32_t window, int32_t min_area, int32_t* reid_prev,
                                int32_t* reid_next, int32_t* reid_sim, int32_t* identity, int32_t* totals, int16_t* signature, void* scratch,
                                int64_t scratch_bytes, cgs_stream_t stream_) {
    if (!track_hist || !tracks || !n_tracks || !reid_prev || !reid_next || !reid_sim || !identity || !totals || !signature || !scratch ||
        n < 1 || max_tracks < 1 || sim_milli < 1 || sim_milli > 1000 || window < 1 || window > CGS_OBJ_REID_MAX_WINDOW || min_area < 1 ||
        ((uintptr_t)track_hist & 3u) || ((uintptr_t)tracks & 3u) || ((uintptr_t)tracks_extra & 3u) || ((uintptr_t)n_tracks & 3u) ||
        ((uintptr_t)reid_prev & 3u) || ((uintptr_t)reid_next & 3u) || ((uintptr_t)reid_sim & 3u) || ((uintptr_t)identity & 3u) ||
        ((uintptr_t)totals & 3u) || ((uintptr_t)signature & 15u) || ((uintptr_t)scratch & 7u) ||
        scratch_bytes < cgs_objects_reid_scratch_bytes(n, max_tracks))
        return CGS_ERR_BADARG;
    if (n > CGS_OBJ_REID_MAX_FRAMES) return CGS_ERR_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    const int64_t M = max_tracks;
    const ReidLayout o = reid_layout(n, M);
    int32_t* s = static_cast<int32_t*>(scratch);
    unsigned long long* pred = reinterpret_cast<unsigned long long*>(s + o.pred);
    int32_t *succ = s + o.succ, *F = s + o.F, *L = s + o.L, *D = s + o.D, *root_a = s + o.root_a, *root_b = s + o.root_b,
            *depth_a = s + o.depth_a, *depth_b = s + o.depth_b, *rank = s + o.rank, *start = s + o.start;
    hipError_t e = hipMemsetAsync(totals, 0, 4 * sizeof(int32_t), stream);
    if (e != hipSuccess) return (int)e;
    e = hipMemsetAsync(scratch, 0, sizeof(int32_t) * 3 * (size_t)M, stream);      // pred and succ
    if (e != hipSuccess) return (int)e;
    const unsigned waves4 = blocks_for(M, OR_WAVES), lanes = blocks_for(M, OR_THREADS);
    hipLaunchKernelGGL(reid_signature_kernel, dim3(waves4), dim3(OR_THREADS), 0, stream, track_hist, tracks, tracks_extra, n_tracks, (int)n,
                       (int)max_tracks, (int)min_area, signature, F, L, D, start, totals);
    CGS_HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(reid_pair_kernel, dim3(waves4), dim3(OR_THREADS), 0, stream, signature, F, L, D, start, n_tracks, (int)n,
                       (int)max_tracks, (int)sim_milli, (int)window, succ, pred);
    CGS_HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(reid_link_kernel, dim3(lanes), dim3(OR_THREADS), 0, stream, succ, pred, n_tracks, (int)max_tracks, reid_prev,
                       reid_next, reid_sim, identity, root_a, depth_a, totals);
    CGS_HIP_CHECK_LAUNCH();
    const int64_t cap = n < M ? n : M;                                    // the most tracks one chain can hold
    for (int64_t reach = 1; reach < cap - 1; reach <<= 1) {
        hipLaunchKernelGGL(reid_resolve_kernel, dim3(lanes), dim3(OR_THREADS), 0, stream, root_a, depth_a, root_b, depth_b, (int)max_tracks);
        CGS_HIP_CHECK_LAUNCH();
        int32_t* swap = root_a;
        root_a = root_b;
        root_b = swap;
        swap = depth_a;
        depth_a = depth_b;
        depth_b = swap;
    }
    hipLaunchKernelGGL(reid_number_kernel, dim3(1), dim3(OR_SCAN_THREADS), 0, stream, reid_prev, n_tracks, (int)max_tracks, rank, totals);
    CGS_HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(reid_finish_kernel, dim3(lanes), dim3(OR_THREADS), 0, stream, root_a, depth_a, rank, n_tracks, (int)max_tracks,
                       identity, totals);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}
