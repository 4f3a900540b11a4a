// Evaluation scoring on the device: the intersection / union counts Handler.get_iou and the reference's CRF grid search take from
// numpy `&` / `|` over the whole stack (main.py:1253, 1267-1269), for a whole threshold grid (cgs_iou_curve) or for K label stacks
// (cgs_iou_counts) in one pass over the data.  Everything is integer counting: any order of accumulation gives the same numbers.
//
// cgs_iou_curve.  For ascending thresholds a pixel is on exactly for the thresholds below its value, so a pixel contributes ONE bin
// index k = #{t : thr[t] < v} (<= when inclusive; a NaN compares false everywhere: k = 0, on for nothing) to one of two (T+1)-bin
// histograms, hT (truth set) and hF (truth clear), and
//     inter[t] = sum_{k > t} hT[k],   union[t] = #truth + sum_{k > t} hF[k],   #truth = sum_k hT[k].
// curve_hist makes the histograms, curve_finish the suffix sums.
//   - the thresholds sit in LDS; k comes from a branch-free binary search (at most 11 LDS reads per pixel);
//   - real masks are bimodal: almost every pixel lands in bin 0 or bin T.  Those two bins never touch LDS: every lane counts its own
//     hits in four registers (bin 0 / bin T x truth clear / set), reduced over the wave once at the end;
//   - the bins in between go to a per-wave sub-histogram in LDS (32-bit); when all such lanes of a wave-instruction share one bin
//     (a constant stack) one lane adds the population count instead of 64 serialised adds to one address;
//   - a workgroup adds its non-zero bins to the 64-bit global histograms with vector atomics (integer: order-free).
//
// cgs_iou_counts.  `groups` workgroups per stack; 16 bytes of labels and of truth per lane per step, the bytes' "non-zero" reduced to one bit
// per byte inside each 32-bit word and counted with popcount; per-lane 32-bit counts, one 64-bit atomic pair per workgroup.
//
// Loads are 16 bytes wide wherever 16 pixels (4 for the fp32 values) are left, at whatever alignment the caller's pointers have (the
// vector types below are declared with the alignment of their elements); the remaining pixels are read one by one.
#include <algorithm>

#include "cgs_common.h"

namespace {

constexpr int MET_THREADS = 256;
constexpr int MET_WAVES = MET_THREADS / CGS_WAVE;
constexpr int MET_MAX_T = 1024;
constexpr int MET_MAX_GROUPS = 1024;                  // 4 workgroups per CU: the grid-stride loops start with every CU busy
constexpr int64_t MET_GROUP_PIXELS = 1ll << 31;       // a workgroup's 32-bit counters see fewer pixels than this

typedef float f32x4_u __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32x4_u __attribute__((ext_vector_type(4), aligned(1)));
typedef uint32_t u32_u __attribute__((aligned(1)));

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += (uint32_t)__shfl_xor((int)v, m, 64);
    return v;
}

// bit 7 of every byte of x that is not zero
__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t x) {
    return (((x & 0x7F7F7F7Fu) + 0x7F7F7F7Fu) | x) & 0x80808080u;
}

struct CurveCtx {
    const float* thr;        // LDS, T ascending thresholds
    uint32_t* hist;          // LDS, this wave's sub-histogram: [2][T + 1], truth clear first
    int T, top;              // top = the largest power of two <= T
    uint32_t edge[4];        // bin 0 / bin T of truth clear, bin 0 / bin T of truth set (this lane's own pixels)
};

template <bool INCLUSIVE>
__device__ __forceinline__ void curve_pixel(CurveCtx& c, float v, bool set, bool live) {
    int k = 0;
    for (int step = c.top; step; step >>= 1) {
        const int j = k + step;
        if (j <= c.T) {
            const float t = c.thr[j - 1];
            if (INCLUSIVE ? (t <= v) : (t < v)) k = j;
        }
    }
    const bool lo = live && k == 0, hi = live && k == c.T;           // T >= 1: never both
    c.edge[0] += (lo && !set);
    c.edge[1] += (hi && !set);
    c.edge[2] += (lo && set);
    c.edge[3] += (hi && set);
    const bool mid = live && !lo && !hi;
    const unsigned long long m = __ballot(mid);
    if (m) {                                                     // wave-uniform
        const int key = k + (set ? c.T + 1 : 0);
        const int first = __ffsll((long long)m) - 1;
        const int key0 = __shfl(key, first, 64);
        if (__ballot(mid && key == key0) == m) {
            if ((int)(threadIdx.x & (CGS_WAVE - 1)) == first) atomicAdd(&c.hist[key0], (uint32_t)__popcll(m));
        } else if (mid) {
            atomicAdd(&c.hist[key], 1u);
        }
    }
}

template <bool INCLUSIVE>
__global__ void __launch_bounds__(MET_THREADS)
curve_hist(const float* __restrict__ v, const uint8_t* __restrict__ truth, const float* __restrict__ thr, int T, int64_t px,
           unsigned long long* __restrict__ hist) {
    __shared__ float s_thr[MET_MAX_T];
    __shared__ uint32_t s_hist[MET_WAVES * 2 * (MET_MAX_T + 1)];
    __shared__ uint32_t s_edge[MET_WAVES][4];
    const int bins = 2 * (T + 1);
    for (int i = threadIdx.x; i < T; i += MET_THREADS) s_thr[i] = thr[i];
    for (int i = threadIdx.x; i < MET_WAVES * bins; i += MET_THREADS) s_hist[i] = 0u;
    __syncthreads();
    const int wave = threadIdx.x / CGS_WAVE, lane = threadIdx.x & (CGS_WAVE - 1);
    CurveCtx c;
    c.thr = s_thr;
    c.hist = s_hist + wave * bins;
    c.T = T;
    c.top = 1;
    while (2 * c.top <= T) c.top *= 2;
    c.edge[0] = c.edge[1] = c.edge[2] = c.edge[3] = 0u;

    // groups of 4 pixels: neighbouring lanes read neighbouring 16 B of v and 4 B of truth.  The trip count is the same for every lane of
    // the workgroup (curve_pixel holds wave-wide operations); lanes past the end run it with live = false.
    const int64_t quads = px >> 2;
    const int64_t stride = (int64_t)gridDim.x * MET_THREADS;
    for (int64_t base = (int64_t)blockIdx.x * MET_THREADS; base < quads; base += stride) {
        const int64_t q = base + threadIdx.x;
        const bool live = q < quads;
        f32x4_u f = {0.f, 0.f, 0.f, 0.f};
        uint32_t t4 = 0u;
        if (live) {
            f = *reinterpret_cast<const f32x4_u*>(v + 4 * q);
            t4 = *reinterpret_cast<const u32_u*>(truth + 4 * q);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) curve_pixel<INCLUSIVE>(c, f[e], ((t4 >> (8 * e)) & 0xFFu) != 0u, live);
    }
    if (blockIdx.x == 0) {                                       // the px % 4 pixels left over: wave 0 of workgroup 0
        const int64_t i = 4 * quads + threadIdx.x;
        if (threadIdx.x < CGS_WAVE) {
            const bool live = i < px;
            curve_pixel<INCLUSIVE>(c, live ? v[i] : 0.f, live && truth[i] != 0, live);
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const uint32_t s = wave_sum_u32(c.edge[e]);
        if (lane == 0) s_edge[wave][e] = s;
    }
    __syncthreads();
    for (int i = threadIdx.x; i < bins; i += MET_THREADS) {
        uint32_t s = 0u;
#pragma unroll
        for (int w = 0; w < MET_WAVES; ++w) s += s_hist[w * bins + i];
        const int half = i >= T + 1, k = i - half * (T + 1);
#pragma unroll
        for (int w = 0; w < MET_WAVES; ++w) {
            if (k == 0) s += s_edge[w][2 * half];
            if (k == T) s += s_edge[w][2 * half + 1];
        }
        if (s) atomicAdd(&hist[i], (unsigned long long)s);
    }
}

// counts[t] = (sum_{k > t} hT[k], #truth + sum_{k > t} hF[k]): an inclusive suffix sum over bins 1..T, one workgroup, thread t = bin t + 1
__global__ void __launch_bounds__(MET_MAX_T)
curve_finish(const unsigned long long* __restrict__ hist, int T, int64_t* __restrict__ counts) {
    __shared__ unsigned long long s_f[MET_MAX_T], s_t[MET_MAX_T];
    const int t = threadIdx.x;
    const unsigned long long* hF = hist;
    const unsigned long long* hT = hist + (T + 1);
    s_f[t] = t < T ? hF[t + 1] : 0ull;
    s_t[t] = t < T ? hT[t + 1] : 0ull;
    __syncthreads();
    for (int d = 1; d < T; d <<= 1) {
        const unsigned long long af = t + d < T ? s_f[t + d] : 0ull, at = t + d < T ? s_t[t + d] : 0ull;
        __syncthreads();
        s_f[t] += af;
        s_t[t] += at;
        __syncthreads();
    }
    if (t < T) {
        const unsigned long long n_truth = hT[0] + s_t[0];
        counts[2 * t] = (int64_t)s_t[t];
        counts[2 * t + 1] = (int64_t)(n_truth + s_f[t]);
    }
}

__global__ void __launch_bounds__(MET_THREADS)
iou_counts_kernel(const uint8_t* __restrict__ labels, const uint8_t* __restrict__ truth, int64_t px, int groups,
                  unsigned long long* __restrict__ counts) {
    __shared__ uint32_t s_part[MET_WAVES][2];
    const int stack = blockIdx.x / groups, group = blockIdx.x - stack * groups;
    const uint8_t* lab = labels + (int64_t)stack * px;
    uint32_t inter = 0u, uni = 0u;
    const int64_t chunks = px >> 4;
    const int64_t stride = (int64_t)groups * MET_THREADS;
    for (int64_t q = (int64_t)group * MET_THREADS + threadIdx.x; q < chunks; q += stride) {
        const u32x4_u a = *reinterpret_cast<const u32x4_u*>(lab + 16 * q);
        const u32x4_u b = *reinterpret_cast<const u32x4_u*>(truth + 16 * q);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const uint32_t na = nonzero_bytes(a[e]), nb = nonzero_bytes(b[e]);
            inter += (uint32_t)__popc(na & nb);
            uni += (uint32_t)__popc(na | nb);
        }
    }
    if (group == 0 && threadIdx.x < 16) {                        // the px % 16 pixels left over
        const int64_t i = 16 * chunks + threadIdx.x;
        if (i < px) {
            const bool a = lab[i] != 0, b = truth[i] != 0;
            inter += (a && b);
            uni += (a || b);
        }
    }
    inter = wave_sum_u32(inter);
    uni = wave_sum_u32(uni);
    const int wave = threadIdx.x / CGS_WAVE, lane = threadIdx.x & (CGS_WAVE - 1);
    if (lane == 0) {
        s_part[wave][0] = inter;
        s_part[wave][1] = uni;
    }
    __syncthreads();
    if (threadIdx.x < 2) {
        unsigned long long s = 0ull;
#pragma unroll
        for (int w = 0; w < MET_WAVES; ++w) s += s_part[w][threadIdx.x];
        if (s) atomicAdd(&counts[2 * stack + threadIdx.x], s);
    }
}

// workgroups for `work` lane-steps: every CU busy, and no workgroup's 32-bit counters within reach of 2^32 pixels
unsigned met_groups(int64_t work, int64_t px) {
    int64_t g = std::max<int64_t>(1, std::min<int64_t>((work + MET_THREADS - 1) / MET_THREADS, MET_MAX_GROUPS));
    g = std::max(g, (px + MET_GROUP_PIXELS - 1) / MET_GROUP_PIXELS);
    return (unsigned)g;
}

}  // namespace

extern "C" int cgs_iou_curve(const float* v, const uint8_t* truth, const float* thr, int32_t T, int32_t inclusive, int64_t px,
                             int64_t* counts, cgs_stream_t stream_) {
    if (!v || !truth || !thr || !counts || T < 1 || T > MET_MAX_T || px < 1 || (inclusive != 0 && inclusive != 1) ||
        ((uintptr_t)v & 3u) || ((uintptr_t)thr & 3u) || ((uintptr_t)counts & 7u))
        return CGS_ERR_BADARG;
    hipStream_t stream = (hipStream_t)stream_;
    const size_t bytes = 2 * (size_t)(T + 1) * sizeof(unsigned long long);
    unsigned long long* hist = nullptr;
    hipError_t e = hipMallocAsync((void**)&hist, bytes, stream);
    if (e != hipSuccess) return (int)e;
    int rc = CGS_OK;
    e = hipMemsetAsync(hist, 0, bytes, stream);
    if (e != hipSuccess) rc = (int)e;
    if (rc == CGS_OK) {
        const dim3 grid(met_groups(px >> 2, px));
        if (inclusive)
            hipLaunchKernelGGL(curve_hist<true>, grid, dim3(MET_THREADS), 0, stream, v, truth, thr, (int)T, px, hist);
        else
            hipLaunchKernelGGL(curve_hist<false>, grid, dim3(MET_THREADS), 0, stream, v, truth, thr, (int)T, px, hist);
        hipLaunchKernelGGL(curve_finish, dim3(1), dim3(MET_MAX_T), 0, stream, hist, (int)T, counts);
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) rc = (int)le;
    }
    e = hipFreeAsync(hist, stream);
    if (rc == CGS_OK && e != hipSuccess) rc = (int)e;
    return rc;
}

extern "C" int cgs_iou_counts(const uint8_t* labels, const uint8_t* truth, int32_t K, int64_t px, int64_t* counts, cgs_stream_t stream_) {
    if (!labels || !truth || !counts || K < 1 || px < 1 || ((uintptr_t)counts & 7u)) return CGS_ERR_BADARG;
    const unsigned groups = met_groups(px >> 4, px);
    if ((int64_t)groups * K > 0x7FFFFFFFll) return CGS_ERR_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    const hipError_t e = hipMemsetAsync(counts, 0, 2 * (size_t)K * sizeof(int64_t), stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(iou_counts_kernel, dim3(groups * (unsigned)K), dim3(MET_THREADS), 0, stream, labels, truth, px, (int)groups,
                       reinterpret_cast<unsigned long long*>(counts));
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}
