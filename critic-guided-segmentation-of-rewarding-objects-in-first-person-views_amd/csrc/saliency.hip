// The saliency baseline's post-processing on the device, for a whole grid of thresholds at once (Handler._saliency_post, main.py:976-1003):
// a pixel of frame f is on at threshold t when
//     min(double(sal) / (double(S) + DBL_MIN) * double(pred_f), 1.0) > t                       (float64, as numpy 2 evaluates the host form)
// with S the normaliser: a number per threshold (global mode, gscale[t] = float32(mean * t), built by the caller) or the frame's k[t]-th
// smallest value (per-frame mode, NaN sorted last as np.sort does).  The threshold is ALSO the normaliser, so every threshold is its own
// problem; what makes a grid cheap is that for pred > 0 the quotient and the product are correctly rounded and therefore monotone in sal:
// the on-set is an upper set of the frame's sorted order (below the NaNs, which are on for nothing).  So, one workgroup per frame:
//   1. the 4096 values become 32-bit words (key << 1 | truth) in LDS: a non-negative float's bit pattern orders as the float does, a NaN
//      gets one key above +inf, -0.0 (and anything negative, which the contract excludes) the key of 0;
//   2. a bitonic sort of the words in LDS, then a prefix count of the truth bits in sorted order (uint16, 4097 entries);
//   3. every thread takes thresholds t = tid, tid + 256, ...: a binary search over the sorted positions below the first NaN, each probe
//      evaluating the exact float64 predicate above on the probed value (plain C++ operators: IEEE division and multiplication, nothing
//      to contract), gives the first on position; the counts follow from the prefix table and go to counts[t] with 64-bit integer
//      atomics (any order of frames gives the same numbers).  For pred <= 0, pred NaN or t >= 1 nothing is on and nothing is searched;
//   4. the hard mask of ONE threshold (`which`) is the same predicate evaluated on every pixel directly, four pixels per 32-bit store.
// Thresholds <= 0 (or k outside 0..4095, clamped here) are outside the contract: they give unspecified counts, no fault.
#include "cgs_common.h"

namespace {

constexpr int SAL_THREADS = 256;
constexpr int SAL_WAVES = SAL_THREADS / CGS_WAVE;
constexpr int SAL_SIDE = 64;
constexpr int SAL_PX = SAL_SIDE * SAL_SIDE;
constexpr int SAL_PER = SAL_PX / SAL_THREADS;          // sorted positions per thread in the prefix count
constexpr int SAL_MAX_T = 1024;
constexpr uint32_t SAL_NAN_KEY = 0x7FC00000u;          // above +inf (0x7F800000); as a float it is the quiet NaN
constexpr double SAL_TINY = 2.2250738585072014e-308;   // DBL_MIN = np.finfo(np.float64).tiny

typedef float f32x4_u __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t u32_u __attribute__((aligned(1)));

__device__ __forceinline__ uint32_t sal_key(float v) {
    if (v != v) return SAL_NAN_KEY;
    return v > 0.f ? __float_as_uint(v) : 0u;
}

// the exact predicate; false for a NaN anywhere (min(NaN, 1) is NaN in numpy, and NaN > t is false).  The caller has checked t < 1.
__device__ __forceinline__ bool sal_on(float v, double denom, double p, double t) {
    return (double)v / denom * p > t;
}

__global__ void __launch_bounds__(SAL_THREADS)
saliency_sweep_kernel(const float* __restrict__ sal, const float* __restrict__ preds, const uint8_t* __restrict__ truth,
                      const double* __restrict__ thr, const float* __restrict__ gscale, const int32_t* __restrict__ kth, int T, int which,
                      unsigned long long* __restrict__ counts, float* __restrict__ scale, uint8_t* __restrict__ hard) {
    __shared__ uint32_t s_word[SAL_PX];                // key << 1 | truth
    __shared__ uint16_t s_pre[SAL_PX + 1];             // s_pre[i] = truth pixels among the sorted positions below i
    __shared__ uint32_t s_wave[SAL_WAVES];
    const int tid = threadIdx.x, lane = tid & (CGS_WAVE - 1), wave = tid / CGS_WAVE;
    const int64_t frame = blockIdx.x;
    const float* v = sal + frame * SAL_PX;
    const uint8_t* y = truth ? truth + frame * SAL_PX : nullptr;

#pragma unroll
    for (int r = 0; r < SAL_PX / (4 * SAL_THREADS); ++r) {
        const int q = r * SAL_THREADS + tid;
        const f32x4_u f = *reinterpret_cast<const f32x4_u*>(v + 4 * q);
        const uint32_t t4 = y ? *reinterpret_cast<const u32_u*>(y + 4 * q) : 0u;
#pragma unroll
        for (int e = 0; e < 4; ++e) s_word[4 * q + e] = (sal_key(f[e]) << 1) | (((t4 >> (8 * e)) & 0xFFu) != 0u ? 1u : 0u);
    }
    __syncthreads();

    // bitonic sort, ascending: SAL_PX / 2 compare-exchanges per step, every pair touched by one thread only
    for (int k = 2; k <= SAL_PX; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
#pragma unroll
            for (int e = 0; e < SAL_PX / (2 * SAL_THREADS); ++e) {
                const int t = e * SAL_THREADS + tid;
                const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
                const uint32_t a = s_word[lo], b = s_word[hi];
                if ((a > b) == ((lo & k) == 0)) {
                    s_word[lo] = b;
                    s_word[hi] = a;
                }
            }
            __syncthreads();
        }
    }

    // prefix count of the truth bits: 16 consecutive positions per thread, a wave scan, the waves' totals through LDS
    uint32_t own = 0u;
#pragma unroll
    for (int e = 0; e < SAL_PER; ++e) own += s_word[SAL_PER * tid + e] & 1u;
    uint32_t incl = own;
#pragma unroll
    for (int d = 1; d < CGS_WAVE; d <<= 1) {
        const uint32_t up = (uint32_t)__shfl_up((int)incl, d, CGS_WAVE);
        if (lane >= d) incl += up;
    }
    if (lane == CGS_WAVE - 1) s_wave[wave] = incl;
    __syncthreads();
    uint32_t run = incl - own;
    for (int w2 = 0; w2 < wave; ++w2) run += s_wave[w2];
#pragma unroll
    for (int e = 0; e < SAL_PER; ++e) {
        s_pre[SAL_PER * tid + e] = (uint16_t)run;
        run += s_word[SAL_PER * tid + e] & 1u;
    }
    if (tid == SAL_THREADS - 1) s_pre[SAL_PX] = (uint16_t)run;
    __syncthreads();

    // the first NaN position (SAL_PX when there is none): every thread walks the same 12 probes
    int nn;
    {
        int lo = 0, hi = SAL_PX;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if ((s_word[mid] >> 1) >= SAL_NAN_KEY) hi = mid; else lo = mid + 1;
        }
        nn = lo;
    }
    const double p = (double)preds[frame];
    const bool p_ok = p > 0.0;                          // false for a NaN
    const uint32_t n_truth = s_pre[SAL_PX], truth_live = s_pre[nn];

    for (int t = tid; t < T; t += SAL_THREADS) {
        float S;
        if (gscale) {
            S = gscale[t];
        } else {
            const int kk = min(max(kth[t], 0), SAL_PX - 1);
            S = __uint_as_float(s_word[kk] >> 1);
        }
        scale[frame * T + t] = S;
        if (!y) continue;
        const double tt = thr[t];
        int pos = nn;
        if (p_ok && tt < 1.0) {
            const double denom = (double)S + SAL_TINY;
            int lo = 0, hi = nn;
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (sal_on(__uint_as_float(s_word[mid] >> 1), denom, p, tt)) hi = mid; else lo = mid + 1;
            }
            pos = lo;
        }
        const uint32_t inter = truth_live - s_pre[pos];
        const uint32_t uni = n_truth + (uint32_t)(nn - pos) - inter;
        if (inter) atomicAdd(&counts[2 * t], (unsigned long long)inter);
        if (uni) atomicAdd(&counts[2 * t + 1], (unsigned long long)uni);
    }

    if (which >= 0) {                                   // wave-uniform: a kernel argument
        const double tw = thr[which];
        float S;
        if (gscale) {
            S = gscale[which];
        } else {
            const int kk = min(max(kth[which], 0), SAL_PX - 1);
            S = __uint_as_float(s_word[kk] >> 1);
        }
        const double denom = (double)S + SAL_TINY;
        const bool live = p_ok && tw < 1.0;
        uint8_t* out = hard + frame * SAL_PX;
#pragma unroll
        for (int r = 0; r < SAL_PX / (4 * SAL_THREADS); ++r) {
            const int q = r * SAL_THREADS + tid;
            const f32x4_u f = *reinterpret_cast<const f32x4_u*>(v + 4 * q);
            uint32_t packed = 0u;
#pragma unroll
            for (int e = 0; e < 4; ++e) packed |= (live && sal_on(f[e], denom, p, tw) ? 1u : 0u) << (8 * e);
            *reinterpret_cast<uint32_t*>(out + 4 * q) = packed;
        }
    }
}

}  // namespace

extern "C" int cgs_saliency_sweep(const float* sal, const float* preds, const uint8_t* truth, const double* thr, const float* gscale,
                                  const int32_t* k, int32_t T, int32_t n, int32_t h, int32_t w, int32_t which, int64_t* counts,
                                  float* scale, uint8_t* hard, cgs_stream_t stream_) {
    if (T < 1 || T > SAL_MAX_T || n < 1 || h < 1 || w < 1 || which < -1 || which >= T) return CGS_ERR_BADARG;
    if (h != SAL_SIDE || w != SAL_SIDE) return CGS_ERR_UNSUPPORTED;
    if (!sal || !preds || !thr || !scale || (!gscale && !k) || (truth && !counts) || (which >= 0 && !hard) || ((uintptr_t)sal & 3u) ||
        ((uintptr_t)preds & 3u) || ((uintptr_t)thr & 7u) || ((uintptr_t)gscale & 3u) || ((uintptr_t)k & 3u) || ((uintptr_t)counts & 7u) ||
        ((uintptr_t)scale & 3u) || ((uintptr_t)hard & 3u))
        return CGS_ERR_BADARG;
    hipStream_t stream = (hipStream_t)stream_;
    if (truth) {
        const hipError_t e = hipMemsetAsync(counts, 0, 2 * (size_t)T * sizeof(int64_t), stream);
        if (e != hipSuccess) return (int)e;
    }
    hipLaunchKernelGGL(saliency_sweep_kernel, dim3((unsigned)n), dim3(SAL_THREADS), 0, stream, sal, preds, truth, thr, gscale, k, (int)T,
                       (int)which, reinterpret_cast<unsigned long long*>(counts), scale, hard);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}
