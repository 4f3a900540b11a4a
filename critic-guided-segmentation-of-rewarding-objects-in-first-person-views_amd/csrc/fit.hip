// Frames of any size for -process -fit (include/cgs_hip.h): the way in, cgs_fit_down_u8, shrinks uint8 frames of 64..4096 pixels a side
// to the network's 64 x 64 grid with the exact box average; the way out, cgs_fit_up_joint, brings a 64 x 64 map back to the frame's size
// by joint bilateral upsampling (Kopf et al. 2007) guided by the frame, so that the outline follows the frame's edges.
//
// cgs_fit_down_u8.  On an axis of length L source pixel s covers [64 s, 64 s + 64) and output cell o covers [L o, L o + L); w_L(o, s) is
// the length of the overlap.  One workgroup takes one output row of one frame:
//   1. rows     the source rows that overlap the cell row, (H oy) / 64 .. (H oy + H - 1) / 64, are read once each (a row shared by two
//               cell rows is read by both workgroups).  A thread owns the same bytes of every row -- chunk t, t + 256, ... of VEC bytes,
//               VEC = 16, 4 or 1, the widest load for which the frames' base and the row length 3 W are both aligned -- and keeps
//               col[b] = sum_y w_H(oy, y) v[y][b] in registers: 48 accumulators cover the longest row, 3 x 4096 bytes.
//   2. columns  the column sums go to LDS (3 W words) and thread (ox, c) adds up its cell, S = sum_x w_W(ox, x) col[x][c].
//   3. round    (2 S + H W) / (2 H W), half up.
// Widths: col <= 255 x 4096 < 2^20 and S <= 255 x 4096^2 = 2^32 - 2^24, so both fit an unsigned 32-bit word exactly; 2 S + H W is below
// 2^34 and is formed and divided in 64 bits.  Nothing is rounded before the one division, so the result is the exact box average.
// Traffic: every frame byte once (plus the shared boundary rows), 192 bytes out per workgroup: bound by the read of the frames.
//
// cgs_fit_up_joint.  A band is the rows of the frame whose home cell row is qy0; a workgroup takes 256 columns of one band.  The five
// cell rows qy0 - 2 .. qy0 + 2 of `low` (packed, with the squared length of the colour) and of the map are staged in LDS, 2.5 KiB; a
// thread is one column x, whose 5 x 5 taps are the same cells for every row of the band, so it moves them to registers once.  Per pixel:
//   pass 1   d2[tap] = |g|^2 + |l|^2 - 2 g.l, integers (the byte dot product is one instruction), and their minimum.  A tap outside
//            the grid carries |l|^2 = 2^30, so it never is the minimum.
//   pass 2   w = exp2(-((d2 - d2_min) cr + ey[dy] + ex[dx])) with cr = log2(e) / (2 sigma_r^2) and ey, ex = f^2 log2(e) / (2 sigma_s^2):
//            one hardware exponential per tap; the integer difference is taken before anything is rounded.  A tap outside the grid has
//            ex or ey = +inf, so its weight is exp2(-inf) = +0 exactly and it adds nothing: skipped, not clamped.
//            num = fma(w, m, num), den = den + w in the same tap order (dy outer, dx inner): 0 <= m <= 1 keeps num <= den at every
//            step, so 0 <= soft <= 1, and a map that is 1 wherever a weight is non-zero gives num == den and soft == 1.0f exactly.
// The tap of d2_min has the weight exp2(-(ey + ex)) >= exp(-6.25 / sigma_s^2), so den > 0 for sigma_s >= 0.5, which the entry enforces.
// No atomics; soft = num / den is the IEEE division.  About 12 VALU operations and one exponential per tap against 3 bytes read and 4 to
// 6 written per pixel: bound by instruction issue, not by HBM.
#include "pixel_common.h"

namespace {

constexpr int FIT_THREADS = 256;
constexpr int FIT_SIDE = CGS_FIT_SIDE;                // the network's grid
constexpr int FIT_ACC = 48;                           // bytes of a row per thread: 3 x CGS_FIT_MAX_SIDE / FIT_THREADS
constexpr int FIT_R = CGS_FIT_RADIUS, FIT_TAPS = 2 * FIT_R + 1;
constexpr uint32_t FIT_FAR = 1u << 30;                // |l|^2 of a tap outside the grid: above every real d2 (<= 195075) by far
static_assert(FIT_ACC * FIT_THREADS == 3 * CGS_FIT_MAX_SIDE && FIT_SIDE == 64 && 3 * FIT_SIDE <= FIT_THREADS, "fit_down layout");

template <int VEC> struct fit_word;
template <> struct fit_word<16> { typedef uint4 type; };
template <> struct fit_word<4> { typedef uint32_t type; };
template <> struct fit_word<1> { typedef uint8_t type; };

template <int VEC, int J>
__device__ __forceinline__ uint32_t fit_byte(const typename fit_word<VEC>::type& v) {
    if constexpr (VEC == 16) {
        const uint32_t word = J < 4 ? v.x : J < 8 ? v.y : J < 12 ? v.z : v.w;
        return (word >> (8 * (J & 3))) & 255u;
    } else if constexpr (VEC == 4) {
        return (v >> (8 * J)) & 255u;
    } else {
        return v;
    }
}

template <int VEC, int J>
__device__ __forceinline__ void fit_add(uint32_t* acc, const typename fit_word<VEC>::type& v, uint32_t wy) {
    acc[J] += wy * fit_byte<VEC, J>(v);
    if constexpr (J + 1 < VEC) fit_add<VEC, J + 1>(acc, v, wy);
}

template <int VEC>
__global__ void __launch_bounds__(FIT_THREADS)
fit_down_kernel(const uint8_t* __restrict__ frames, int H, int W, uint8_t* __restrict__ out) {
    extern __shared__ __attribute__((aligned(16))) uint32_t s_col[];       // [3 W] column sums of this cell row
    typedef typename fit_word<VEC>::type word_t;
    constexpr int CHUNKS = FIT_ACC / VEC;
    const int oy = blockIdx.x & (FIT_SIDE - 1), f = blockIdx.x / FIT_SIDE, t = threadIdx.x;
    const int row_bytes = 3 * W, nchunks = row_bytes / VEC;                // VEC divides 3 W (the entry chose it so)
    const uint8_t* frame = frames + (int64_t)f * H * row_bytes;
    const int lo = H * oy, hi = lo + H, y0 = lo / 64, y1 = (hi - 1) / 64;

    uint32_t acc[FIT_ACC];
#pragma unroll
    for (int i = 0; i < FIT_ACC; ++i) acc[i] = 0u;
    for (int y = y0; y <= y1; ++y) {
        const uint32_t wy = (uint32_t)(min(64 * y + 64, hi) - max(64 * y, lo));
        const word_t* row = reinterpret_cast<const word_t*>(frame + (int64_t)y * row_bytes);
#pragma unroll
        for (int k = 0; k < CHUNKS; ++k) {
            const int c = t + k * FIT_THREADS;
            if (c < nchunks) {
                const word_t v = row[c];
                fit_add<VEC, 0>(acc + k * VEC, v, wy);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < CHUNKS; ++k) {
        const int c = t + k * FIT_THREADS;
        if (c < nchunks) {
#pragma unroll
            for (int j = 0; j < VEC; ++j) s_col[c * VEC + j] = acc[k * VEC + j];
        }
    }
    __syncthreads();

    if (t < 3 * FIT_SIDE) {
        const int ox = t / 3, c = t - 3 * ox;
        const int xlo = W * ox, xhi = xlo + W, x0 = xlo / 64, x1 = (xhi - 1) / 64;
        uint32_t S = 0u;                                                   // <= 255 H W < 2^32
        for (int x = x0; x <= x1; ++x) S += (uint32_t)(min(64 * x + 64, xhi) - max(64 * x, xlo)) * s_col[3 * x + c];
        const uint64_t hw = (uint64_t)H * (uint64_t)W;
        out[((int64_t)f * FIT_SIDE + oy) * (3 * FIT_SIDE) + t] = (uint8_t)((2ull * S + hw) / (2ull * hw));
    }
}

__global__ void __launch_bounds__(FIT_THREADS)
fit_up_kernel(const void* __restrict__ map, int map_kind, const uint8_t* __restrict__ guide, const uint8_t* __restrict__ low, int H, int W,
              float cs, float cr, float inv2h, float inv2w, float thresh, int inclusive, float* __restrict__ soft,
              uint8_t* __restrict__ grey, uint8_t* __restrict__ hard) {
    __shared__ uint32_t s_low[FIT_TAPS][FIT_SIDE];                         // r | g << 8 | b << 16
    __shared__ uint32_t s_ll[FIT_TAPS][FIT_SIDE];                          // r^2 + g^2 + b^2
    __shared__ float s_map[FIT_TAPS][FIT_SIDE];
    const int qy0 = blockIdx.y, f = blockIdx.z, t = threadIdx.x;
    const int x = blockIdx.x * FIT_THREADS + t;
    const float inf = __builtin_inff();

    // the five cell rows of this band; a row outside the grid is never read back (its ey is +inf and its registers are preset)
    for (int i = t; i < FIT_TAPS * FIT_SIDE; i += FIT_THREADS) {
        const int r = i / FIT_SIDE, qx = i & (FIT_SIDE - 1), qy = qy0 + r - FIT_R;
        if (qy >= 0 && qy < FIT_SIDE) {
            const int64_t cell = ((int64_t)f * FIT_SIDE + qy) * FIT_SIDE + qx;
            const uint32_t cr_ = low[3 * cell], cg_ = low[3 * cell + 1], cb_ = low[3 * cell + 2];
            s_low[r][qx] = cr_ | (cg_ << 8) | (cb_ << 16);
            s_ll[r][qx] = cr_ * cr_ + cg_ * cg_ + cb_ * cb_;
            s_map[r][qx] = map_kind == CGS_FIT_MAP_U8 ? (static_cast<const uint8_t*>(map)[cell] ? 1.0f : 0.0f)
                                                      : static_cast<const float*>(map)[cell];
        }
    }
    __syncthreads();
    if (x >= W) return;

    // this column's taps: the same cells for every row of the band
    const int qx0 = ((2 * x + 1) * 32) / W;
    uint32_t lw[FIT_TAPS][FIT_TAPS], ll[FIT_TAPS][FIT_TAPS];
    float m[FIT_TAPS][FIT_TAPS], ex[FIT_TAPS];
#pragma unroll
    for (int dx = 0; dx < FIT_TAPS; ++dx) {
        const int qx = qx0 + dx - FIT_R;
        const float fx = (float)((2 * x + 1) * 64 - W * (2 * qx + 1)) * inv2w;
        ex[dx] = (qx >= 0 && qx < FIT_SIDE) ? fx * fx * cs : inf;
    }
#pragma unroll
    for (int dy = 0; dy < FIT_TAPS; ++dy) {
        const int qy = qy0 + dy - FIT_R;
#pragma unroll
        for (int dx = 0; dx < FIT_TAPS; ++dx) {
            const int qx = qx0 + dx - FIT_R;
            const bool in = qy >= 0 && qy < FIT_SIDE && qx >= 0 && qx < FIT_SIDE;
            lw[dy][dx] = in ? s_low[dy][qx] : 0u;
            ll[dy][dx] = in ? s_ll[dy][qx] : FIT_FAR;
            m[dy][dx] = in ? s_map[dy][qx] : 0.0f;
        }
    }

    const int ylo = (qy0 * H + 31) >> 6, yhi = ((qy0 + 1) * H + 31) >> 6;   // the rows y with ((2 y + 1) 32) / H == qy0
    for (int y = ylo; y < yhi; ++y) {
        const int64_t p = ((int64_t)f * H + y) * W + x;
        const uint32_t g = (uint32_t)guide[3 * p] | ((uint32_t)guide[3 * p + 1] << 8) | ((uint32_t)guide[3 * p + 2] << 16);
        const uint32_t gg = px_dot3(g, g);
        float ey[FIT_TAPS];
#pragma unroll
        for (int dy = 0; dy < FIT_TAPS; ++dy) {
            const int qy = qy0 + dy - FIT_R;
            const float fy = (float)((2 * y + 1) * 64 - H * (2 * qy + 1)) * inv2h;
            ey[dy] = (qy >= 0 && qy < FIT_SIDE) ? fy * fy * cs : inf;
        }
        uint32_t d2[FIT_TAPS][FIT_TAPS], dmin = FIT_FAR;
#pragma unroll
        for (int dy = 0; dy < FIT_TAPS; ++dy)
#pragma unroll
            for (int dx = 0; dx < FIT_TAPS; ++dx) {
                d2[dy][dx] = gg + ll[dy][dx] - 2u * px_dot3(g, lw[dy][dx]);
                dmin = min(dmin, d2[dy][dx]);
            }
        float num = 0.0f, den = 0.0f;
#pragma unroll
        for (int dy = 0; dy < FIT_TAPS; ++dy)
#pragma unroll
            for (int dx = 0; dx < FIT_TAPS; ++dx) {
                const float arg = fmaf((float)(d2[dy][dx] - dmin), cr, ey[dy] + ex[dx]);
                const float w = __builtin_amdgcn_exp2f(-arg);
                num = fmaf(w, m[dy][dx], num);
                den += w;
            }
        const float s = num / den;
        if (soft) soft[p] = s;
        if (grey) grey[p] = (uint8_t)(s * 255.0f);
        if (hard) hard[p] = inclusive ? (s >= thresh) : (s > thresh);
    }
}

template <int VEC>
void fit_down_launch(const uint8_t* frames, int n, int h, int w, uint8_t* out, hipStream_t stream) {
    hipLaunchKernelGGL(fit_down_kernel<VEC>, dim3((unsigned)n * FIT_SIDE), dim3(FIT_THREADS), (size_t)3 * w * sizeof(uint32_t), stream, frames,
                       h, w, out);
}

}  // namespace

extern "C" int cgs_fit_down_u8(const uint8_t* frames, int32_t n, int32_t h, int32_t w, uint8_t* out, cgs_stream_t stream_) {
    if (!frames || !out || n < 1 || h < 1 || w < 1 || (int64_t)n * FIT_SIDE > 0x7fffffffll) return CGS_ERR_BADARG;
    if (h < FIT_SIDE || w < FIT_SIDE || h > CGS_FIT_MAX_SIDE || w > CGS_FIT_MAX_SIDE) return CGS_ERR_UNSUPPORTED;
    const uintptr_t a = (uintptr_t)frames | (uintptr_t)(3 * w);            // every row starts at frames + a multiple of 3 w
    if (!(a & 15u)) fit_down_launch<16>(frames, n, h, w, out, (hipStream_t)stream_);
    else if (!(a & 3u)) fit_down_launch<4>(frames, n, h, w, out, (hipStream_t)stream_);
    else fit_down_launch<1>(frames, n, h, w, out, (hipStream_t)stream_);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}

extern "C" int cgs_fit_up_joint(const void* map, int32_t map_kind, const uint8_t* guide, const uint8_t* low, int32_t n, int32_t h, int32_t w,
                                float sigma_s, float sigma_r, float thresh, int32_t inclusive, float* soft, uint8_t* grey, uint8_t* hard,
                                cgs_stream_t stream_) {
    if (!map || !guide || !low || n < 1 || n > 65535 || h < 1 || w < 1 || (map_kind != CGS_FIT_MAP_F32 && map_kind != CGS_FIT_MAP_U8) ||
        !(sigma_s >= 0.5f) || !(sigma_r > 0.0f) || sigma_s > 3.0e38f || sigma_r > 3.0e38f || (hard && thresh != thresh) ||
        (map_kind == CGS_FIT_MAP_F32 && ((uintptr_t)map & 3u)) || ((uintptr_t)soft & 3u))
        return CGS_ERR_BADARG;
    if (h < FIT_SIDE || w < FIT_SIDE || h > CGS_FIT_MAX_SIDE || w > CGS_FIT_MAX_SIDE) return CGS_ERR_UNSUPPORTED;
    if (!soft && !grey && !hard) return CGS_OK;
    const double log2e = 1.4426950408889634;
    const float cs = (float)(log2e / (2.0 * (double)sigma_s * (double)sigma_s)), cr = (float)(log2e / (2.0 * (double)sigma_r * (double)sigma_r));
    hipLaunchKernelGGL(fit_up_kernel, dim3((unsigned)((w + FIT_THREADS - 1) / FIT_THREADS), FIT_SIDE, (unsigned)n), dim3(FIT_THREADS), 0,
                       (hipStream_t)stream_, map, (int)map_kind, guide, low, (int)h, (int)w, cs, cr, (float)(1.0 / (2.0 * h)),
                       (float)(1.0 / (2.0 * w)), thresh, (int)inclusive, soft, grey, hard);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}
