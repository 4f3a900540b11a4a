// The overlay video of -process --source-video (include/cgs_hip.h): cgs_overlay_compose tints every frame by its upsampled mask, draws
// the outline of the thresholded mask and lays the panels of a frame side by side, all in integers.
//
//   tint      q = alpha256 grey (<= 65280);  out_c = (frame_c (65280 - q) + tint_c q + 32640) / 65280: below 2^24, one 32-bit division by a
//             constant.
//   outline   E_0 = hard; E_{i+1}[p] = E_i[p] and its four neighbours' E_i, a neighbour OUTSIDE the frame counting as on; a pixel is on
//             the outline when hard[p] & ~E_t[p] and is then the tint colour, opaque.  The frame's edge counting as on means a mask that
//             the frame cuts draws no line along the frame's edge -- the opposite of the scoring convention of boundary.hip, on purpose.
//
// A workgroup takes a band of OV_BAND rows of one frame:
//   1. pack    the hard rows of the band and t halo rows above and below become bit rows in LDS, 64 pixels a word by ballot (a row of 4096
//              is 64 words).  A row outside the frame and the bits past column W are all ones.
//   2. erode   t times on the bit rows, between two LDS buffers: a word ANDed with the words above and below and with itself shifted by one
//              bit each way, the bit that crosses a word boundary carried in from the neighbouring word (a one at the frame's edge).  Rows
//              outside the frame stay all ones.  After i passes rows i .. R - 1 - i of the R = OV_BAND + 2 t staged rows are right, so after
//              t passes the band's own rows are.
//   3. stream  a thread takes PX pixels at a time -- 16, 4 or 1: the widest for which guide, grey, out and W are all aligned, so that every
//              access is one 16-, 4- or 1-byte load or store -- reads the frame once and writes all panels.
// With hard == NULL or t == 0 steps 1 and 2 are not run.  Traffic per pixel: 3 + 1 bytes read (+ 1 of hard, the halo rows read twice), 3 k
// written.  No atomics, no allocation, deterministic.
#include "cgs_common.h"

namespace {

constexpr int OV_THREADS = 256;
constexpr int OV_BAND = 16;                                               // rows of a band
constexpr int OV_ROWS = OV_BAND + 2 * CGS_OVERLAY_MAX_OUTLINE;            // staged bit rows at the thickest outline
constexpr int OV_WORDS = CGS_FIT_MAX_SIDE / 64;                           // 64-bit words of the longest row
constexpr uint32_t OV_DEN = 65280u, OV_HALF = 32640u;

typedef uint32_t ov_u32x4 __attribute__((ext_vector_type(4)));

template <bool NT, typename T>
__device__ __forceinline__ void ov_put(T* p, const T& v) {
    if (NT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}

// PX pixels as 3 PX colour bytes in 32-bit words (PX = 16: 12 words, PX = 4: 3 words)
template <int PX>
__device__ __forceinline__ void ov_load_rgb(const uint8_t* p, uint32_t* w) {
    if constexpr (PX == 16) {
        const ov_u32x4* q = reinterpret_cast<const ov_u32x4*>(p);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            const ov_u32x4 v = q[i];
            w[4 * i] = v.x; w[4 * i + 1] = v.y; w[4 * i + 2] = v.z; w[4 * i + 3] = v.w;
        }
    } else {
        const uint32_t* q = reinterpret_cast<const uint32_t*>(p);
#pragma unroll
        for (int i = 0; i < 3; ++i) w[i] = q[i];
    }
}

template <int PX, bool NT>
__device__ __forceinline__ void ov_store_rgb(uint8_t* p, const uint32_t* w) {
    if constexpr (PX == 16) {
        ov_u32x4* q = reinterpret_cast<ov_u32x4*>(p);
#pragma unroll
        for (int i = 0; i < 3; ++i) {
            ov_u32x4 v;
            v.x = w[4 * i]; v.y = w[4 * i + 1]; v.z = w[4 * i + 2]; v.w = w[4 * i + 3];
            ov_put<NT>(q + i, v);
        }
    } else {
        uint32_t* q = reinterpret_cast<uint32_t*>(p);
#pragma unroll
        for (int i = 0; i < 3; ++i) ov_put<NT>(q + i, w[i]);
    }
}

__device__ __forceinline__ uint32_t ov_tint(uint32_t fr, uint32_t tint, uint32_t q) {
    return (fr * (OV_DEN - q) + tint * q + OV_HALF) / OV_DEN;
}

template <int PX, bool NT>
__global__ void __launch_bounds__(OV_THREADS)
overlay_kernel(const uint8_t* __restrict__ guide, const uint8_t* __restrict__ grey, const uint8_t* __restrict__ hard, int H, int W,
               uint32_t tint, uint32_t alpha256, int thick, int panels, uint8_t* __restrict__ out) {
    __shared__ unsigned long long s_hard[OV_ROWS][OV_WORDS];              // E_0
    __shared__ unsigned long long s_e[2][OV_ROWS][OV_WORDS];              // E_i, E_{i+1}
    const int t = threadIdx.x, f = blockIdx.y, y0 = (int)blockIdx.x * OV_BAND;
    const int rows = min(OV_BAND, H - y0);
    const int nwords = (W + 63) >> 6;
    const bool outline = hard != nullptr && thick > 0;                    // (the same in every thread)
    const int last = thick & 1;                                           // the buffer that holds E_t

    if (outline) {
        const int R = rows + 2 * thick, lane = t & 63, wave = t >> 6;
        const uint8_t* hf = hard + (int64_t)f * H * W;
        for (int item = wave; item < R * nwords; item += OV_THREADS / 64) {      // (the same in every lane of a wave)
            const int lr = item / nwords, j = item - lr * nwords;
            const int y = y0 - thick + lr, x = 64 * j + lane;
            const bool in = y >= 0 && y < H && x < W;
            const bool on = in ? hf[(int64_t)y * W + x] != 0 : true;
            const unsigned long long word = __ballot(on);
            if (lane == 0) {
                s_hard[lr][j] = word;
                s_e[0][lr][j] = word;
            }
        }
        __syncthreads();
        const unsigned long long past = (W & 63) ? ~0ull << (W & 63) : 0ull;      // the bits past column W in the last word: they stay on
        for (int i = 0; i < thick; ++i) {
            const int src = i & 1, dst = src ^ 1;
            for (int item = t; item < R * nwords; item += OV_THREADS) {
                const int lr = item / nwords, j = item - lr * nwords;
                const int y = y0 - thick + lr;
                unsigned long long e = ~0ull;
                if (y >= 0 && y < H) {
                    const unsigned long long c = s_e[src][lr][j];
                    const unsigned long long up = lr > 0 ? s_e[src][lr - 1][j] : ~0ull;
                    const unsigned long long dn = lr + 1 < R ? s_e[src][lr + 1][j] : ~0ull;
                    const unsigned long long lo = j > 0 ? s_e[src][lr][j - 1] >> 63 : 1ull;              // the pixel left of bit 0
                    const unsigned long long hi = j + 1 < nwords ? s_e[src][lr][j + 1] << 63 : 1ull << 63; // the pixel right of bit 63
                    e = c & up & dn & ((c << 1) | lo) & ((c >> 1) | hi);
                    if (j + 1 == nwords) e |= past;
                }
                s_e[dst][lr][j] = e;
            }
            __syncthreads();
        }
    }

    const int groups = W / PX;                                            // PX divides W (the entry chose it so)
    const int64_t frame_px = (int64_t)f * H * W;
    const int64_t out_row = (int64_t)3 * panels * W;
    const uint32_t tr = tint & 255u, tg = (tint >> 8) & 255u, tb = tint >> 16;
    for (int item = t; item < rows * groups; item += OV_THREADS) {
        const int ry = item / groups, gx = item - ry * groups;
        const int y = y0 + ry, x = gx * PX;
        const int64_t p = frame_px + (int64_t)y * W + x;
        uint8_t* dst = out + ((int64_t)f * H + y) * out_row + 3 * x;
        uint32_t ol = 0u;                                                 // bit i: pixel x + i is on the outline
        if (outline) {
            const int lr = ry + thick, j = x >> 6, sh = x & 63;           // PX divides 64: the PX bits lie in one word
            ol = (uint32_t)((s_hard[lr][j] & ~s_e[last][lr][j]) >> sh);
        }
        if constexpr (PX == 1) {
            const uint32_t g = grey[p], q = alpha256 * g;
            const uint32_t r = guide[3 * p], gg = guide[3 * p + 1], b = guide[3 * p + 2];
            const bool o = ol & 1u;
            const uint32_t vr = o ? tr : ov_tint(r, tr, q), vg = o ? tg : ov_tint(gg, tg, q), vb = o ? tb : ov_tint(b, tb, q);
            uint8_t* at = dst;
            if (panels > 1) {
                ov_put<NT>(at, (uint8_t)r); ov_put<NT>(at + 1, (uint8_t)gg); ov_put<NT>(at + 2, (uint8_t)b);
                at += 3 * W;
            }
            ov_put<NT>(at, (uint8_t)vr); ov_put<NT>(at + 1, (uint8_t)vg); ov_put<NT>(at + 2, (uint8_t)vb);
            if (panels > 2) {
                at += 3 * W;
                ov_put<NT>(at, (uint8_t)g); ov_put<NT>(at + 1, (uint8_t)g); ov_put<NT>(at + 2, (uint8_t)g);
            }
        } else {
            constexpr int NW = 3 * PX / 4;
            uint32_t fr[NW], ov[NW], gr[NW], gw[PX / 4];
            ov_load_rgb<PX>(guide + 3 * p, fr);
            if constexpr (PX == 16) {
                const ov_u32x4 v = *reinterpret_cast<const ov_u32x4*>(grey + p);
                gw[0] = v.x; gw[1] = v.y; gw[2] = v.z; gw[3] = v.w;
            } else {
                gw[0] = *reinterpret_cast<const uint32_t*>(grey + p);
            }
#pragma unroll
            for (int i = 0; i < NW; ++i) ov[i] = gr[i] = 0u;
#pragma unroll
            for (int i = 0; i < PX; ++i) {
                const uint32_t g = (gw[i >> 2] >> (8 * (i & 3))) & 255u, q = alpha256 * g;
                const bool o = (ol >> i) & 1u;
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int b = 3 * i + c;                              // byte of the group
                    const uint32_t v = (fr[b >> 2] >> (8 * (b & 3))) & 255u;
                    const uint32_t tc = c == 0 ? tr : (c == 1 ? tg : tb);
                    ov[b >> 2] |= (o ? tc : ov_tint(v, tc, q)) << (8 * (b & 3));
                    gr[b >> 2] |= g << (8 * (b & 3));
                }
            }
            uint8_t* at = dst;
            if (panels > 1) {
                ov_store_rgb<PX, NT>(at, fr);
                at += 3 * W;
            }
            ov_store_rgb<PX, NT>(at, ov);
            if (panels > 2) ov_store_rgb<PX, NT>(at + 3 * W, gr);
        }
    }
}

template <int PX>
void overlay_launch(bool nt, dim3 grid, hipStream_t s, const uint8_t* guide, const uint8_t* grey, const uint8_t* hard, int h, int w,
                    uint32_t tint, uint32_t alpha256, int thick, int panels, uint8_t* out) {
    if (nt)
        hipLaunchKernelGGL((overlay_kernel<PX, true>), grid, dim3(OV_THREADS), 0, s, guide, grey, hard, h, w, tint, alpha256, thick, panels, out);
    else
        hipLaunchKernelGGL((overlay_kernel<PX, false>), grid, dim3(OV_THREADS), 0, s, guide, grey, hard, h, w, tint, alpha256, thick, panels, out);
}

}  // namespace

extern "C" int cgs_overlay_compose(const uint8_t* guide, const uint8_t* grey, const uint8_t* hard, int32_t n, int32_t h, int32_t w,
                                   int32_t r, int32_t g, int32_t b, int32_t alpha256, int32_t thickness, int32_t layout, int32_t flags,
                                   uint8_t* out, cgs_stream_t stream_) {
    if (!guide || !grey || !out || n < 1 || n > 65535 || h < 1 || w < 1 || r < 0 || r > 255 || g < 0 || g > 255 || b < 0 || b > 255 ||
        alpha256 < 0 || alpha256 > 256 || thickness < 0 || thickness > CGS_OVERLAY_MAX_OUTLINE || layout < CGS_OVERLAY_ONLY ||
        layout > CGS_OVERLAY_TRIPLE || (flags & ~CGS_OVERLAY_NONTEMPORAL))
        return CGS_ERR_BADARG;
    if (h < CGS_FIT_SIDE || w < CGS_FIT_SIDE || h > CGS_FIT_MAX_SIDE || w > CGS_FIT_MAX_SIDE) return CGS_ERR_UNSUPPORTED;
    const uint32_t tint = (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
    const dim3 grid((unsigned)((h + OV_BAND - 1) / OV_BAND), (unsigned)n);
    const bool nt = flags & CGS_OVERLAY_NONTEMPORAL;
    // every row of guide and out starts at a multiple of 3 w from the base, every panel 3 w further, every row of grey at a multiple of w
    const uintptr_t a = (uintptr_t)guide | (uintptr_t)grey | (uintptr_t)out | (uintptr_t)w;
    if (!(a & 15u))
        overlay_launch<16>(nt, grid, (hipStream_t)stream_, guide, grey, hard, h, w, tint, (uint32_t)alpha256, thickness, layout, out);
    else if (!(a & 3u))
        overlay_launch<4>(nt, grid, (hipStream_t)stream_, guide, grey, hard, h, w, tint, (uint32_t)alpha256, thickness, layout, out);
    else
        overlay_launch<1>(nt, grid, (hipStream_t)stream_, guide, grey, hard, h, w, tint, (uint32_t)alpha256, thickness, layout, out);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}
