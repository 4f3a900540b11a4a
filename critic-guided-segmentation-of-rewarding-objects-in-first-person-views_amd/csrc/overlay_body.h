// What the two overlay kernels share: cgs_overlay_compose (csrc/overlay.hip) and cgs_overlay_compose_tracks (csrc/overlay_tracks.hip)
// differ in the colour an overlay pixel takes and in what the tracked kernel stages for it.  The tint formula, the outline and its edge
// convention, the band, the packed loads and stores, the argument check and the choice of the access width are stated here and nowhere
// else.  Step 3 below stays written out in each kernel, around its own colour: one loop for both, a template over the pixel's colour,
// gave the same bytes but a tracked kernel 1 to 2 % slower with objects in the frame (profiles/video_refactor_ab.md).
//
//   tint      q = alpha256 grey (<= 65280);  out_c = (frame_c (65280 - q) + tint_c q + 32640) / 65280: below 2^24, one 32-bit division by a
//             constant.
//   outline   E_0 = hard; E_{i+1}[p] = E_i[p] and its four neighbours' E_i, a neighbour OUTSIDE the frame counting as on; a pixel is on
//             the outline when hard[p] & ~E_t[p] and is then the overlay colour, opaque.  The frame's edge counting as on means a mask that
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
#pragma once
#include <type_traits>

#include "pixel_common.h"

constexpr int OV_THREADS = 256;
constexpr int OV_BAND = 16;                                               // rows of a band
constexpr int OV_ROWS = OV_BAND + 2 * CGS_OVERLAY_MAX_OUTLINE;            // staged bit rows at the thickest outline
constexpr int OV_WORDS = CGS_FIT_MAX_SIDE / 64;                           // 64-bit words of the longest row
constexpr uint32_t OV_DEN = 65280u, OV_HALF = 32640u;

typedef uint32_t ov_u32x4 __attribute__((ext_vector_type(4)));

struct OvOutline {                                                        // the bit rows of a band, in LDS
    unsigned long long hard[OV_ROWS][OV_WORDS];                           // E_0
    unsigned long long e[2][OV_ROWS][OV_WORDS];                           // E_i, E_{i+1}
};

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
            px_put<NT>(q + i, v);
        }
    } else {
        uint32_t* q = reinterpret_cast<uint32_t*>(p);
#pragma unroll
        for (int i = 0; i < 3; ++i) px_put<NT>(q + i, w[i]);
    }
}

__device__ __forceinline__ uint32_t ov_tint(uint32_t fr, uint32_t tint, uint32_t q) {
    return (fr * (OV_DEN - q) + tint * q + OV_HALF) / OV_DEN;
}

// Steps 1 and 2 for the band of `rows` rows from y0 of frame f.  Every thread of the workgroup calls it, under a condition that is the same
// in the whole workgroup (hard != NULL and thick > 0); it ends on a barrier, after which o.hard and o.e[thick & 1] hold the band's rows
// at rows thick .. thick + rows - 1.
__device__ __forceinline__ void ov_outline(OvOutline& o, const uint8_t* __restrict__ hard, int f, int y0, int rows, int H, int W, int thick) {
    const int t = threadIdx.x, nwords = (W + 63) >> 6;
    const int R = rows + 2 * thick, lane = t & 63, wave = t >> 6;
    const uint8_t* hf = hard + (int64_t)f * H * W;
    for (int item = wave; item < R * nwords; item += OV_THREADS / 64) {      // (the same in every lane of a wave)
        const int lr = item / nwords, j = item - lr * nwords;
        const int y = y0 - thick + lr, x = 64 * j + lane;
        const bool in = y >= 0 && y < H && x < W;
        const bool on = in ? hf[(int64_t)y * W + x] != 0 : true;
        const unsigned long long word = __ballot(on);
        if (lane == 0) {
            o.hard[lr][j] = word;
            o.e[0][lr][j] = word;
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
                const unsigned long long c = o.e[src][lr][j];
                const unsigned long long up = lr > 0 ? o.e[src][lr - 1][j] : ~0ull;
                const unsigned long long dn = lr + 1 < R ? o.e[src][lr + 1][j] : ~0ull;
                const unsigned long long lo = j > 0 ? o.e[src][lr][j - 1] >> 63 : 1ull;              // the pixel left of bit 0
                const unsigned long long hi = j + 1 < nwords ? o.e[src][lr][j + 1] << 63 : 1ull << 63; // the pixel right of bit 63
                e = c & up & dn & ((c << 1) | lo) & ((c >> 1) | hi);
                if (j + 1 == nwords) e |= past;
            }
            o.e[dst][lr][j] = e;
        }
        __syncthreads();
    }
}

// ---------------------------------------------------------------------------------------------------------------- the host side
struct OvLaunch {
    uint32_t tint;                                                        // r | g << 8 | b << 16
    dim3 grid;                                                            // (bands of a frame, frames)
};

// The arguments that both entries take.  `more_bad`: an argument error of the caller's own; like every argument error it comes before
// CGS_ERR_UNSUPPORTED.
inline int ov_prepare(const uint8_t* guide, const uint8_t* grey, const uint8_t* out, int32_t n, int32_t h, int32_t w, int32_t r, int32_t g,
                      int32_t b, int32_t alpha256, int32_t thickness, int32_t layout, int32_t flags, bool more_bad, OvLaunch* l) {
    if (!guide || !grey || !out || n < 1 || n > 65535 || h < 1 || w < 1 || r < 0 || r > 255 || g < 0 || g > 255 || b < 0 || b > 255 ||
        alpha256 < 0 || alpha256 > 256 || thickness < 0 || thickness > CGS_OVERLAY_MAX_OUTLINE || layout < CGS_OVERLAY_ONLY ||
        layout > CGS_OVERLAY_TRIPLE || (flags & ~CGS_OVERLAY_NONTEMPORAL) || more_bad)
        return CGS_ERR_BADARG;
    if (h < CGS_FIT_SIDE || w < CGS_FIT_SIDE || h > CGS_FIT_MAX_SIDE || w > CGS_FIT_MAX_SIDE) return CGS_ERR_UNSUPPORTED;
    l->tint = (uint32_t)r | ((uint32_t)g << 8) | ((uint32_t)b << 16);
    l->grid = dim3((unsigned)((h + OV_BAND - 1) / OV_BAND), (unsigned)n);
    return CGS_OK;
}

// Calls launch(PX, NT) with PX = 16, 4 or 1 and NT = true or false as std::integral_constants: the kernel's template arguments.  Every row
// of guide and out starts at a multiple of 3 w from the base, every panel 3 w further, every row of grey at a multiple of w, so the
// alignment of the three bases and of w is that of every access.
template <typename Launch>
void ov_dispatch(const uint8_t* guide, const uint8_t* grey, const uint8_t* out, int32_t w, int32_t flags, Launch launch) {
    const bool nt = flags & CGS_OVERLAY_NONTEMPORAL;
    auto either = [&](auto px) {
        if (nt)
            launch(px, std::true_type());
        else
            launch(px, std::false_type());
    };
    const uintptr_t a = (uintptr_t)guide | (uintptr_t)grey | (uintptr_t)out | (uintptr_t)w;
    if (!(a & 15u))
        either(std::integral_constant<int, 16>());
    else if (!(a & 3u))
        either(std::integral_constant<int, 4>());
    else
        either(std::integral_constant<int, 1>());
}
