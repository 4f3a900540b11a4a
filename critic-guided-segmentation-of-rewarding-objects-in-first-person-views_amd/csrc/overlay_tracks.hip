// The overlay video of -process --source-video --overlay-tracks (include/cgs_hip.h): cgs_overlay_compose_tracks is cgs_overlay_compose
// with a colour per tracked object in place of the one tint, and with every object's bounding box and track number drawn on the overlay
// panel, all in integers.  The left panel, the grey panel, the tint formula and the outline are those of csrc/overlay.hip: both kernels
// are built from csrc/overlay_body.h, and what is here is what the tracked overlay stages and step 3 with its colour per pixel.
//
//   colour    of track t >= 1: c_k = 64 + ((t 2654435761 mod 2^32) >> 8 k & 255) 191 / 255, track_paint_kernel's (csrc/objects_track.hip);
//             of no track: the caller's colour.
//   object    of pixel (y, x): the label of its home cell ((2 p + 1) 32) / L when that is 1..K; with a home label of 0 the labelled cell of
//             the 5 x 5 cells around the home cell nearest to the pixel's centre (dxn^2 H^2 + dyn^2 W^2 in 64 bits, ties in raster order);
//             with a home label above K none.
//   box       of object l with area > 0 and a track: the pixels of cells x0..x1, y0..y1 (cell c of an axis of length L holds the pixels
//             (c L + 31) / 64 .. ((c + 1) L + 31) / 64 - 1); its border is B pixels thick; a plate of s (6 d + 1) x 9 s pixels at its top
//             left corner carries the d digits of the track number, 5 x 7 glyphs of the caller's font scaled by s = max(1, min(H, W) / 256).
//   priority  plate (smallest label first), border (smallest label first), outline, tint.
//
// A workgroup takes a band of OV_BAND rows of one frame (csrc/overlay_body.h) and stages besides the bit rows of the outline:
//   cells     the label rows of the band's cells and 2 rows above and below, a byte a cell (0: none, 255: above K), with 2 zero columns
//             each side: a cell outside the grid and an unlabelled cell read the same, so the search has no bounds to check.  A second
//             pass marks the unlabelled cells of the band's own rows that have a labelled cell among their 5 x 5 with 254: only their
//             pixels search (a network's mask is rarely exactly 0, so grey != 0 far from every object is the common case);
//   colours   of the labels 0..K of the frame;
//   boxes     in pixels, those whose rows (the plate's included) cross the band, in label order: wave 0, one lane an object, ordered by a
//             ballot -- no atomics.
// A thread takes PX = 16, 4 or 1 pixels as there, first collects the boxes that touch its pixels in a 64-bit mask, and only then looks at
// them pixel by pixel.  The search runs only where its answer can show: grey != 0 or an outline pixel, and a home label of 0; its
// distances are sums of a per-column and a per-row term, each one 32 x 32 -> 64 bit product.  A home cell ((2 p + 1) 32) / L is one
// multiply-high by ceil(2^32 / L): exact for L <= 4096, where (2 p + 1) 32 < 2^18 and the multiplier's error L' < L gives a 2^18 L' < 2^32.
// 40 KB of LDS, four workgroups a compute unit as csrc/overlay.hip.
#include "overlay_body.h"

namespace {

constexpr int OT_SIDE = CGS_FIT_SIDE, OT_R = CGS_FIT_RADIUS;              // the 64-cell grid and the search radius
constexpr int OT_CELL_ROWS = OV_BAND + 2 * OT_R;                          // H >= 64: a band of 16 rows lies in at most 16 cell rows
constexpr int OT_CELL_COLS = OT_SIDE + 2 * OT_R;
constexpr int OT_K = CGS_OVERLAY_MAX_TRACK_OBJECTS;
constexpr uint8_t OT_ABOVE = 255;                                         // a label above K
constexpr uint8_t OT_NEAR = 254;                                          // unlabelled, with a labelled cell among the 5 x 5 around it

struct OtBox {                                                            // in pixels, inclusive; all below 4096 + 16 * 61
    int16_t x0, y0, x1, y1;                                               // the rectangle
    int16_t xe, ye;                                                       // the last column / row of rectangle and plate together
    int16_t pw;                                                           // the plate's width
    uint32_t colour;
    unsigned long long digits;                                            // 4 bits a digit, the most significant in bits 0..3
};

struct OtShared {
    OvOutline outline;
    uint8_t cell[OT_CELL_ROWS][OT_CELL_COLS];
    uint32_t colour[OT_K + 1];
    OtBox box[OT_K];
    int nbox;
    uint8_t font[CGS_OVERLAY_FONT_GLYPHS * CGS_OVERLAY_FONT_ROWS];
};

__device__ __forceinline__ uint32_t ot_track_colour(uint32_t t) {         // t >= 1; r | g << 8 | b << 16
    const uint32_t hsh = t * 2654435761u;
    uint32_t c = 0u;
#pragma unroll
    for (int k = 0; k < 3; ++k) c |= (64u + ((hsh >> (8 * k)) & 255u) * 191u / 255u) << (8 * k);
    return c;
}

__device__ __forceinline__ int ot_home(int p, uint32_t inv) {              // ((2 p + 1) 32) / L with inv = ceil(2^32 / L)
    return (int)__umulhi((uint32_t)(2 * p + 1) * 32u, inv);
}

// The label of the cell nearest to the centre of pixel (y, x) among the labelled cells of the 5 x 5 window around its home cell
// (row `lr` of sh.cell, column cx + OT_R); 0 when there is none.  |dxn| <= 6 W and |dyn| <= 6 H (a window cell's centre is at most three
// cells from the pixel's), so a square is below 2^32 and a distance below 2^56.
__device__ __forceinline__ uint32_t ot_search(const OtShared& sh, int y, int x, int cy, int cx, int lr, int H, int W) {
    const uint32_t hh = (uint32_t)(H * H), ww = (uint32_t)(W * W);
    unsigned long long ex[2 * OT_R + 1], ey[2 * OT_R + 1];
#pragma unroll
    for (int d = -OT_R; d <= OT_R; ++d) {
        const int dxn = (2 * x + 1) * OT_SIDE - (2 * (cx + d) + 1) * W;
        const int dyn = (2 * y + 1) * OT_SIDE - (2 * (cy + d) + 1) * H;
        ex[d + OT_R] = (unsigned long long)(uint32_t)(dxn * dxn) * hh;
        ey[d + OT_R] = (unsigned long long)(uint32_t)(dyn * dyn) * ww;
    }
    unsigned long long best = ~0ull;
    uint32_t pick = 0u;
#pragma unroll
    for (int dy = 0; dy <= 2 * OT_R; ++dy) {                              // raster order; a later cell wins only when strictly nearer
#pragma unroll
        for (int dx = 0; dx <= 2 * OT_R; ++dx) {
            const uint32_t l = sh.cell[lr + dy - OT_R][cx + dx];
            const unsigned long long cost = ex[dx] + ey[dy];
            if (l != 0u && l < OT_NEAR && cost < best) {
                best = cost;
                pick = l;
            }
        }
    }
    return pick;
}

// cgs_overlay_compose_tracks_carried (CARRIED): an object with age > 0 has bit 24 (OT_CARRIED) set in its sh.colour and in its box's colour
// -- above the three channels, so no byte that is written sees it.  Off the stripe ((x + y) / (2 s) odd) such an object's pixel takes no
// tint and its box has no border; plate, digits and outline are as without the flag.  Everything the flag adds stands under
// `if constexpr (CARRIED)`: the kernel of cgs_overlay_compose_tracks is the one it was.
constexpr uint32_t OT_CARRIED = 1u << 24;

// Plate and border of the boxes in `hits` at pixel (y, x): true and the colour when one of them covers the pixel.
template <bool CARRIED>
__device__ __forceinline__ bool ot_decorate(const OtShared& sh, unsigned long long hits, int y, int x, int s, int thick, bool stripe,
                                            uint32_t* colour) {
    unsigned long long m = hits;
#pragma unroll 1
    while (m) {
        const OtBox& b = sh.box[__builtin_ctzll(m)];
        m &= m - 1;
        const int px = x - b.x0, py = y - b.y0;
        if (px < 0 || px >= b.pw || py < 0 || py >= 9 * s) continue;
        uint32_t c = b.colour;
        const int ux = px / s - 1, uy = py / s - 1;                       // glyph origins are multiples of s: whole units of s from the plate
        if (ux >= 0 && uy >= 0 && uy < CGS_OVERLAY_FONT_ROWS) {
            const int j = ux / 6, gx = ux - 6 * j;                        // px < s (6 d + 1): j < d
            const uint32_t digit = (uint32_t)(b.digits >> (4 * j)) & 15u;
            if (gx < 5 && ((sh.font[digit * CGS_OVERLAY_FONT_ROWS + uy] >> (4 - gx)) & 1u)) c = 0u;
        }
        *colour = c;
        return true;
    }
    m = hits;
#pragma unroll 1
    while (m) {
        const OtBox& b = sh.box[__builtin_ctzll(m)];
        m &= m - 1;
        if (x < b.x0 || x > b.x1 || y < b.y0 || y > b.y1) continue;
        if constexpr (CARRIED)
            if ((b.colour & OT_CARRIED) && !stripe) continue;             // a carried object's border is hatched
        if (x - b.x0 < thick || b.x1 - x < thick || y - b.y0 < thick || b.y1 - y < thick) {
            *colour = b.colour;
            return true;
        }
    }
    return false;
}

template <int PX, bool NT, bool CARRIED>
__global__ void __launch_bounds__(OV_THREADS)
overlay_tracks_kernel(const uint8_t* __restrict__ guide, const uint8_t* __restrict__ grey, const uint8_t* __restrict__ hard,
                      const int32_t* __restrict__ labels, const int32_t* __restrict__ ids, const int32_t* __restrict__ table,
                      const uint8_t* __restrict__ font, int H, int W, int K, uint32_t tint, uint32_t alpha256, int thick, int boxes,
                      int panels, uint8_t* __restrict__ out, const int32_t* __restrict__ age) {
    __shared__ OtShared sh;
    const int t = threadIdx.x, f = blockIdx.y, y0 = (int)blockIdx.x * OV_BAND;
    const int rows = min(OV_BAND, H - y0);
    const bool outline = hard != nullptr && thick > 0;                    // (the same in every thread)
    const int s = max(1, min(H, W) >> 8);                                 // the scale of plate and digits
    const uint32_t inv_h = (uint32_t)((0xFFFFFFFFull + (uint32_t)H) / (uint32_t)H);      // ceil(2^32 / H)
    const uint32_t inv_w = (uint32_t)((0xFFFFFFFFull + (uint32_t)W) / (uint32_t)W);
    const int c_lo = ot_home(y0, inv_h) - OT_R;                           // the cell row of sh.cell[0]
    const int c_rows = ot_home(y0 + rows - 1, inv_h) - c_lo + 1 + OT_R;   // <= OT_CELL_ROWS

    // ---- cells, colours, font, boxes
    {
        const int32_t* lf = labels + (int64_t)f * OT_SIDE * OT_SIDE;
        for (int item = t; item < c_rows * OT_CELL_COLS; item += OV_THREADS) {
            const int lr = item / OT_CELL_COLS, lc = item - lr * OT_CELL_COLS;
            const int cy = c_lo + lr, cx = lc - OT_R;
            uint8_t v = 0;
            if (cy >= 0 && cy < OT_SIDE && cx >= 0 && cx < OT_SIDE) {
                const int32_t l = lf[cy * OT_SIDE + cx];
                v = l <= 0 ? (uint8_t)0 : (l <= K ? (uint8_t)l : OT_ABOVE);
            }
            sh.cell[lr][lc] = v;
        }
        if (t <= OT_K) {
            uint32_t c = tint;
            if (t >= 1 && t <= K) {
                const int32_t id = ids[(int64_t)f * K + t - 1];
                if (id > 0) c = ot_track_colour((uint32_t)id);
                if constexpr (CARRIED)
                    if (age[(int64_t)f * K + t - 1] > 0) c |= OT_CARRIED;
            }
            sh.colour[t] = c;
        }
        if (t >= 64 && t < 64 + CGS_OVERLAY_FONT_GLYPHS * CGS_OVERLAY_FONT_ROWS) sh.font[t - 64] = font[t - 64];
        if (t < 64) {                                                     // wave 0: lane t is object t + 1
            bool keep = false;
            OtBox b;
            if (boxes > 0 && t < K) {
                const int32_t* row = table + ((int64_t)f * K + t) * CGS_OBJ_FIELDS;
                const int32_t id = ids[(int64_t)f * K + t];
                const int area = row[0], cx0 = row[1], cy0 = row[2], cx1 = row[3], cy1 = row[4];
                if (area > 0 && id > 0 && cx0 >= 0 && cy0 >= 0 && cx0 <= cx1 && cy0 <= cy1 && cx1 < OT_SIDE && cy1 < OT_SIDE) {
                    b.x0 = (int16_t)((cx0 * W + 31) >> 6);
                    b.x1 = (int16_t)((((cx1 + 1) * W + 31) >> 6) - 1);
                    b.y0 = (int16_t)((cy0 * H + 31) >> 6);
                    b.y1 = (int16_t)((((cy1 + 1) * H + 31) >> 6) - 1);
                    uint32_t v = (uint32_t)id;
                    unsigned long long digits = 0ull;
                    int d = 0;
                    do {                                                  // the least significant digit first: it ends in the highest place
                        digits = (digits << 4) | (v % 10u);
                        v /= 10u;
                        ++d;
                    } while (v);
                    b.digits = digits;
                    b.pw = (int16_t)(s * (6 * d + 1));
                    b.xe = (int16_t)max((int)b.x1, b.x0 + b.pw - 1);
                    b.ye = (int16_t)max((int)b.y1, b.y0 + 9 * s - 1);
                    b.colour = ot_track_colour((uint32_t)id);
                    if constexpr (CARRIED)
                        if (age[(int64_t)f * K + t] > 0) b.colour |= OT_CARRIED;
                    keep = b.ye >= y0 && b.y0 <= y0 + rows - 1;
                }
            }
            const unsigned long long kept = __ballot(keep);
            if (keep) sh.box[__popcll(kept & ((1ull << t) - 1ull))] = b;
            if (t == 0) sh.nbox = __popcll(kept);
        }
    }

    __syncthreads();
    for (int item = t; item < (c_rows - 2 * OT_R) * OT_SIDE; item += OV_THREADS) {       // the cells that are some pixel's home cell
        const int lr = OT_R + item / OT_SIDE, lc = OT_R + (item & (OT_SIDE - 1));
        if (sh.cell[lr][lc] != 0u) continue;
        bool any = false;
#pragma unroll
        for (int dy = -OT_R; dy <= OT_R; ++dy)
#pragma unroll
            for (int dx = -OT_R; dx <= OT_R; ++dx) {
                const uint32_t l = sh.cell[lr + dy][lc + dx];             // (0 or OT_NEAR, whichever a neighbour's pass has left: neither counts)
                any |= l != 0u && l < OT_NEAR;
            }
        if (any) sh.cell[lr][lc] = OT_NEAR;
    }

    // every path reaches a barrier between the pass above and the streaming below: ov_outline ends on one
    if (outline)
        ov_outline(sh.outline, hard, f, y0, rows, H, W, thick);
    else
        __syncthreads();

    const int last = thick & 1;                                           // the buffer that holds E_t
    const int groups = W / PX;                                            // PX divides W (ov_dispatch chose it so)
    const int nbox = sh.nbox;
    const int64_t frame_px = (int64_t)f * H * W;
    const int64_t out_row = (int64_t)3 * panels * W;
    for (int item = t; item < rows * groups; item += OV_THREADS) {
        const int ry = item / groups, gx = item - ry * groups;
        const int y = y0 + ry, x = gx * PX;
        const int64_t p = frame_px + (int64_t)y * W + x;
        uint8_t* dst = out + ((int64_t)f * H + y) * out_row + 3 * x;
        uint32_t ol = 0u;                                                 // bit i: pixel x + i is on the outline
        if (outline) {
            const int lr = ry + thick, j = x >> 6, sh_ = x & 63;          // PX divides 64: the PX bits lie in one word
            ol = (uint32_t)((sh.outline.hard[lr][j] & ~sh.outline.e[last][lr][j]) >> sh_);
        }
        const int cy = ot_home(y, inv_h), lr = cy - c_lo;
        unsigned long long hits = 0ull;                                   // the boxes that touch these PX pixels
        for (int e = 0; e < nbox; ++e) {
            const OtBox& b = sh.box[e];
            if (y >= b.y0 && y <= b.ye && x + PX - 1 >= b.x0 && x <= b.xe) hits |= 1ull << e;
        }
        // the overlay colour of pixel x + i: frame (r, g, b), grey byte g, outline bit o
        auto pixel = [&](int i, uint32_t r, uint32_t gg, uint32_t b, uint32_t g, bool o) -> uint32_t {
            uint32_t c;
            bool stripe = true;
            if constexpr (CARRIED) stripe = (((uint32_t)(x + i + y) / (uint32_t)(2 * s)) & 1u) == 0u;
            if (hits && ot_decorate<CARRIED>(sh, hits, y, x + i, s, boxes, stripe, &c)) return c;
            c = tint;
            if (g != 0u || o) {                                           // elsewhere the colour does not show
                const int cx = ot_home(x + i, inv_w);
                uint32_t l = sh.cell[lr][cx + OT_R];
                if (l == OT_NEAR) l = ot_search(sh, y, x + i, cy, cx, lr, H, W);
                if (l < OT_NEAR) c = sh.colour[l];
            }
            if (o) return c;
            uint32_t q = alpha256 * g;
            if constexpr (CARRIED) {
                if ((c & OT_CARRIED) && !stripe) q = 0u;                  // off the stripe the frame's pixel passes through
                c &= ~OT_CARRIED;
            }
            return ov_tint(r, c & 255u, q) | (ov_tint(gg, (c >> 8) & 255u, q) << 8) | (ov_tint(b, c >> 16, q) << 16);
        };
        if constexpr (PX == 1) {
            const uint32_t g = grey[p];
            const uint32_t r = guide[3 * p], gg = guide[3 * p + 1], b = guide[3 * p + 2];
            const uint32_t v = pixel(0, r, gg, b, g, ol & 1u);
            uint8_t* at = dst;
            if (panels > 1) {
                px_put<NT>(at, (uint8_t)r); px_put<NT>(at + 1, (uint8_t)gg); px_put<NT>(at + 2, (uint8_t)b);
                at += 3 * W;
            }
            px_put<NT>(at, (uint8_t)v); px_put<NT>(at + 1, (uint8_t)(v >> 8)); px_put<NT>(at + 2, (uint8_t)(v >> 16));
            if (panels > 2) {
                at += 3 * W;
                px_put<NT>(at, (uint8_t)g); px_put<NT>(at + 1, (uint8_t)g); px_put<NT>(at + 2, (uint8_t)g);
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
                const uint32_t g = (gw[i >> 2] >> (8 * (i & 3))) & 255u;
                uint32_t ch[3];
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int b = 3 * i + c;                              // byte of the group
                    ch[c] = (fr[b >> 2] >> (8 * (b & 3))) & 255u;
                }
                const uint32_t v = pixel(i, ch[0], ch[1], ch[2], g, (ol >> i) & 1u);
#pragma unroll
                for (int c = 0; c < 3; ++c) {
                    const int b = 3 * i + c;
                    ov[b >> 2] |= ((v >> (8 * c)) & 255u) << (8 * (b & 3));
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

}  // namespace

extern "C" int cgs_overlay_compose_tracks(const uint8_t* guide, const uint8_t* grey, const uint8_t* hard, const int32_t* labels,
                                          const int32_t* ids, const int32_t* table, const uint8_t* font, int32_t n, int32_t h, int32_t w,
                                          int32_t max_objects, int32_t r, int32_t g, int32_t b, int32_t alpha256, int32_t thickness,
                                          int32_t boxes, int32_t layout, int32_t flags, uint8_t* out, cgs_stream_t stream_) {
    const bool bad = !labels || !ids || !table || !font || max_objects < 1 || boxes < 0 || boxes > CGS_OVERLAY_MAX_BOXES ||
                     (((uintptr_t)labels | (uintptr_t)ids | (uintptr_t)table) & 3u);
    OvLaunch l;
    if (const int rc = ov_prepare(guide, grey, out, n, h, w, r, g, b, alpha256, thickness, layout, flags, bad, &l)) return rc;
    if (max_objects > OT_K) return CGS_ERR_UNSUPPORTED;
    ov_dispatch(guide, grey, out, w, flags, [&](auto px, auto nt) {
        hipLaunchKernelGGL((overlay_tracks_kernel<decltype(px)::value, decltype(nt)::value, false>), l.grid, dim3(OV_THREADS), 0,
                           (hipStream_t)stream_, guide, grey, hard, labels, ids, table, font, (int)h, (int)w, (int)max_objects, l.tint,
                           (uint32_t)alpha256, (int)thickness, (int)boxes, (int)layout, out, (const int32_t*)nullptr);
    });
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}

extern "C" int cgs_overlay_compose_tracks_carried(const uint8_t* guide, const uint8_t* grey, const uint8_t* hard, const int32_t* labels,
                                                  const int32_t* ids, const int32_t* table, const int32_t* age, const uint8_t* font,
                                                  int32_t n, int32_t h, int32_t w, int32_t max_objects, int32_t r, int32_t g, int32_t b,
                                                  int32_t alpha256, int32_t thickness, int32_t boxes, int32_t layout, int32_t flags,
                                                  uint8_t* out, cgs_stream_t stream_) {
    const bool bad = !labels || !ids || !table || !age || !font || max_objects < 1 || boxes < 0 || boxes > CGS_OVERLAY_MAX_BOXES ||
                     (((uintptr_t)labels | (uintptr_t)ids | (uintptr_t)table | (uintptr_t)age) & 3u);
    OvLaunch l;
    if (const int rc = ov_prepare(guide, grey, out, n, h, w, r, g, b, alpha256, thickness, layout, flags, bad, &l)) return rc;
    if (max_objects > OT_K) return CGS_ERR_UNSUPPORTED;
    ov_dispatch(guide, grey, out, w, flags, [&](auto px, auto nt) {
        hipLaunchKernelGGL((overlay_tracks_kernel<decltype(px)::value, decltype(nt)::value, true>), l.grid, dim3(OV_THREADS), 0,
                           (hipStream_t)stream_, guide, grey, hard, labels, ids, table, font, (int)h, (int)w, (int)max_objects, l.tint,
                           (uint32_t)alpha256, (int)thickness, (int)boxes, (int)layout, out, age);
    });
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}
