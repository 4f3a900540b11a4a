// The overlay video of -process --source-video (include/cgs_hip.h): cgs_overlay_compose tints every frame by its upsampled mask, draws
// the outline of the thresholded mask and lays the panels of a frame side by side, all in integers.  The formulas and the band algorithm
// (steps 1 to 3) are in csrc/overlay_body.h; what is here is step 3 with the plain overlay's colour -- one tint -- and the entry.
#include "overlay_body.h"

namespace {

template <int PX, bool NT>
__global__ void __launch_bounds__(OV_THREADS)
overlay_kernel(const uint8_t* __restrict__ guide, const uint8_t* __restrict__ grey, const uint8_t* __restrict__ hard, int H, int W,
               uint32_t tint, uint32_t alpha256, int thick, int panels, uint8_t* __restrict__ out) {
    __shared__ OvOutline s_o;
    const int f = blockIdx.y, y0 = (int)blockIdx.x * OV_BAND;
    const int rows = min(OV_BAND, H - y0);
    const bool outline = hard != nullptr && thick > 0;                    // (the same in every thread)
    if (outline) ov_outline(s_o, hard, f, y0, rows, H, W, thick);
    const int last = thick & 1;                                           // the buffer that holds E_t
    const int groups = W / PX;                                            // PX divides W (ov_dispatch chose it so)
    const int64_t frame_px = (int64_t)f * H * W;
    const int64_t out_row = (int64_t)3 * panels * W;
    const uint32_t tr = tint & 255u, tg = (tint >> 8) & 255u, tb = tint >> 16;
    for (int item = threadIdx.x; item < rows * groups; item += OV_THREADS) {
        const int ry = item / groups, gx = item - ry * groups;
        const int y = y0 + ry, x = gx * PX;
        const int64_t p = frame_px + (int64_t)y * W + x;
        uint8_t* dst = out + ((int64_t)f * H + y) * out_row + 3 * x;
        uint32_t ol = 0u;                                                 // bit i: pixel x + i is on the outline
        if (outline) {
            const int lr = ry + thick, j = x >> 6, sh = x & 63;           // PX divides 64: the PX bits lie in one word
            ol = (uint32_t)((s_o.hard[lr][j] & ~s_o.e[last][lr][j]) >> sh);
        }
        if constexpr (PX == 1) {
            const uint32_t g = grey[p], q = alpha256 * g;
            const uint32_t r = guide[3 * p], gg = guide[3 * p + 1], b = guide[3 * p + 2];
            const bool o = ol & 1u;
            const uint32_t vr = o ? tr : ov_tint(r, tr, q), vg = o ? tg : ov_tint(gg, tg, q), vb = o ? tb : ov_tint(b, tb, q);
            uint8_t* at = dst;
            if (panels > 1) {
                px_put<NT>(at, (uint8_t)r); px_put<NT>(at + 1, (uint8_t)gg); px_put<NT>(at + 2, (uint8_t)b);
                at += 3 * W;
            }
            px_put<NT>(at, (uint8_t)vr); px_put<NT>(at + 1, (uint8_t)vg); px_put<NT>(at + 2, (uint8_t)vb);
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

}  // namespace

extern "C" int cgs_overlay_compose(const uint8_t* guide, const uint8_t* grey, const uint8_t* hard, int32_t n, int32_t h, int32_t w,
                                   int32_t r, int32_t g, int32_t b, int32_t alpha256, int32_t thickness, int32_t layout, int32_t flags,
                                   uint8_t* out, cgs_stream_t stream_) {
    OvLaunch l;
    if (const int rc = ov_prepare(guide, grey, out, n, h, w, r, g, b, alpha256, thickness, layout, flags, false, &l)) return rc;
    ov_dispatch(guide, grey, out, w, flags, [&](auto px, auto nt) {
        hipLaunchKernelGGL((overlay_kernel<decltype(px)::value, decltype(nt)::value>), l.grid, dim3(OV_THREADS), 0, (hipStream_t)stream_, guide,
                           grey, hard, (int)h, (int)w, l.tint, (uint32_t)alpha256, (int)thickness, (int)layout, out);
    });
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}
