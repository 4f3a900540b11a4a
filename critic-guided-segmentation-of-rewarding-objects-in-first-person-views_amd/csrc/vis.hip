// Frame composition of the -viscritic / -vismasker videos (Handler.visualize's make_video, main.py:818-874), one launch per chunk of
// frames of one video.
//
// A frame is [H, 256, 3] uint8, H = 4 (64 R + 64): R image tiles (the RGB frame; with R = 2 the frame times its mask under it), then
// the two plot strips (ground truth, prediction; 32 source rows each), every SOURCE row shown x4 nearest, then three labels blended
// over the finished pixels (include/cgs_hip.h).  An output row is 768 B = 48 x 16 B and four source pixels are 48 B = 3 pieces, so
// piece j = 3 g + s of a row is dwords 4 s .. 4 s + 3 of the 12-dword group g: it needs source pixels 4 g + s and 4 g + s + 1 only.
//
// Launch: one workgroup of 256 lanes per VIS_ROWS source rows of one frame.  A lane builds a 16-byte piece once and stores it to the
// four output rows that repeat it; where an output row crosses a label cell the lane blends the cell's coverage into its registers
// first, so every output byte is written exactly once.  The kernel is write-bound: per 64 bytes stored a lane reads two source pixels
// (6 B, and 8 B of mask in the masked tile) or, in a plot strip, two perm / row entries that stay in L1 / L2.
#include "pixel_common.h"

namespace {

constexpr int VIS_TILE = 64;                         // source tile side = columns of a plot strip
constexpr int VIS_SCALE = 4;                         // nearest upscale
constexpr int VIS_PLOT = 32;                         // source rows of a plot strip (ph)
constexpr int VIS_W = VIS_TILE * VIS_SCALE;          // 256 px
constexpr int VIS_PIECES = VIS_W * 3 / 16;           // 16-byte pieces per output row (48)
constexpr int VIS_ROWS = 16;                         // source rows per workgroup
constexpr int VIS_THREADS = 256;
constexpr int VIS_LABELS = 1 + CGS_VIS_VALUES;       // the index label, then one per value row: the order the reference draws them in

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// dword (4 s + i) of a group: bytes (m, m+1, m+2, m) mod 3 of the channels of one pixel c = R | G << 8 | B << 16, m = (4 s + i) % 3
__device__ __forceinline__ uint32_t rotated(uint32_t c, int m) {
    return m == 0 ? (c | (c << 24)) : (m == 1 ? ((c >> 8) | (c << 16)) : ((c >> 16) | (c << 8)));
}

// PIL's paste of white through the coverage a: ((v >> 8) + v) >> 8 with v = dst (255 - a) + 255 a + 128, per byte of the piece.
// `cell` is row (y - ly) of the label's 64-px atlas cell, lx the label's left edge; piece j holds bytes 16 j .. 16 j + 15 of the row,
// i.e. pixels x0 = 16 j / 3 .. x0 + 5.  Their six coverages are loaded first (independent loads; 0 outside the cell, which leaves the
// byte as it is), then the sixteen bytes are blended from registers.
__device__ __forceinline__ u32x4 blend(u32x4 v, const uint8_t* __restrict__ cell, int lx, int j) {
    const int x0 = 16 * j / 3, r = j % 3;                              // byte 16 j + m belongs to pixel x0 + (r + m) / 3
    uint64_t cover = 0;
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        const int cx = x0 + t - lx;
        const uint32_t a = (cx >= 0 && cx < CGS_VIS_CELL_W) ? cell[cx] : 0u;        // (x < 256 always: the frame edge clips the cell)
        cover |= (uint64_t)a << (8 * t);
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        uint32_t w = 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
            const uint32_t a = (uint32_t)(cover >> (8 * ((r + 4 * i + b) / 3))) & 0xFFu;
            const uint32_t d = (v[i] >> (8 * b)) & 0xFFu;
            const uint32_t t = d * (255u - a) + 255u * a + 128u;
            w |= (((t >> 8) + t) >> 8) << (8 * b);
        }
        v[i] = w;
    }
    return v;
}

template <bool NT>
__global__ void __launch_bounds__(VIS_THREADS)
vis_compose_kernel(const uint8_t* __restrict__ X, const float* __restrict__ masks, const int32_t* __restrict__ perm,
                   const uint8_t* __restrict__ rows, const int32_t* __restrict__ ids, const uint8_t* __restrict__ atlas, int n_labels,
                   int N, int R, int j0, u32x4* __restrict__ out) {
    const int S = VIS_TILE * R + VIS_PLOT * CGS_VIS_VALUES;            // source rows of a frame
    const int units = S / VIS_ROWS;
    const int f = blockIdx.x / units, unit = blockIdx.x - f * units;
    const int jf = j0 + f;                                             // position in the (sorted) video
    const int p = perm ? perm[jf] : jf;                                // source frame
    const int H = S * VIS_SCALE;
    u32x4* frame = out + (size_t)f * H * VIS_PIECES;
    // label cells: (x, y) of the reference's draw.text calls (main.py:857-862) and this frame's atlas cell, or null
    const int lx[VIS_LABELS] = {CGS_VIS_INDEX_X, CGS_VIS_VALUE_X, CGS_VIS_VALUE_X};
    const int ly[VIS_LABELS] = {H - 12 - VIS_SCALE * VIS_PLOT * CGS_VIS_VALUES - 1, CGS_VIS_VALUE_Y, CGS_VIS_VALUE_Y + CGS_VIS_VALUE_DY};
    const uint8_t* cell[VIS_LABELS];
#pragma unroll
    for (int l = 0; l < VIS_LABELS; ++l) {
        const int id = ids[(size_t)p * VIS_LABELS + l];
        cell[l] = (unsigned)id < (unsigned)n_labels ? atlas + (size_t)id * CGS_VIS_CELL_W * CGS_VIS_CELL_H : nullptr;
    }
    for (int i = threadIdx.x; i < VIS_ROWS * VIS_PIECES; i += VIS_THREADS) {
        const int srow = unit * VIS_ROWS + i / VIS_PIECES;
        const int j = i % VIS_PIECES;
        const int s = j % 3, px = j + j / 3;                           // pixels px, px + 1 of the source row
        uint32_t c0, c1;
        if (srow < VIS_TILE * R) {
            const int tile = srow / VIS_TILE, sy = srow % VIS_TILE;
            const size_t at = ((size_t)p * VIS_TILE + sy) * VIS_TILE + px;
            const uint8_t* q = X + at * 3;
            uint32_t b[6];
#pragma unroll
            for (int k = 0; k < 6; ++k) b[k] = q[k];
            if (tile == 1) {
                // uint8(float32(x) * m): one IEEE fp32 product (no FMA to contract into), truncated; m in [0, 1]
                const float m0 = masks[at], m1 = masks[at + 1];
#pragma unroll
                for (int k = 0; k < 6; ++k) {
                    const float v = __fmul_rn((float)b[k], k < 3 ? m0 : m1);
                    b[k] = (uint32_t)(int)fminf(fmaxf(v, 0.0f), 255.0f);
                }
            }
            c0 = b[0] | (b[1] << 8) | (b[2] << 16);
            c1 = b[3] | (b[4] << 8) | (b[5] << 16);
        } else {
            const int r = srow - VIS_TILE * R;
            const int v = r / VIS_PLOT, pr = r % VIS_PLOT;
            const uint8_t* rv = rows + (size_t)v * N;
            uint32_t c[2];
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int col = px + k, at = jf + col - VIS_TILE / 2;  // value index of this column
                bool on = false;
                if (at >= 0 && at < N) on = rv[perm ? perm[at] : at] == pr;
                c[k] = on ? (col == VIS_TILE / 2 ? 0x0000FFu : 0xFFFFFFu) : 0u;     // the current frame's column is red
            }
            c0 = c[0];
            c1 = c[1];
        }
        u32x4 piece;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int w = 4 * s + k;
            piece[k] = rotated(w / 3 == s ? c0 : c1, w % 3);
        }
        // labels: which cells this piece's pixels (16 j / 3 .. (16 j + 15) / 3) can touch
        const int x_lo = 16 * j / 3, x_hi = (16 * j + 15) / 3;
        bool touch[VIS_LABELS];
        bool any = false;
#pragma unroll
        for (int l = 0; l < VIS_LABELS; ++l) {
            touch[l] = cell[l] && x_hi >= lx[l] && x_lo < lx[l] + CGS_VIS_CELL_W && VIS_SCALE * srow + VIS_SCALE > ly[l] &&
                       VIS_SCALE * srow < ly[l] + CGS_VIS_CELL_H;
            any |= touch[l];
        }
        u32x4* dst = frame + (size_t)(VIS_SCALE * srow) * VIS_PIECES + j;
#pragma unroll
        for (int q = 0; q < VIS_SCALE; ++q) {
            u32x4 v = piece;
            if (any) {
                const int y = VIS_SCALE * srow + q;
#pragma unroll
                for (int l = 0; l < VIS_LABELS; ++l)
                    if (touch[l] && y >= ly[l] && y < ly[l] + CGS_VIS_CELL_H) v = blend(v, cell[l] + (y - ly[l]) * CGS_VIS_CELL_W, lx[l], j);
            }
            px_put<NT>(dst + q * VIS_PIECES, v);
        }
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int cgs_vis_compose(const uint8_t* X, const float* masks_or_null, const int32_t* perm_or_null, const uint8_t* rows,
                               const int32_t* label_ids, const uint8_t* atlas, int32_t n_labels, int32_t N, int32_t R, int32_t j0,
                               int32_t n, int32_t flags, uint8_t* out, cgs_stream_t stream) {
    if (!X || !rows || !label_ids || !atlas || n_labels < 1 || N < 1 || (R != 1 && R != 2) || (R == 2 && !masks_or_null) || j0 < 0 ||
        n < 1 || (int64_t)j0 + n > N || !out || !aligned16(out) || (flags & ~CGS_VIS_NONTEMPORAL))
        return CGS_ERR_BADARG;
    const int units = (VIS_TILE * R + VIS_PLOT * CGS_VIS_VALUES) / VIS_ROWS;
    if ((int64_t)n * units > 0x7FFFFFFF) return CGS_ERR_BADARG;
    const dim3 grid((unsigned)(n * units));
    const hipStream_t s = (hipStream_t)stream;
    u32x4* o = reinterpret_cast<u32x4*>(out);
    if (flags & CGS_VIS_NONTEMPORAL)
        hipLaunchKernelGGL(vis_compose_kernel<true>, grid, dim3(VIS_THREADS), 0, s, X, masks_or_null, perm_or_null, rows, label_ids, atlas,
                           n_labels, N, R, j0, o);
    else
        hipLaunchKernelGGL(vis_compose_kernel<false>, grid, dim3(VIS_THREADS), 0, s, X, masks_or_null, perm_or_null, rows, label_ids, atlas,
                           n_labels, N, R, j0, o);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}
