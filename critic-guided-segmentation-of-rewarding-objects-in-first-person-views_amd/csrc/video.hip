// Frame composition of the -test / --output-video evaluation video (main.py:1027-1087), one launch per chunk of frames.
//
// A frame is [H, W, 3] uint8: the title band (h_top rows), `rows` rows of `cols` cells, the legend band (h_bottom rows).  A cell is one
// 64 x 64 source tile shown x3 nearest (out[y][x] = tile[y/3][x/3]), so a cell row of an output row is 192 px = 576 B = 36 x 16 B and
// every 16-byte store lies inside one cell.  Cell pixel values are the reference's uint8(255 v) with v in float64 (include/cgs_hip.h).
//
// Launch: grid (units, frames), one workgroup per unit of one frame.  A unit is one band row (a 16-byte copy of the pre-rendered band
// row, which stays in L2) or one SOURCE row of a cell row: its lanes build each 16-byte piece once and store it to the three output
// rows it is repeated on.  Lane j owns 16-byte piece j of the output row, so every store instruction of a wave covers 1 KB contiguous.
// The kernel is write-bound: the source reads (3 pixels per lane, at most 8 B each) are about a tenth of the bytes written.
#include "pixel_common.h"

namespace {

constexpr int VTILE = 64;                       // source tile side
constexpr int VSCALE = 3;                       // nearest upscale
constexpr int VCELL_PIECES = VTILE * VSCALE * 3 / 16;     // 16-byte pieces per cell row of an output row (36)

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

struct VideoCells {
    cgs_video_cell c[CGS_VIDEO_MAX_CELLS];
};

__device__ __forceinline__ uint32_t quant(double v) {
    // uint8(255 v) of numpy: IEEE double product, truncation; inputs are in [0, 1] (clamped here, NaN -> 0)
    v = fmin(fmax(v, 0.0), 1.0);
    return (uint32_t)(int)(255.0 * v);
}

__device__ __forceinline__ uint32_t grey(uint32_t q) { return q | (q << 8) | (q << 16); }

// R | G << 8 | B << 16 of source pixel (f, sy, px) of cell d
__device__ __forceinline__ uint32_t cell_pixel(const cgs_video_cell& d, long pix) {
    if (d.mode == CGS_VIDEO_CONST) return grey(quant(d.value));
    if (d.kind == CGS_VIDEO_RGB8) {
        const uint8_t* s = static_cast<const uint8_t*>(d.src) + pix * 3;
        return (uint32_t)s[0] | ((uint32_t)s[1] << 8) | ((uint32_t)s[2] << 16);     // uint8(255 (x / 255)) == x for every byte
    }
    if (d.kind == CGS_VIDEO_MASK8) {
        const uint32_t m = static_cast<const uint8_t*>(d.src)[pix] != 0;
        if (d.mode == CGS_VIDEO_GREY) return m ? 0xFFFFFFu : 0u;
        // main.py:1050-1051 against the truth y: TP (0,1,0), FN (1,0,0), FP (.5,.5,.5) -> 127, TN black
        const uint32_t y = d.y[pix] != 0;
        return y ? (m ? 0x00FF00u : 0x0000FFu) : (m ? 0x7F7F7Fu : 0u);
    }
    if (d.kind == CGS_VIDEO_F32) return grey(quant((double)static_cast<const float*>(d.src)[pix]));
    return grey(quant(static_cast<const double*>(d.src)[pix]));
}

// bytes [r, r + 16) of the 27-byte run "c0 c0 c0 c1 c1 c1 c2 c2 c2" (three output pixels per source pixel), r in [0, 9)
__device__ __forceinline__ u32x4 piece(uint32_t c0, uint32_t c1, uint32_t c2, int r) {
    const uint32_t R0 = c0 & 0xFF, G0 = (c0 >> 8) & 0xFF, B0 = c0 >> 16;
    const uint32_t R1 = c1 & 0xFF, G1 = (c1 >> 8) & 0xFF, B1 = c1 >> 16;
    const uint32_t R2 = c2 & 0xFF, G2 = (c2 >> 8) & 0xFF, B2 = c2 >> 16;
    uint32_t P[7];
    P[0] = R0 | G0 << 8 | B0 << 16 | R0 << 24;
    P[1] = G0 | B0 << 8 | R0 << 16 | G0 << 24;
    P[2] = B0 | R1 << 8 | G1 << 16 | B1 << 24;
    P[3] = R1 | G1 << 8 | B1 << 16 | R1 << 24;
    P[4] = G1 | B1 << 8 | R2 << 16 | G2 << 24;
    P[5] = B2 | R2 << 8 | G2 << 16 | B2 << 24;
    P[6] = R2 | G2 << 8 | B2 << 16;
    const int a = r >> 2, sh = (r & 3) * 8;
    u32x4 out;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t lo = a == 0 ? P[i] : (a == 1 ? P[i + 1] : P[i + 2]);
        const uint32_t hi = a == 0 ? P[i + 1] : (a == 1 ? P[i + 2] : P[i + 3]);
        out[i] = (uint32_t)(((((uint64_t)hi) << 32) | lo) >> sh);
    }
    return out;
}

template <bool NT>
__global__ void video_compose_kernel(VideoCells cells, int cols, int cell_rows, int f0, int h_top, int h_bottom, const u32x4* __restrict__ top,
                                     const u32x4* __restrict__ bottom, u32x4* __restrict__ out) {
    const int rp = cols * VCELL_PIECES;                          // pieces per output row
    const int H = h_top + cell_rows * VTILE * VSCALE + h_bottom;
    const int unit = blockIdx.x;
    u32x4* frame = out + (size_t)blockIdx.y * H * rp;
    if (unit < h_top) {
        for (int j = threadIdx.x; j < rp; j += blockDim.x) px_put<NT>(frame + (size_t)unit * rp + j, top[(size_t)unit * rp + j]);
        return;
    }
    const int u = unit - h_top;
    if (u >= cell_rows * VTILE) {
        const int b = u - cell_rows * VTILE;
        u32x4* dst = frame + (size_t)(h_top + cell_rows * VTILE * VSCALE + b) * rp;
        for (int j = threadIdx.x; j < rp; j += blockDim.x) px_put<NT>(dst + j, bottom[(size_t)b * rp + j]);
        return;
    }
    const int cr = u / VTILE, sy = u % VTILE;
    const long row_pix = ((long)(f0 + blockIdx.y) * VTILE + sy) * VTILE;      // first source pixel of this row in a [n,64,64] stack
    u32x4* dst = frame + (size_t)(h_top + cr * VTILE * VSCALE + sy * VSCALE) * rp;
    for (int j = threadIdx.x; j < rp; j += blockDim.x) {
        const int col = j / VCELL_PIECES;
        const int b = (j - col * VCELL_PIECES) * 16;             // byte offset in the cell row
        const int p0 = b / 9;                                    // 9 bytes per source pixel
        const cgs_video_cell& d = cells.c[cr * cols + col];
        const uint32_t c0 = cell_pixel(d, row_pix + p0);
        const uint32_t c1 = cell_pixel(d, row_pix + p0 + 1);
        const uint32_t c2 = p0 + 2 < VTILE ? cell_pixel(d, row_pix + p0 + 2) : 0u;    // (the last piece of a cell needs two pixels)
        const u32x4 v = piece(c0, c1, c2, b - 9 * p0);
        px_put<NT>(dst + j, v);
        px_put<NT>(dst + rp + j, v);
        px_put<NT>(dst + 2 * rp + j, v);
    }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int cgs_video_compose(const cgs_video_cell* cells, int32_t rows, int32_t cols, int32_t f0, int32_t n, const uint8_t* top,
                                 int32_t h_top, const uint8_t* bottom, int32_t h_bottom, int32_t flags, uint8_t* out, cgs_stream_t stream) {
    if (!cells || rows < 1 || cols < 1 || rows * cols > CGS_VIDEO_MAX_CELLS || f0 < 0 || n < 1 || n > 65535 || h_top < 0 ||
        h_bottom < 0 || (h_top && !top) || (h_bottom && !bottom) || !out || (flags & ~CGS_VIDEO_NONTEMPORAL))
        return CGS_ERR_BADARG;
    if (!aligned16(out) || (h_top && !aligned16(top)) || (h_bottom && !aligned16(bottom))) return CGS_ERR_BADARG;
    VideoCells vc = {};
    for (int i = 0; i < rows * cols; ++i) {
        const cgs_video_cell& d = cells[i];
        if (d.mode == CGS_VIDEO_CONST) {
            vc.c[i] = d;
            continue;
        }
        if (!d.src || d.kind < CGS_VIDEO_RGB8 || d.kind > CGS_VIDEO_F64) return CGS_ERR_BADARG;
        if (d.mode == CGS_VIDEO_CODE) {
            if (d.kind != CGS_VIDEO_MASK8 || !d.y) return CGS_ERR_BADARG;
        } else if (d.mode != CGS_VIDEO_GREY) {
            return CGS_ERR_BADARG;
        }
        vc.c[i] = d;
    }
    const int rp = cols * VCELL_PIECES;
    const int threads = rp >= 1024 ? 1024 : (rp + 63) / 64 * 64;
    const dim3 grid((unsigned)(h_top + rows * VTILE + h_bottom), (unsigned)n);
    const hipStream_t s = (hipStream_t)stream;
    const u32x4* t = reinterpret_cast<const u32x4*>(top);
    const u32x4* bt = reinterpret_cast<const u32x4*>(bottom);
    u32x4* o = reinterpret_cast<u32x4*>(out);
    if (flags & CGS_VIDEO_NONTEMPORAL)
        hipLaunchKernelGGL(video_compose_kernel<true>, grid, dim3(threads), 0, s, vc, cols, rows, f0, h_top, h_bottom, t, bt, o);
    else
        hipLaunchKernelGGL(video_compose_kernel<false>, grid, dim3(threads), 0, s, vc, cols, rows, f0, h_top, h_bottom, t, bt, o);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}
