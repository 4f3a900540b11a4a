// Smoothing of a stack of 64 x 64 masks along time for -process --source-video --smooth (include/cgs_hip.h): cgs_temporal_smooth, a
// spatio-temporal joint bilateral filter guided by the shrunk frames.  The network has no memory, so its masks flicker when they are played
// as a video; this filter averages a cell with the cells of the frames around it whose colour is still the cell's colour.
//
// For output frame f and cell p the taps are, in this order (the order of the two fp32 sums):
//   k = 0                       the centre tap (f, p) alone, weight exactly 1: num = z[f][p], den = 1
//   k = -radius .. -1, 1 .. radius (ascending), frame g = f + k, skipped when g is outside [0, n)
//     dy = -1, 0, 1 (outer), dx = -1, 0, 1 (inner): cell p + (dy, dx) of frame g, skipped when it is outside the grid
//       w = exp2(-(d2 cr + k^2 ct + (dy^2 + dx^2) cs)),  num = fma(w, z[g][p + (dy, dx)], num),  den = den + w
// with cr = log2(e) / (2 sigma_r^2), ct = log2(e) / (2 sigma_t^2), sigma_t = radius / 2, cs = log2(e) / 2 (a spatial sigma of one cell) and
// d2 the squared colour distance of low[g][p + (dy, dx)] and low[f][p], an integer (<= 195075, exact in fp32) formed before anything is
// rounded.  One hardware exponential per tap.  out = num / den is the IEEE division.  den >= 1, so no minimum has to be subtracted;
// 0 <= z <= 1 keeps num <= den at every step, so 0 <= out <= 1, and a stack that is 1 wherever a weight is non-zero gives num == den and
// out == 1.0f exactly.  Motion is not compensated: the 3 x 3 search and the range term stand in for a motion model.
//
// One workgroup per output frame, 256 threads x 16 cells (thread t owns column t & 63 of rows t / 64 + 4 j), num and den in registers.
// The frames g are walked one at a time: the frame's packed colour and its z go to LDS as 66 x 66 planes, the one-cell apron left at
// colour 0 and z 0; a tap on the apron gets the exponent +inf from its row or column term, so its weight is exp2(-inf) = +0 exactly and it
// adds +0 to both sums: skipped, not clamped, without a bounds test on the reads.  A frame is 28 KB (12 KB of colour, 16 KB of z) and is
// read by 2 radius + 1 workgroups that run at about the same time, so the repeats come out of L2.  No atomics, no allocation.
#include "temporal_body.h"

namespace {

constexpr int TS_THREADS = 256;
constexpr int TS_SIDE = 64;
constexpr int TS_CELLS = TS_SIDE * TS_SIDE / TS_THREADS;      // 16 cells a thread
constexpr int TS_PITCH = TS_SIDE + 2;                         // a plane with its apron
static_assert(CGS_TEMPORAL_SIDE == TS_SIDE && TS_THREADS == 4 * TS_SIDE, "temporal layout");

__global__ void __launch_bounds__(TS_THREADS)
temporal_smooth_kernel(const float* __restrict__ z, const uint8_t* __restrict__ low, int n, int f0, int radius, float cr, float ct, float cs,
                       float* __restrict__ out) {
    __shared__ uint32_t s_c[TS_PITCH * TS_PITCH];             // r | g << 8 | b << 16, apron 0
    __shared__ float s_z[TS_PITCH * TS_PITCH];                // apron 0
    const int t = threadIdx.x, col = t & (TS_SIDE - 1), row0 = t >> 6;
    const int f = f0 + (int)blockIdx.x;
    const float inf = __builtin_inff();

    for (int i = t; i < TS_PITCH * TS_PITCH; i += TS_THREADS) {
        s_c[i] = 0u;
        s_z[i] = 0.0f;
    }

    // the centre tap: weight exactly 1
    uint32_t c0[TS_CELLS], cc[TS_CELLS];
    float num[TS_CELLS], den[TS_CELLS];
#pragma unroll
    for (int j = 0; j < TS_CELLS; ++j) {
        const int64_t cell = ((int64_t)f * TS_SIDE + (row0 + 4 * j)) * TS_SIDE + col;
        c0[j] = px_colour(low, cell);
        cc[j] = px_dot3(c0[j], c0[j]);
        num[j] = z[cell];
        den[j] = 1.0f;
    }
    // the column term of the exponent is the same for every cell of the thread
    float ex[3];
#pragma unroll
    for (int dx = 0; dx < 3; ++dx) {
        const int x = col + dx - 1;
        ex[dx] = (x >= 0 && x < TS_SIDE) ? (dx == 1 ? 0.0f : cs) : inf;
    }

    for (int k = -radius; k <= radius; ++k) {
        const int g = f + k;
        if (k == 0 || g < 0 || g >= n) continue;              // (the same in every thread) a frame outside the stack is skipped
        __syncthreads();                                      // the frame before is read to its end (and, the first time, the apron is set)
#pragma unroll
        for (int j = 0; j < TS_CELLS; ++j) {
            const int r = row0 + 4 * j;
            const int64_t cell = ((int64_t)g * TS_SIDE + r) * TS_SIDE + col;
            s_c[(r + 1) * TS_PITCH + col + 1] = px_colour(low, cell);
            s_z[(r + 1) * TS_PITCH + col + 1] = z[cell];
        }
        __syncthreads();
        const float kk = (float)(k * k);
#pragma unroll
        for (int j = 0; j < TS_CELLS; ++j) {
            const int r = row0 + 4 * j;
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
                const int y = r + dy - 1;
                const float ey = (y >= 0 && y < TS_SIDE) ? (dy == 1 ? 0.0f : cs) : inf;
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int at = (r + dy) * TS_PITCH + col + dx;
                    ts_tap(cc[j], c0[j], s_c[at], s_z[at], cr, kk, ct, ey + ex[dx], num[j], den[j]);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < TS_CELLS; ++j)
        out[((int64_t)blockIdx.x * TS_SIDE + (row0 + 4 * j)) * TS_SIDE + col] = num[j] / den[j];
}

}  // namespace

extern "C" int cgs_temporal_smooth(const float* z, const uint8_t* low, int32_t n, int32_t f0, int32_t f1, int32_t radius, float sigma_r,
                                   float* out, cgs_stream_t stream_) {
    TsCoef c;
    if (const int rc = ts_prepare(z, low, out, n, f0, f1, radius, sigma_r, false, &c)) return rc;
    hipLaunchKernelGGL(temporal_smooth_kernel, dim3((unsigned)(f1 - f0)), dim3(TS_THREADS), 0, (hipStream_t)stream_, z, low, (int)n, (int)f0,
                       (int)radius, c.cr, c.ct, c.cs, out);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}
