// Block-matched motion for the temporal mask filter of -process --source-video --smooth R --smooth-motion S (include/cgs_hip.h):
// cgs_temporal_flow estimates one integer vector per 8 x 8-cell block between neighbouring shrunk frames, cgs_temporal_smooth_mc is
// cgs_temporal_smooth (csrc/temporal.hip) with the 3 x 3 taps of frame f + k centred where the chain of those vectors carries the cell.
// What is compensated: a translation of whole cells, up to S cells a frame, constant over a block.  What is not: motion inside a block,
// motion of a fraction of a cell, and occlusion -- there the range term is what is left, as before.
//
// cgs_temporal_flow.  For frame pair g, block (by, bx) and direction fwd (frame g -> g + 1; bwd: g + 1 -> g) the answer is the candidate
// d = (dy, dx), |dy|, |dx| <= S, the displaced block wholly inside the grid, with the smallest SAD(d) = sum over the 64 cells q of the block
// and the three colours of |src[q][c] - dst[q + d][c]|; equal SADs go to the candidate that comes first by (dy^2 + dx^2, dy, dx).  SAD <=
// 64 * 765 = 48960 < 2^16 and the rank < 81 < 2^7, so SAD << 7 | rank is one uint32 key whose minimum is the answer.  The rank is the
// candidate's place in that order among all 81 candidates of S = 4: the candidates of a smaller S are a subset of them, in the same order.
// One workgroup per frame pair, both directions: the two frames' packed colours in LDS (32 KB); thread t owns direction t >> 7, block
// (t >> 1) & 63 and every second candidate (t & 1), its block's 64 source cells in registers, one v_sad_u8 per cell and candidate; the
// two threads of a block meet through one lane exchange.  No atomics, no allocation; a vector depends on its two frames only.
//
// cgs_temporal_smooth_mc.  The path of cell p of frame f: m_0 = 0, m_{j+1} = m_j + fwd[f + j][block of clamp(p + m_j)] (bwd[f - j - 1] for
// k < 0); the taps of frame f + k are the 3 x 3 cells p + m_k + (dy, dx), skipped when outside the grid.  Everything else -- weights, the
// integer d2 against low[f][p], the spatial term on (dy, dx) alone, the tap order, the two fp32 sums, the exponential, the division -- is
// temporal_smooth_kernel's: the tap itself is the one function both call (ts_tap, csrc/temporal_body.h), so that an all-zero field gives its
// output bit for bit.  The tables of the 2 radius
// frame pairs around f go to LDS (2 KB); a forward path is carried from k to k + 1, a backward path (k runs -radius .. -1) is walked
// again from p for each k: |k| dependent reads of an 8 x 8 table.  A tap centre can lie anywhere, so every address is bounded: the table
// is read at the clamped cell, and the centre's row and column are clamped to -2 .. 65 on planes of 70 x 70 with an apron of three cells
// (colour 0, z 0).  A centre at -2 or beyond has all three of its taps outside the grid either way and a centre inside -1 .. 64 is not
// moved, so the clamp changes no tap that counts; the taps are then nine fixed offsets from one address, and one on the apron has the
// exponent +inf and the weight +0 exactly, as in temporal_smooth_kernel.  For any int8 content of the fields |m| <= 8 * 128.
#include "temporal_body.h"

namespace {

constexpr int TM_THREADS = 256;
constexpr int TM_SIDE = 64;
constexpr int TM_BLOCK = CGS_TEMPORAL_BLOCK;                  // cells a side of a block
constexpr int TM_BLOCKS = TM_SIDE / TM_BLOCK;                 // 8 blocks a side
constexpr int TM_SPAN = 2 * CGS_TEMPORAL_MAX_SEARCH + 1;      // 9 candidates a side
constexpr int TM_CAND = TM_SPAN * TM_SPAN;                    // 81
constexpr int TM_CELLS = TM_SIDE * TM_SIDE / TM_THREADS;      // 16 cells a thread
constexpr int TM_APRON = 3;                                   // cells of apron: a clamped centre at -2 or 65 has its taps at -3 .. 66
constexpr int TM_PITCH = TM_SIDE + 2 * TM_APRON;              // a plane with its apron
static_assert(CGS_TEMPORAL_SIDE == TM_SIDE && TM_THREADS == 4 * TM_SIDE && TM_BLOCK == 8 && TM_BLOCKS * TM_BLOCKS == 64, "temporal layout");
static_assert(TM_CAND <= 128 && 64 * 765 < (1 << 16), "the key is SAD << 7 | rank");
static_assert(TM_THREADS == 2 * 2 * TM_BLOCKS * TM_BLOCKS, "two threads per direction and block");

__device__ __forceinline__ uint32_t tm_sad3(uint32_t a, uint32_t b, uint32_t acc) {     // acc + sum of |a_c - b_c| over the bytes
#if __has_builtin(__builtin_amdgcn_sad_u8)
    return __builtin_amdgcn_sad_u8(a, b, acc);
#else
    for (int c = 0; c < 24; c += 8) {
        const int x = (int)((a >> c) & 255u) - (int)((b >> c) & 255u);
        acc += (uint32_t)(x < 0 ? -x : x);
    }
    return acc;
#endif
}

__device__ __forceinline__ int tm_clamp(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

// ---------------------------------------------------------------------------------------------------------------- the block motion
__global__ void __launch_bounds__(TM_THREADS)
temporal_flow_kernel(const uint8_t* __restrict__ low, int search, int8_t* __restrict__ fwd, int8_t* __restrict__ bwd) {
    __shared__ uint32_t s_c[2][TM_SIDE * TM_SIDE];            // frames g and g + 1, r | g << 8 | b << 16
    __shared__ uint8_t s_rank[TM_CAND], s_cand[TM_CAND];      // candidate (dy + 4) * 9 + dx + 4 -> its rank, and back
    const int t = threadIdx.x;
    const int64_t g = blockIdx.x;

    for (int i = t; i < 2 * TM_SIDE * TM_SIDE; i += TM_THREADS) s_c[0][i] = px_colour(low, g * TM_SIDE * TM_SIDE + i);
    if (t < TM_CAND) {
        // the order (dy^2 + dx^2, dy, dx) as one integer; the rank is the number of candidates in front
        auto order = [](int c) {
            const int dy = c / TM_SPAN - CGS_TEMPORAL_MAX_SEARCH, dx = c % TM_SPAN - CGS_TEMPORAL_MAX_SEARCH;
            return (dy * dy + dx * dx) * TM_CAND + c;
        };
        const int mine = order(t);
        int rank = 0;
        for (int c = 0; c < TM_CAND; ++c) rank += order(c) < mine ? 1 : 0;
        s_rank[t] = (uint8_t)rank;
        s_cand[rank] = (uint8_t)t;
    }
    __syncthreads();

    const int dir = t >> 7, block = (t >> 1) & 63, half = t & 1;
    const int y0 = (block >> 3) * TM_BLOCK, x0 = (block & 7) * TM_BLOCK;
    const uint32_t* src = s_c[dir];                           // fwd: frame g is the source, g + 1 is searched; bwd: the other way round
    const uint32_t* dst = s_c[dir ^ 1];
    uint32_t own[TM_BLOCK * TM_BLOCK];
#pragma unroll
    for (int i = 0; i < TM_BLOCK * TM_BLOCK; ++i) own[i] = src[(y0 + (i >> 3)) * TM_SIDE + x0 + (i & 7)];

    uint32_t best = 0xffffffffu;
    for (int c = half; c < TM_CAND; c += 2) {
        const int dy = c / TM_SPAN - CGS_TEMPORAL_MAX_SEARCH, dx = c % TM_SPAN - CGS_TEMPORAL_MAX_SEARCH;
        const int y = y0 + dy, x = x0 + dx;
        if (dy < -search || dy > search || dx < -search || dx > search || y < 0 || y + TM_BLOCK > TM_SIDE || x < 0 || x + TM_BLOCK > TM_SIDE)
            continue;                                         // the displaced block lies inside the grid: every read below is inside dst
        uint32_t sad = 0;
#pragma unroll
        for (int i = 0; i < TM_BLOCK * TM_BLOCK; ++i) sad = tm_sad3(own[i], dst[(y + (i >> 3)) * TM_SIDE + x + (i & 7)], sad);
        const uint32_t key = (sad << 7) | s_rank[c];
        best = key < best ? key : best;
    }
    const uint32_t other = (uint32_t)__shfl_xor((int)best, 1, 64);      // (0, 0) is always valid and has an even index: a key exists
    best = other < best ? other : best;
    if (half == 0) {
        const int c = s_cand[best & 127u];
        int8_t* out = (dir ? bwd : fwd) + (g * (TM_BLOCKS * TM_BLOCKS) + block) * 2;
        out[0] = (int8_t)(c / TM_SPAN - CGS_TEMPORAL_MAX_SEARCH);
        out[1] = (int8_t)(c % TM_SPAN - CGS_TEMPORAL_MAX_SEARCH);
    }
}

// ---------------------------------------------------------------------------------------------------------------- the filter along it
// One step of a path: the vector of the block that holds the cell (r + my, col + mx), clamped into the grid.
__device__ __forceinline__ void tm_step(const uint16_t* __restrict__ table, int r, int col, int& my, int& mx) {
    const int qy = tm_clamp(r + my, 0, TM_SIDE - 1), qx = tm_clamp(col + mx, 0, TM_SIDE - 1);
    const uint32_t v = table[(qy >> 3) * TM_BLOCKS + (qx >> 3)];
    my += (int)(int8_t)(v & 255u);
    mx += (int)(int8_t)(v >> 8);
}

__global__ void __launch_bounds__(TM_THREADS)
temporal_smooth_mc_kernel(const float* __restrict__ z, const uint8_t* __restrict__ low, const int8_t* __restrict__ fwd,
                          const int8_t* __restrict__ bwd, int n, int f0, int radius, float cr, float ct, float cs, float* __restrict__ out) {
    __shared__ uint32_t s_c[TM_PITCH * TM_PITCH];             // r | g << 8 | b << 16, apron 0
    __shared__ float s_z[TM_PITCH * TM_PITCH];                // apron 0
    __shared__ uint16_t s_m[2][CGS_TEMPORAL_MAX_RADIUS][TM_BLOCKS * TM_BLOCKS];      // [0][j] = fwd[f + j], [1][j] = bwd[f - j - 1]: dy | dx << 8
    const int t = threadIdx.x, col = t & (TM_SIDE - 1), row0 = t >> 6;
    const int f = f0 + (int)blockIdx.x;
    const float inf = __builtin_inff();

    for (int i = t; i < TM_PITCH * TM_PITCH; i += TM_THREADS) {
        s_c[i] = 0u;
        s_z[i] = 0.0f;
    }
    for (int i = t; i < 2 * radius * TM_BLOCKS * TM_BLOCKS; i += TM_THREADS) {
        const int b = i & 63, j = (i >> 6) % radius, dir = (i >> 6) / radius;
        const int pair = dir ? f - j - 1 : f + j;             // the pair (pair, pair + 1) of the stack; outside it the table is never read
        uint32_t v = 0u;
        if (pair >= 0 && pair + 1 < n) {
            const int8_t* m = (dir ? bwd : fwd) + ((int64_t)pair * (TM_BLOCKS * TM_BLOCKS) + b) * 2;
            v = (uint32_t)(uint8_t)m[0] | ((uint32_t)(uint8_t)m[1] << 8);
        }
        s_m[dir][j][b] = (uint16_t)v;
    }

    // the centre tap: weight exactly 1
    uint32_t c0[TM_CELLS], cc[TM_CELLS];
    float num[TM_CELLS], den[TM_CELLS];
    int fy[TM_CELLS], fx[TM_CELLS];                           // the forward path, carried from k to k + 1
#pragma unroll
    for (int j = 0; j < TM_CELLS; ++j) {
        const int64_t cell = ((int64_t)f * TM_SIDE + (row0 + 4 * j)) * TM_SIDE + col;
        c0[j] = px_colour(low, cell);
        cc[j] = px_dot3(c0[j], c0[j]);
        num[j] = z[cell];
        den[j] = 1.0f;
        fy[j] = 0;
        fx[j] = 0;
    }

    for (int k = -radius; k <= radius; ++k) {
        const int g = f + k;
        if (k == 0 || g < 0 || g >= n) continue;              // (the same in every thread) a frame outside the stack is skipped
        __syncthreads();                                      // the frame before is read to its end (and, the first time, the apron and the tables are set)
#pragma unroll
        for (int j = 0; j < TM_CELLS; ++j) {
            const int r = row0 + 4 * j;
            const int64_t cell = ((int64_t)g * TM_SIDE + r) * TM_SIDE + col;
            s_c[(r + TM_APRON) * TM_PITCH + col + TM_APRON] = px_colour(low, cell);
            s_z[(r + TM_APRON) * TM_PITCH + col + TM_APRON] = z[cell];
        }
        __syncthreads();
        const float kk = (float)(k * k);
#pragma unroll
        for (int j = 0; j < TM_CELLS; ++j) {
            const int r = row0 + 4 * j;
            int my = 0, mx = 0;
            if (k > 0) {                                      // frames f + 1 .. f + k all exist: the steps 0 .. k - 1 were or are taken here
                tm_step(s_m[0][k - 1], r, col, fy[j], fx[j]);
                my = fy[j];
                mx = fx[j];
            } else {
                for (int i = 0; i < -k; ++i) tm_step(s_m[1][i], r, col, my, mx);
            }
            // the centre p + m_k, clamped to within two cells of the grid, and the row and column terms of the exponent of its 3 x 3 taps
            const int cy = tm_clamp(r + my, -2, TM_SIDE + 1), cx = tm_clamp(col + mx, -2, TM_SIDE + 1);
            const int centre = (cy + TM_APRON) * TM_PITCH + cx + TM_APRON;
            float ey[3], ex[3];
#pragma unroll
            for (int d = 0; d < 3; ++d) {
                const int y = cy + d - 1, x = cx + d - 1;
                ey[d] = (y >= 0 && y < TM_SIDE) ? (d == 1 ? 0.0f : cs) : inf;
                ex[d] = (x >= 0 && x < TM_SIDE) ? (d == 1 ? 0.0f : cs) : inf;
            }
#pragma unroll
            for (int dy = 0; dy < 3; ++dy) {
#pragma unroll
                for (int dx = 0; dx < 3; ++dx) {
                    const int at = centre + (dy - 1) * TM_PITCH + dx - 1;
                    ts_tap(cc[j], c0[j], s_c[at], s_z[at], cr, kk, ct, ey[dy] + ex[dx], num[j], den[j]);
                }
            }
        }
    }
#pragma unroll
    for (int j = 0; j < TM_CELLS; ++j)
        out[((int64_t)blockIdx.x * TM_SIDE + (row0 + 4 * j)) * TM_SIDE + col] = num[j] / den[j];
}

}  // namespace

extern "C" int cgs_temporal_flow(const uint8_t* low, int32_t n, int32_t search, int8_t* fwd, int8_t* bwd, cgs_stream_t stream_) {
    if (!low || !fwd || !bwd || n < 2 || search < 1) return CGS_ERR_BADARG;
    if (search > CGS_TEMPORAL_MAX_SEARCH) return CGS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(temporal_flow_kernel, dim3((unsigned)(n - 1)), dim3(TM_THREADS), 0, (hipStream_t)stream_, low, (int)search, fwd, bwd);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}

extern "C" int cgs_temporal_smooth_mc(const float* z, const uint8_t* low, const int8_t* fwd, const int8_t* bwd, int32_t n, int32_t f0,
                                      int32_t f1, int32_t radius, float sigma_r, float* out, cgs_stream_t stream_) {
    TsCoef c;
    if (const int rc = ts_prepare(z, low, out, n, f0, f1, radius, sigma_r, n > 1 && (!fwd || !bwd), &c)) return rc;
    hipLaunchKernelGGL(temporal_smooth_mc_kernel, dim3((unsigned)(f1 - f0)), dim3(TM_THREADS), 0, (hipStream_t)stream_, z, low, fwd, bwd,
                       (int)n, (int)f0, (int)radius, c.cr, c.ct, c.cs, out);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}
