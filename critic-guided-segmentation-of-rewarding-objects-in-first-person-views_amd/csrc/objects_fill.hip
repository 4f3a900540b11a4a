// The masks that a bridged track misses (cgs_objects_track_fill, include/cgs_hip.h): for every frame m that a link of gap >= 2 jumps
// over, the link's tail object is carried from its frame a = m - j to m along the chain of backward block vectors the link was decided
// on (cgs_objects_track_mc's path), and the cells it lands on that hold no object of frame m become a new object of that frame.
// Everything is integer; the only global atomics are the four integer adds of `totals`, so nothing depends on an order.
//
// One workgroup, one frame m, 256 lanes: lane (wave, x) owns the 16 cells (wave + 4 r, x), kept in registers from the first read to
// the last write.
//   span    the words S(m, j), j = 1..G: one LDS atomic OR per entry of gap / prev of the frames m + 1 .. m + G that names a tail in
//           frame m - j.  No word set (most frames): the frame is copied and the workgroup is done.
//   stage   (with a field) frame m - j for every j with S(m, j) != 0, a byte per cell, already masked by S(m, j): a staged cell is
//           non-zero exactly when it can claim; and the J vector tables bwd[m - 1] .. bwd[m - J], J the largest such j.
//   walk    all 16 cells of a lane side by side through the J steps (track_level_kernel<true>'s walk): after step j the staged frame
//           m - j is read where the walk stands, and the first j that finds a label there claims the cell.  Without a field the walk
//           stands still and frame m - j is read from memory where the cell is.  Pure selection: no atomic decides a pixel.
//   rank    the candidates (j, p) that claimed a cell are a 512-bit map (one LDS OR per run of equal claims in a row); a candidate's
//           rank in (j, p) order is a popcount below its bit, its label base + rank + 1, dropped above K.
//   table   cgs_objects_label's row of every new object with LDS integer atomics, one set per run of a row.
// cgs_objects_track_fill_window gives a workgroup to the frames f0 <= m < f1 only and writes their outputs at m - f0: what a stream
// needs, whose window holds halo frames on both sides (objects.FillStream).  The reads are those of the whole stack's frame m.
// Every read is bounded for any content of the inputs: an entry of gap / prev is used only inside its range, a staged label is a
// byte in 0..K, the table index of a step comes from a clamped cell, the staged cell is checked, |m_j| <= 8 * 128.
#include "pixel_common.h"

namespace {

constexpr int OF_THREADS = 256;
constexpr int OF_WAVES = OF_THREADS / CGS_WAVE;
constexpr int OF_MAX_K = CGS_OBJ_MATCH_MAX_OBJECTS;
constexpr int OF_SIDE = CGS_OBJ_MAX_SIDE;
constexpr int OF_BLOCKS = OF_SIDE / CGS_TEMPORAL_BLOCK;
constexpr int OF_MAX_GAP = CGS_OBJ_TRACK_MAX_GAP;
constexpr int OF_ROWS = OF_SIDE / OF_WAVES;             // rows of a frame per lane
constexpr int OF_BIG = 0x7fffffff;
static_assert(OF_MAX_K == CGS_WAVE && OF_SIDE == CGS_WAVE && OF_SIDE == CGS_TEMPORAL_SIDE && CGS_TEMPORAL_BLOCK == 8,
              "a row and a frame's objects are one wave-wide word each, a block is 8 cells");
static_assert(OF_MAX_K < 256 && OF_MAX_GAP * OF_MAX_K == 2 * OF_THREADS && CGS_OBJ_FIELDS == 8, "a staged label is a byte");

__device__ __forceinline__ unsigned long long wave_or(unsigned long long v) {
    uint32_t lo = (uint32_t)v, hi = (uint32_t)(v >> 32);
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        lo |= (uint32_t)__shfl_xor((int)lo, m, CGS_WAVE);
        hi |= (uint32_t)__shfl_xor((int)hi, m, CGS_WAVE);
    }
    return (unsigned long long)lo | ((unsigned long long)hi << 32);
}

template <bool MC>
__global__ void __launch_bounds__(OF_THREADS)
fill_kernel(const int32_t* __restrict__ labels, const int8_t* __restrict__ bwd, int n, int h, int w, int K, int G,
            const int32_t* __restrict__ prev, const int32_t* __restrict__ gap, const int32_t* __restrict__ track,
            int32_t* __restrict__ out_labels, int32_t* __restrict__ out_track, int32_t* __restrict__ age, int32_t* __restrict__ table,
            int32_t* __restrict__ totals, int f0) {
    __shared__ unsigned long long s_S[OF_MAX_GAP];                       // [j - 1]: the tails in frame m - j of links that jump over m
    __shared__ unsigned long long s_C[OF_MAX_GAP];                       // [j - 1]: those of them that claimed a cell
    __shared__ unsigned long long s_pres[OF_WAVES];
    __shared__ int s_max[OF_WAVES];
    __shared__ int s_tab[OF_MAX_K * CGS_OBJ_FIELDS];
    __shared__ uint8_t s_L[MC ? OF_MAX_GAP : 1][OF_SIDE * OF_SIDE];      // MC: [j - 1] = frame m - j, masked by S(m, j)
    __shared__ uint16_t s_m[MC ? OF_MAX_GAP : 1][OF_BLOCKS * OF_BLOCKS];  // MC: [s] = bwd[m - s - 1], dy | dx << 8
    const int m = f0 + (int)blockIdx.x, tid = threadIdx.x, x = tid & (CGS_WAVE - 1), wave = tid / CGS_WAVE;
    const bool live = x < w;
    const int64_t hw = (int64_t)h * w, fm = (int64_t)m * hw, rowK = (int64_t)m * K;
    const int64_t fo = (int64_t)blockIdx.x * hw, rowO = (int64_t)blockIdx.x * K;    // the outputs hold the frames f0 .. only

    if (tid < OF_MAX_GAP) s_S[tid] = s_C[tid] = 0ull;
    for (int i = tid; i < OF_MAX_K * CGS_OBJ_FIELDS; i += OF_THREADS) {
        const int c = i & 7;
        s_tab[i] = (c == 1 || c == 2 || c == 7) ? OF_BIG : (c == 3 || c == 4) ? -1 : 0;
    }
    int own[OF_ROWS];                                                    // the lane's cells of frame m; 0 outside the frame
#pragma unroll
    for (int r = 0; r < OF_ROWS; ++r) {
        const int y = wave + OF_WAVES * r;
        own[r] = (live && y < h) ? labels[fm + (int64_t)y * w + x] : 0;
    }
    __syncthreads();
    for (int i = tid; i < G * K; i += OF_THREADS) {                      // entry l of frame f = m + d
        const int d = i / K + 1, l = i - (d - 1) * K;
        const int64_t f = (int64_t)m + d;
        if (f < n) {
            const int g = gap[f * K + l], p = prev[f * K + l];
            if (g > d && g <= G + 1 && g <= f && p >= 1 && p <= K) atomicOr(&s_S[g - d - 1], 1ull << (p - 1));     // j = g - d in 1..min(G, m)
        }
    }
    unsigned long long pres = 0ull;
    int top = 0;
#pragma unroll
    for (int r = 0; r < OF_ROWS; ++r) {
        top = max(top, own[r]);
        if (own[r] >= 1 && own[r] <= K) pres |= 1ull << (own[r] - 1);
    }
    top = px_wave_max(top);
    pres = wave_or(pres);
    if (x == 0) {
        s_max[wave] = top;
        s_pres[wave] = pres;
    }
    __syncthreads();
    const int base = max(max(s_max[0], s_max[1]), max(s_max[2], s_max[3]));
    const unsigned long long present = s_pres[0] | s_pres[1] | s_pres[2] | s_pres[3];
    int J = 0;                                                           // the largest j with a spanning link: uniform
    for (int j = 0; j < G; ++j)
        if (s_S[j]) J = j + 1;

    if (J == 0) {                                                        // no link jumps over m: a copy
#pragma unroll
        for (int r = 0; r < OF_ROWS; ++r) {
            const int y = wave + OF_WAVES * r;
            if (live && y < h) out_labels[fo + (int64_t)y * w + x] = own[r];
        }
        if (tid < K) {
            out_track[rowO + tid] = ((present >> tid) & 1ull) ? track[rowK + tid] : 0;
            age[rowO + tid] = 0;
        }
        if (table)
            for (int i = tid; i < K * CGS_OBJ_FIELDS; i += OF_THREADS) table[rowO * CGS_OBJ_FIELDS + i] = 0;
        return;
    }

    int key[OF_ROWS];                                                    // the claim of a cell: j << 8 | p, 0 for none
#pragma unroll
    for (int r = 0; r < OF_ROWS; ++r) key[r] = 0;
    if constexpr (MC) {                                                  // h = w = 64 here: every cell is inside
#pragma unroll
        for (int k = 0; k < (OF_MAX_GAP * OF_BLOCKS * OF_BLOCKS + OF_THREADS - 1) / OF_THREADS; ++k) {
            const int i = tid + k * OF_THREADS;
            if (i < J * OF_BLOCKS * OF_BLOCKS) {                         // m - 1 - s >= m - J >= 0, and m <= n - 2 when a link spans it
                const int8_t* v = bwd + ((int64_t)(m - 1 - (i >> 6)) * (OF_BLOCKS * OF_BLOCKS) + (i & 63)) * 2;
                s_m[i >> 6][i & 63] = (uint16_t)((uint32_t)(uint8_t)v[0] | ((uint32_t)(uint8_t)v[1] << 8));
            }
        }
        for (int j = 1; j <= J; ++j) {
            const unsigned long long S = s_S[j - 1];
            if (!S) continue;
            const int64_t fa = (int64_t)(m - j) * hw;
            int pa[OF_ROWS];                                             // all of a lane's loads in flight before the first is used
#pragma unroll
            for (int r = 0; r < OF_ROWS; ++r) pa[r] = labels[fa + (wave + OF_WAVES * r) * OF_SIDE + x];
#pragma unroll
            for (int r = 0; r < OF_ROWS; ++r) {
                const int p = pa[r];
                s_L[j - 1][(wave + OF_WAVES * r) * OF_SIDE + x] = (uint8_t)((p >= 1 && p <= K && ((S >> (p - 1)) & 1ull)) ? p : 0);
            }
        }
        __syncthreads();
        int my[OF_ROWS], mx[OF_ROWS];
#pragma unroll
        for (int r = 0; r < OF_ROWS; ++r) my[r] = mx[r] = 0;
        for (int j = 1; j <= J; ++j) {
            const bool spans = s_S[j - 1] != 0ull;
#pragma unroll
            for (int r = 0; r < OF_ROWS; ++r) {
                const int y = wave + OF_WAVES * r;
                const int qy = min(max(y + my[r], 0), OF_SIDE - 1), qx = min(max(x + mx[r], 0), OF_SIDE - 1);
                const uint32_t v = s_m[j - 1][(qy >> 3) * OF_BLOCKS + (qx >> 3)];
                my[r] += (int)(int8_t)(v & 255u);
                mx[r] += (int)(int8_t)(v >> 8);
                const int sy = y + my[r], sx = x + mx[r];
                if (spans && key[r] == 0 && own[r] <= 0 && sy >= 0 && sy < OF_SIDE && sx >= 0 && sx < OF_SIDE) {
                    const int p = s_L[j - 1][sy * OF_SIDE + sx];
                    if (p) key[r] = (j << 8) | p;
                }
            }
        }
    } else {
        for (int j = 1; j <= J; ++j) {
            const unsigned long long S = s_S[j - 1];
            if (!S) continue;
            const int64_t fa = (int64_t)(m - j) * hw;
#pragma unroll
            for (int r = 0; r < OF_ROWS; ++r) {
                const int y = wave + OF_WAVES * r;
                if (live && y < h && key[r] == 0 && own[r] <= 0) {
                    const int p = labels[fa + (int64_t)y * w + x];
                    if (p >= 1 && p <= K && ((S >> (p - 1)) & 1ull)) key[r] = (j << 8) | p;
                }
            }
        }
    }

#pragma unroll
    for (int r = 0; r < OF_ROWS; ++r) {                                  // the candidates that hold a cell: one OR per run of a row
        const int left = __shfl_up(key[r], 1, CGS_WAVE);
        if (key[r] && (x == 0 || key[r] != left)) atomicOr(&s_C[(key[r] >> 8) - 1], 1ull << ((key[r] & 255) - 1));
    }
    __syncthreads();
    int before[OF_MAX_GAP], cands = 0;                                   // candidates of a smaller j
#pragma unroll
    for (int j = 0; j < OF_MAX_GAP; ++j) {
        before[j] = cands;
        cands += j < J ? __popcll(s_C[j]) : 0;
    }
    const int room = base < K ? K - base : 0, made = min(cands, room);    // labels base + 1 .. base + made
    const unsigned long long upto = (2ull << x) - 1ull;
#pragma unroll
    for (int r = 0; r < OF_ROWS; ++r) {
        const int y = wave + OF_WAVES * r;
        int nl = 0;
        if (key[r]) {
            const int j = key[r] >> 8, p = key[r] & 255;
            int rank = 0;
#pragma unroll
            for (int k = 0; k < OF_MAX_GAP; ++k)
                if (k == j - 1) rank = before[k];
            rank += __popcll(s_C[j - 1] & ((1ull << (p - 1)) - 1ull));
            if (rank < room) nl = base + rank + 1;
        }
        if (live && y < h) out_labels[fo + (int64_t)y * w + x] = nl ? nl : own[r];
        const int left = __shfl_up(nl, 1, CGS_WAVE);
        const unsigned long long starts = __ballot(x == 0 || nl != left);
        const bool last = x == CGS_WAVE - 1 || ((starts >> (x + 1)) & 1ull);
        if (last && nl) {                                                // the run start .. x of row y
            const int start = 63 - __clzll((long long)(starts & upto)), len = x - start + 1;
            int* row = s_tab + (nl - 1) * CGS_OBJ_FIELDS;
            atomicAdd(row + 0, len);
            atomicMin(row + 1, start);
            atomicMin(row + 2, y);
            atomicMax(row + 3, x);
            atomicMax(row + 4, y);
            atomicAdd(row + 5, (start + x) * len / 2);
            atomicAdd(row + 6, y * len);
            atomicMin(row + 7, y * w + start);
        }
    }
    __syncthreads();

    if (table)
        for (int i = tid; i < K * CGS_OBJ_FIELDS; i += OF_THREADS) table[rowO * CGS_OBJ_FIELDS + i] = s_tab[i & ~7] > 0 ? s_tab[i] : 0;
    if (tid < K && !(tid >= base && tid - base < made)) {                // label tid + 1 is not a new one
        out_track[rowO + tid] = ((present >> tid) & 1ull) ? track[rowK + tid] : 0;
        age[rowO + tid] = 0;
    }
    for (int i = tid; i < J * OF_MAX_K; i += OF_THREADS) {               // candidate (j, p) = (i / 64 + 1, i % 64 + 1)
        const int j = i >> 6, b = i & 63;
        const unsigned long long C = s_C[j];
        if ((C >> b) & 1ull) {
            int rank = __popcll(C & ((1ull << b) - 1ull));
            for (int k = 0; k < j; ++k) rank += __popcll(s_C[k]);
            if (rank < room) {
                age[rowO + base + rank] = j + 1;
                out_track[rowO + base + rank] = track[(int64_t)(m - j - 1) * K + b];
            }
        }
    }
    if (tid < CGS_WAVE) {
        int cells = (tid < K) ? s_tab[tid * CGS_OBJ_FIELDS] : 0;
#pragma unroll
        for (int k = 32; k >= 1; k >>= 1) cells += __shfl_xor(cells, k, CGS_WAVE);
        if (tid == 0) {
            int vanished = 0;
            for (int j = 0; j < J; ++j) vanished += __popcll(s_S[j] & ~s_C[j]);
            if (made) atomicAdd(totals + 0, made);
            if (cells) atomicAdd(totals + 1, cells);
            if (cands > made) atomicAdd(totals + 2, cands - made);
            if (vanished) atomicAdd(totals + 3, vanished);
        }
    }
}

// Both entries: the frames f0 <= m < f1 of the window of n frames, one workgroup each; the outputs hold those frames only.
int fill_launch(const int32_t* labels, const int8_t* bwd, int32_t n, int32_t h, int32_t w, int32_t max_objects, int32_t max_gap,
                const int32_t* prev, const int32_t* gap, const int32_t* track, int32_t* out_labels, int32_t* out_track, int32_t* age,
                int32_t* table, int32_t* totals, int32_t f0, int32_t f1, cgs_stream_t stream_) {
    if (!labels || !prev || !gap || !track || !out_labels || !out_track || !age || !totals || n < 1 || h < 1 || w < 1 || max_objects < 1 ||
        max_gap < 1 || max_gap > OF_MAX_GAP || ((uintptr_t)labels & 3u) || ((uintptr_t)prev & 3u) || ((uintptr_t)gap & 3u) ||
        ((uintptr_t)track & 3u) || ((uintptr_t)out_labels & 3u) || ((uintptr_t)out_track & 3u) || ((uintptr_t)age & 3u) ||
        ((uintptr_t)table & 3u) || ((uintptr_t)totals & 3u) || out_labels == labels || f0 < 0 || f0 > f1 || f1 > n)
        return CGS_ERR_BADARG;
    if (bwd ? (h != OF_SIDE || w != OF_SIDE) : (h > OF_SIDE || w > OF_SIDE)) return CGS_ERR_UNSUPPORTED;
    if (max_objects > OF_MAX_K || n > CGS_OBJ_TRACK_MAX_FRAMES) return CGS_ERR_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    const hipError_t e = hipMemsetAsync(totals, 0, 4 * sizeof(int32_t), stream);
    if (e != hipSuccess) return (int)e;
    if (f0 == f1) return CGS_OK;
    if (bwd)
        hipLaunchKernelGGL(fill_kernel<true>, dim3((unsigned)(f1 - f0)), dim3(OF_THREADS), 0, stream, labels, bwd, (int)n, (int)h, (int)w,
                           (int)max_objects, (int)max_gap, prev, gap, track, out_labels, out_track, age, table, totals, (int)f0);
    else
        hipLaunchKernelGGL(fill_kernel<false>, dim3((unsigned)(f1 - f0)), dim3(OF_THREADS), 0, stream, labels, bwd, (int)n, (int)h, (int)w,
                           (int)max_objects, (int)max_gap, prev, gap, track, out_labels, out_track, age, table, totals, (int)f0);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}

}  // namespace

extern "C" int cgs_objects_track_fill(const int32_t* labels, const int8_t* bwd, int32_t n, int32_t h, int32_t w, int32_t max_objects,
                                      int32_t max_gap, const int32_t* prev, const int32_t* gap, const int32_t* track,
                                      int32_t* out_labels, int32_t* out_track, int32_t* age, int32_t* table, int32_t* totals,
                                      cgs_stream_t stream_) {
    return fill_launch(labels, bwd, n, h, w, max_objects, max_gap, prev, gap, track, out_labels, out_track, age, table, totals, 0, n, stream_);
}

extern "C" int cgs_objects_track_fill_window(const int32_t* labels, const int8_t* bwd, int32_t n, int32_t h, int32_t w, int32_t max_objects,
                                             int32_t max_gap, const int32_t* prev, const int32_t* gap, const int32_t* track, int32_t f0,
                                             int32_t f1, int32_t* out_labels, int32_t* out_track, int32_t* age, int32_t* table,
                                             int32_t* totals, cgs_stream_t stream_) {
    return fill_launch(labels, bwd, n, h, w, max_objects, max_gap, prev, gap, track, out_labels, out_track, age, table, totals, f0, f1, stream_);
}
