// GrabCut-style mask refinement by an exact binary min cut (cgs_graph_cut, include/cgs_hip.h: its header comment is the rule), for a stack
// of frames of at most 64 x 64 cells.  One workgroup of 16 waves per frame; a thread owns the cells tid, tid + 1024, ...  The whole
// graph lives in LDS:
//
//   s_cap   [8][4096] uint16   residual of the arc cell -> neighbour in direction d (E W S N SE NW SW NE: the opposite of d is d ^ 1); an
//                              arc that leaves the frame, or a diagonal at connectivity 4, has 0 and is never followed, so no neighbour
//                              index is formed out of range.  cap[d][p] + cap[d ^ 1][q] is twice the pair's capacity at all times, which
//                              is how the capacities are restored between the cuts of a frame
//   s_ex    [4096] int32       excess (the source is folded away: excess starts as max(cs - ct, 0)); the packed RGB during the set-up
//   s_sink  [4096] int32       residual of cell -> sink, max(ct - cs, 0) at the start
//   s_h     [2][4096] uint16   distance labels, 0xFFFF = the sink cannot be reached; the relabel phase reads one copy and writes the other
//   s_bin, s_lab, s_tri        histogram bin, current label, trimap of a cell;  s_hist [2][512] the two colour models
//
// 132.1 KiB, one workgroup per CU.  Push-relabel, barrier-synchronous, in rounds:
//   search   exact backward breadth-first search from the sink, one level per step (a cell without a distance takes s + 1 when a residual
//            arc leads to a cell of level s), at most h w steps; one barrier per step (three rotating "something changed" flags)
//   done?    no cell with excess has a distance: the flow is maximal, the label is "no distance"
//   sweeps   K times: push phase -- every cell with excess and a distance pushes to the sink, then along the admissible arcs in the order
//            of d, spending the excess it had at the barrier; it alone writes its two arcs' residuals (the neighbour cannot push back in
//            the same phase: that needs the opposite height difference), arrivals are LDS integer atomics -- barrier -- relabel phase --
//            a cell that still has excess and no admissible arc takes the least neighbour height over residual arcs + 1, read from the
//            old copy (heights only rise, so the labelling stays valid when neighbours relabel at once) -- barrier.  The sweeps end early
//            when no cell is active any more.
// Integer adds only, and no phase reads what the same phase writes, so nothing -- the rounds included -- depends on the order in which
// anything happens.  Every loop is bounded (K, h w, max_rounds, iters) and every exit is decided from an LDS word all threads read after
// the same barrier.
#include "cgs_common.h"

namespace {

constexpr int GC_THREADS = 1024;
constexpr int GC_MAX_PX = CGS_CUT_MAX_SIDE * CGS_CUT_MAX_SIDE;
constexpr int GC_CELLS = GC_MAX_PX / GC_THREADS;           // cells of a thread
constexpr int GC_DIRS = 8;
constexpr int GC_INF = 0xFFFF;
constexpr int GC_HARD_BG = 1, GC_HARD_FG = 2;
enum { ACC_D2 = 0, ACC_N1, ACC_BASE, ACC_SINK, ACC_CHANGED, ACC_ON, ACC_DIFF, ACC_SEED, ACC_UNKNOWN, ACC_N };

__device__ __forceinline__ int gc_dy(int d) { return ((0x2225 >> (2 * d)) & 3) - 1; }       // 0 0 1 -1 1 -1 1 -1
__device__ __forceinline__ int gc_dx(int d) { return ((0x8252 >> (2 * d)) & 3) - 1; }       // 1 -1 0 0 1 -1 -1 1

__device__ __forceinline__ bool gc_inside(int d, int x, int y, int h, int w, bool conn8) {
    const int xx = x + gc_dx(d), yy = y + gc_dy(d);
    return (d < 4 || conn8) && xx >= 0 && xx < w && yy >= 0 && yy < h;
}

// every thread of the workgroup calls this: the sum of v over the workgroup is added to *dst (one LDS atomic per wave)
template <typename T>
__device__ __forceinline__ void gc_add(T* dst, T v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, CGS_WAVE);
    if ((threadIdx.x & (CGS_WAVE - 1)) == 0 && v) atomicAdd(dst, v);
}

__device__ __forceinline__ int gc_d2(unsigned a, unsigned b) {
    const int dr = (int)(a >> 16) - (int)(b >> 16), dg = (int)((a >> 8) & 255u) - (int)((b >> 8) & 255u), db = (int)(a & 255u) - (int)(b & 255u);
    return dr * dr + dg * dg + db * db;
}

template <int K>
__global__ void __launch_bounds__(GC_THREADS)
graph_cut_kernel(const uint8_t* __restrict__ frames, const float* __restrict__ z, int kind, float thresh, float lo, float hi, int h, int w,
                 int conn8_, int blog, int iters, int max_rounds, const int32_t* __restrict__ wa, const int32_t* __restrict__ wd,
                 const int32_t* __restrict__ lt, uint8_t* __restrict__ out, int32_t* __restrict__ stats) {
    __shared__ uint16_t s_cap[GC_DIRS][GC_MAX_PX];
    __shared__ int s_ex[GC_MAX_PX];
    __shared__ int s_sink[GC_MAX_PX];
    __shared__ uint16_t s_h[2][GC_MAX_PX];
    __shared__ uint16_t s_bin[GC_MAX_PX];
    __shared__ uint8_t s_lab[GC_MAX_PX];
    __shared__ uint8_t s_tri[GC_MAX_PX];
    __shared__ int s_hist[2][512];
    __shared__ unsigned s_acc[ACC_N];
    __shared__ int s_bfs[3], s_sweep[3], s_active;

    const int tid = threadIdx.x, P = h * w;
    const bool conn8 = conn8_ != 0;
    const int64_t base = (int64_t)blockIdx.x * P;
    const int B = 1 << (3 * blog), shift = 8 - blog;
    int off[GC_DIRS];
#pragma unroll
    for (int d = 0; d < GC_DIRS; ++d) off[d] = gc_dy(d) * w + gc_dx(d);

    if (tid < ACC_N) s_acc[tid] = 0u;
    __syncthreads();

    // ---- set-up: seed labelling, trimap, bins, n-links
    {
        unsigned seed_on = 0u, unknown = 0u;
        for (int p = tid; p < P; p += GC_THREADS) {
            const float v = z[base + p];
            const bool on = kind == CGS_OBJ_F32_GE ? (v >= thresh) : (v > thresh);            // a NaN compares false
            const int tri = (v < lo || v != v) ? GC_HARD_BG : (v > hi ? GC_HARD_FG : 0);
            s_lab[p] = on;
            s_tri[p] = (uint8_t)tri;
            seed_on += on;
            unknown += tri == 0;
            const uint8_t* px = frames + 3 * (base + p);
            const unsigned r = px[0], g = px[1], b = px[2];
            s_ex[p] = (int)((r << 16) | (g << 8) | b);
            s_bin[p] = (uint16_t)(((r >> shift) << (2 * blog)) | ((g >> shift) << blog) | (b >> shift));
#pragma unroll
            for (int d = 0; d < GC_DIRS; ++d) s_cap[d][p] = 0;
        }
        gc_add(&s_acc[ACC_SEED], seed_on);
        gc_add(&s_acc[ACC_UNKNOWN], unknown);
    }
    __syncthreads();
    {
        unsigned sum = 0u;                                     // at most 16002 pairs of at most 195075: below 2^32
        for (int p = tid; p < P; p += GC_THREADS) {
            const int y = p / w, x = p - y * w;
#pragma unroll
            for (int d = 0; d < GC_DIRS; d += 2)
                if (gc_inside(d, x, y, h, w, conn8)) sum += (unsigned)gc_d2((unsigned)s_ex[p], (unsigned)s_ex[p + off[d]]);
        }
        gc_add(&s_acc[ACC_D2], sum);
    }
    __syncthreads();
    {
        const unsigned pairs = (unsigned)(h * (w - 1) + (h - 1) * w + (conn8 ? 2 * (h - 1) * (w - 1) : 0));
        const unsigned mean = pairs ? s_acc[ACC_D2] / pairs : 0u, m = mean ? mean : 1u;
        for (int p = tid; p < P; p += GC_THREADS) {
            const int y = p / w, x = p - y * w;
#pragma unroll
            for (int d = 0; d < GC_DIRS; d += 2) {
                if (!gc_inside(d, x, y, h, w, conn8)) continue;
                const int q = p + off[d];
                const unsigned i = 64u * (unsigned)gc_d2((unsigned)s_ex[p], (unsigned)s_ex[q]) / m;
                const int c = (d < 4 ? wa : wd)[i < (unsigned)(CGS_CUT_TABLE - 1) ? i : (unsigned)(CGS_CUT_TABLE - 1)];
                s_cap[d][p] = (uint16_t)c;                     // (the two arcs of a pair are written by the pair's first cell alone)
                s_cap[d ^ 1][q] = (uint16_t)c;
            }
        }
    }
    const int big = 8 * wa[0] + 1;
    __syncthreads();                                           // (s_ex is free from here on)

    int status = 0, cuts = 0, rounds_max = 0, energy = 0;
    for (int it = 0; it < iters; ++it) {
        // ---- colour models of the current labelling
        for (int i = tid; i < 2 * 512; i += GC_THREADS) (&s_hist[0][0])[i] = 0;
        if (tid == 0) s_acc[ACC_N1] = s_acc[ACC_BASE] = s_acc[ACC_SINK] = s_acc[ACC_CHANGED] = 0u;
        __syncthreads();
        {
            unsigned n1 = 0u;
            for (int p = tid; p < P; p += GC_THREADS) {
                const int lab = s_lab[p];
                atomicAdd(&s_hist[lab][s_bin[p]], 1);
                n1 += lab;
            }
            gc_add(&s_acc[ACC_N1], n1);
        }
        __syncthreads();
        const int N1 = (int)s_acc[ACC_N1], N0 = P - N1;
        if (N1 == 0 || N0 == 0) {                              // (uniform: read after the barrier)
            status |= CGS_CUT_EMPTY;
            break;
        }
        // ---- capacities restored, t-links
        {
            const int l1 = lt[N1 + B], l0 = lt[N0 + B];
            unsigned through = 0u;
            for (int p = tid; p < P; p += GC_THREADS) {
                if (it > 0) {
                    const int y = p / w, x = p - y * w;
#pragma unroll
                    for (int d = 0; d < GC_DIRS; d += 2) {
                        if (!gc_inside(d, x, y, h, w, conn8)) continue;
                        const int q = p + off[d];
                        const uint16_t c = (uint16_t)((s_cap[d][p] + s_cap[d ^ 1][q]) >> 1);
                        s_cap[d][p] = c;
                        s_cap[d ^ 1][q] = c;
                    }
                }
                const int tri = s_tri[p], bin = s_bin[p];
                int cs, ct;                                    // source -> cell, cell -> sink
                if (tri == GC_HARD_FG) {
                    cs = big, ct = 0;
                } else if (tri == GC_HARD_BG) {
                    cs = 0, ct = big;
                } else {
                    cs = l0 - lt[s_hist[0][bin] + 1];          // cost_bg
                    ct = l1 - lt[s_hist[1][bin] + 1];          // cost_fg
                }
                s_ex[p] = cs > ct ? cs - ct : 0;
                s_sink[p] = ct > cs ? ct - cs : 0;
                through += (unsigned)(cs < ct ? cs : ct);
            }
            gc_add(&s_acc[ACC_BASE], through);
        }
        __syncthreads();

        // ---- the cut
        bool finished = false;
        int rounds = 0;
        unsigned to_sink = 0u;
        for (int r = 1; r <= max_rounds; ++r) {
            rounds = r;
            uint16_t* dist = s_h[0];
            for (int p = tid; p < P; p += GC_THREADS) dist[p] = s_sink[p] > 0 ? 1 : GC_INF;
            if (tid == 0) s_bfs[0] = s_bfs[1] = s_bfs[2] = s_sweep[0] = s_sweep[1] = s_sweep[2] = s_active = 0;
            __syncthreads();
            for (int s = 1; s <= P; ++s) {
                bool any = false;
                for (int p = tid; p < P; p += GC_THREADS) {
                    if (dist[p] != GC_INF) continue;
                    bool hit = false;                          // (dist is read only behind a residual > 0, which an arc out of the frame never
                                                               // has: p + off[d] is in range wherever it is used, here and in the sweeps)
#pragma unroll
                    for (int d = 0; d < GC_DIRS; ++d)
                        if (s_cap[d][p] > 0 && dist[p + off[d]] == s) hit = true;
                    if (hit) {
                        dist[p] = (uint16_t)(s + 1);           // (a reader of this step looks for s: s + 1 and 0xFFFF are the same to it)
                        any = true;
                    }
                }
                if (any) s_bfs[s % 3] = 1;
                if (tid == 0) s_bfs[(s + 1) % 3] = 0;
                __syncthreads();
                if (!s_bfs[s % 3]) break;
            }
            int own[GC_CELLS];                                 // the excess of the thread's cells as the last barrier left it
            {
                bool active = false;
#pragma unroll
                for (int i = 0; i < GC_CELLS; ++i) {
                    const int p = tid + i * GC_THREADS;
                    own[i] = p < P ? s_ex[p] : 0;
                    active |= own[i] > 0 && dist[p < P ? p : 0] != GC_INF;
                }
                if (active) s_active = 1;
            }
            __syncthreads();
            if (!s_active) {
                finished = true;
                break;
            }
            if (r == max_rounds) break;
            int cur = 0;
            for (int k = 0; k < K; ++k) {
                const uint16_t* ha = s_h[cur];
                uint16_t* hb = s_h[cur ^ 1];
#pragma unroll
                for (int i = 0; i < GC_CELLS; ++i) {           // push: what a cell had at the barrier, not what arrives meanwhile
                    const int p = tid + i * GC_THREADS, e0 = own[i];
                    if (e0 <= 0) continue;                     // (own is 0 beyond the frame)
                    const int hp = ha[p];
                    if (hp == GC_INF) continue;
                    int e = e0;
                    const int sr = s_sink[p];
                    if (sr > 0) {
                        const int dl = e < sr ? e : sr;
                        s_sink[p] = sr - dl;
                        e -= dl;
                        to_sink += (unsigned)dl;
                    }
#pragma unroll
                    for (int d = 0; d < GC_DIRS; ++d) {
                        const int c = s_cap[d][p];
                        if (e > 0 && c > 0) {
                            const int q = p + off[d];
                            if ((int)ha[q] + 1 == hp) {
                                const int dl = e < c ? e : c;
                                s_cap[d][p] = (uint16_t)(c - dl);
                                s_cap[d ^ 1][q] = (uint16_t)(s_cap[d ^ 1][q] + dl);
                                atomicAdd(&s_ex[q], dl);
                                e -= dl;
                            }
                        }
                    }
                    if (e != e0) atomicAdd(&s_ex[p], e - e0);
                }
                __syncthreads();
                bool any = false;
#pragma unroll
                for (int i = 0; i < GC_CELLS; ++i) {           // relabel
                    const int p = tid + i * GC_THREADS;
                    if (p >= P) continue;
                    const int hp = ha[p], e = s_ex[p];
                    own[i] = e;
                    int nh = hp;
                    if (e > 0 && hp != GC_INF && s_sink[p] == 0) {
                        int least = GC_INF;
                        bool admissible = false;
#pragma unroll
                        for (int d = 0; d < GC_DIRS; ++d) {
                            if (s_cap[d][p] > 0) {
                                const int hq = ha[p + off[d]];
                                admissible |= hq + 1 == hp;
                                least = hq < least ? hq : least;
                            }
                        }
                        if (!admissible) nh = least >= P ? GC_INF : least + 1;        // (a distance is at most h w)
                    }
                    hb[p] = (uint16_t)nh;
                    any |= e > 0 && nh != GC_INF;
                }
                if (any) s_sweep[k % 3] = 1;
                if (tid == 0) s_sweep[(k + 1) % 3] = 0;
                cur ^= 1;
                __syncthreads();
                if (!s_sweep[k % 3]) break;
            }
        }
        rounds_max = rounds > rounds_max ? rounds : rounds_max;
        if (!finished) {                                       // (uniform) the labelling the cut started from stays
            status |= CGS_CUT_NOT_CONVERGED;
            break;
        }
        {
            unsigned changed = 0u;
            for (int p = tid; p < P; p += GC_THREADS) {
                const int nl = s_h[0][p] == GC_INF;
                changed += nl != s_lab[p];
                s_lab[p] = (uint8_t)nl;
            }
            gc_add(&s_acc[ACC_SINK], to_sink);
            gc_add(&s_acc[ACC_CHANGED], changed);
        }
        __syncthreads();
        energy = (int)(s_acc[ACC_BASE] + s_acc[ACC_SINK]);
        ++cuts;
        const bool same = s_acc[ACC_CHANGED] == 0u;
        __syncthreads();                                       // (the next cut clears what was just read)
        if (same) {
            if (cuts < iters) status |= CGS_CUT_EARLY;
            break;
        }
    }

    // ---- output
    {
        unsigned on = 0u, diff = 0u;
        for (int p = tid; p < P; p += GC_THREADS) {
            const int lab = s_lab[p];
            const float v = z[base + p];
            const int seed = kind == CGS_OBJ_F32_GE ? (v >= thresh) : (v > thresh);
            out[base + p] = (uint8_t)lab;
            on += lab;
            diff += lab != seed;
        }
        gc_add(&s_acc[ACC_ON], on);
        gc_add(&s_acc[ACC_DIFF], diff);
    }
    __syncthreads();
    if (tid == 0) {
        int32_t* st = stats + (int64_t)CGS_CUT_FIELDS * blockIdx.x;
        st[0] = status;
        st[1] = cuts;
        st[2] = rounds_max;
        st[3] = energy;
        st[4] = (int)s_acc[ACC_SEED];
        st[5] = (int)s_acc[ACC_ON];
        st[6] = (int)s_acc[ACC_UNKNOWN];
        st[7] = (int)s_acc[ACC_DIFF];
    }
}

template <int K>
int launch(const uint8_t* frames, const float* z, int32_t src_kind, float thresh, float lo, float hi, int32_t n, int32_t h, int32_t w,
           int32_t connectivity, int32_t bins, int32_t iters, int32_t max_rounds, const int32_t* wa, const int32_t* wd, const int32_t* l,
           uint8_t* out, int32_t* stats, cgs_stream_t stream_) {
    hipLaunchKernelGGL(graph_cut_kernel<K>, dim3((unsigned)n), dim3(GC_THREADS), 0, (hipStream_t)stream_, frames, z, (int)src_kind, thresh,
                       lo, hi, (int)h, (int)w, (int)(connectivity == 8), bins == 8 ? 3 : 2, (int)iters, (int)max_rounds, wa, wd, l, out, stats);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}

}  // namespace

extern "C" int cgs_graph_cut_sweeps(const uint8_t* frames, const float* z, int32_t src_kind, float thresh, float lo, float hi, int32_t n,
                                    int32_t h, int32_t w, int32_t connectivity, int32_t bins, int32_t iters, int32_t max_rounds,
                                    int32_t sweeps, const int32_t* wa, const int32_t* wd, const int32_t* l, uint8_t* out, int32_t* stats,
                                    cgs_stream_t stream) {
    if (!frames || !z || !wa || !wd || !l || !out || !stats || n < 1 || (src_kind != CGS_OBJ_F32_GT && src_kind != CGS_OBJ_F32_GE) ||
        !(lo <= thresh && thresh <= hi) || (connectivity != 4 && connectivity != 8) || (bins != 4 && bins != 8) || iters < 1 ||
        iters > CGS_CUT_MAX_ITERS || max_rounds < 1 || max_rounds > CGS_CUT_MAX_ROUNDS)                     // (a NaN fails the compares)
        return CGS_ERR_BADARG;
    if (((uintptr_t)z | (uintptr_t)wa | (uintptr_t)wd | (uintptr_t)l | (uintptr_t)stats) & 3u) return CGS_ERR_BADARG;
    if (h < 1 || w < 1 || h > CGS_CUT_MAX_SIDE || w > CGS_CUT_MAX_SIDE) return CGS_ERR_UNSUPPORTED;
#define GC_ARGS frames, z, src_kind, thresh, lo, hi, n, h, w, connectivity, bins, iters, max_rounds, wa, wd, l, out, stats, stream
    if (sweeps == 16) return launch<16>(GC_ARGS);
    if (sweeps == 32) return launch<32>(GC_ARGS);
    if (sweeps == 64) return launch<64>(GC_ARGS);
#undef GC_ARGS
    return CGS_ERR_UNSUPPORTED;
}

extern "C" int cgs_graph_cut(const uint8_t* frames, const float* z, int32_t src_kind, float thresh, float lo, float hi, int32_t n, int32_t h,
                             int32_t w, int32_t connectivity, int32_t bins, int32_t iters, int32_t max_rounds, const int32_t* wa,
                             const int32_t* wd, const int32_t* l, uint8_t* out, int32_t* stats, cgs_stream_t stream) {
    return cgs_graph_cut_sweeps(frames, z, src_kind, thresh, lo, hi, n, h, w, connectivity, bins, iters, max_rounds, CGS_CUT_SWEEPS, wa, wd, l,
                                out, stats, stream);
}
