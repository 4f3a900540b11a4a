// From per-frame objects to tracks across the frames of one label stack (cgs_objects_track, cgs_objects_track_switches,
// include/cgs_hip.h).  Everything is integer; the only global atomics are integer add / min / max, so nothing depends on an order.
//
//   pairs     cgs_objects_match (objects_match.hip, called, not copied) on frames (f, f + 1) of the same stack gives every object's
//             best partner in the next frame from both sides, and one self-pair of the last frame gives its areas: slot f of `best`
//             in scratch is pair (f, f + 1), slot n - 1 the self-pair, so best[f][0][l - 1][2] is the area of object l of frame f.
//   link      a lane is one (f, l): its side-1 row of pair f - 1 names the partner p, p's side-0 row must name l back, and the
//             threshold must hold; prev and the root pointer ((f - 1) K + p - 1, or itself) are written, the frame's heads are one
//             ballot (kept as a 64-bit mask: a head's rank among them is a popcount below its lane).
//   resolve   pointer doubling root'[i] = root[root[i]] between two buffers, R rounds with 2^R >= n - 1: one launch per round.
//             (A chunked form in LDS was not built: see DESIGN.md.)
//   number    one workgroup scans the per-frame head counts; track number = base[frame of the root] + rank of the root + 1.
//   heads     every head fills the constant fields of its row (first_frame, first_label) and area_min with its own area, in a
//             launch of its own, so that the atomics of the next one start from initialised rows.
//   table     every object adds itself to its track's row: length, area_sum, area_min, area_max, and its backward link's inter and
//             union; the longest length is max(f - first_frame + 1), reduced per workgroup and then one atomic max.
//   paint     one lane per pixel: track_labels and / or rgb.
//
// Launches: init, match (n > 1), self-match, link, R x resolve, number, heads, table, paint: 7 + R + (n > 1), a function of n alone
// (paint is launched also when both its outputs are NULL and then returns at once).
//
// cgs_objects_track_gap bridges gaps of up to G missing frames: the path above as level 1, then per level g = 2 .. G + 1 one launch of
// track_level_kernel over the frame pairs (f - g, f); see "bridged gaps" below and DESIGN.md.
//
// cgs_objects_track_mc is the same path with the earlier frame's labels carried along a block motion field before they are counted:
// track_level_kernel<true> gathers them in LDS, at level 1 too (there it writes `best` in objects_match_kernel's layout); see "carried
// labels" below.  Everything after the counting is the kernels above and below, called as they are.
#include "pixel_common.h"

namespace {

constexpr int OT_THREADS = 256;
constexpr int OT_WAVES = OT_THREADS / CGS_WAVE;
constexpr int OT_MAX_K = CGS_OBJ_MATCH_MAX_OBJECTS;
constexpr int OT_SCAN_THREADS = 1024;
static_assert(OT_MAX_K == CGS_WAVE, "one lane per object of a frame");
static_assert((int64_t)CGS_OBJ_TRACK_MAX_FRAMES * OT_MAX_K < (1ll << 31), "root pointers are int32");
static_assert((int64_t)CGS_OBJ_TRACK_MAX_FRAMES * 8191 < (1ll << 31), "area_sum and union_sum stay inside int32");

// scratch, in 32-bit words (the head masks are 64-bit: their offset is even for every n and K)
struct Layout {
    int64_t milli, counts, best, root_a, root_b, heads, base, words;
};
__host__ __device__ inline Layout layout(int64_t n, int64_t K) {
    Layout o;
    o.milli = 0;
    o.counts = 4;
    o.best = o.counts + 4 * n;
    o.root_a = o.best + 8 * n * K;
    o.root_b = o.root_a + n * K;
    o.heads = o.root_b + n * K;
    o.base = o.heads + 2 * n;
    o.words = o.base + n;
    return o;
}

__global__ void __launch_bounds__(OT_THREADS)
track_init_kernel(int32_t* __restrict__ tracks, int64_t words, int32_t* __restrict__ totals, int32_t* __restrict__ milli, int iou) {
    const int64_t step = (int64_t)gridDim.x * OT_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * OT_THREADS + threadIdx.x; i < words; i += step) tracks[i] = 0;
    if (blockIdx.x == 0 && threadIdx.x < 4) {
        totals[threadIdx.x] = 0;
        milli[threadIdx.x] = iou;
    }
}

__global__ void __launch_bounds__(OT_THREADS)
track_link_kernel(const int32_t* __restrict__ best, int n, int K, int iou, int32_t* __restrict__ prev, int32_t* __restrict__ root,
                  unsigned long long* __restrict__ heads, int32_t* __restrict__ totals) {
    __shared__ int s_cnt[2];
    const int lane = threadIdx.x & (CGS_WAVE - 1), wave = threadIdx.x / CGS_WAVE;
    const int f = blockIdx.x * OT_WAVES + wave;
    const bool in = f < n && lane < K;
    if (threadIdx.x < 2) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const int area = in ? best[(((int64_t)f * 2 + 0) * K + lane) * 4 + 2] : 0;
    const bool obj = area > 0;
    int p = 0;
    if (obj && f > 0) {
        const int32_t* row = best + (((int64_t)(f - 1) * 2 + 1) * K + lane) * 4;      // (partner, inter, own area, partner's area)
        const int q = row[0], inter = row[1], uni = row[2] + row[3] - row[1];
        if (q >= 1 && q <= K && inter > 0 && 1000 * inter >= iou * uni &&
            best[(((int64_t)(f - 1) * 2 + 0) * K + q - 1) * 4] == lane + 1)
            p = q;
    }
    if (in) {
        prev[(int64_t)f * K + lane] = p;
        root[(int64_t)f * K + lane] = p ? (f - 1) * K + p - 1 : f * K + lane;
    }
    const unsigned long long head = __ballot(obj && p == 0), objs = __ballot(obj), links = __ballot(p > 0);
    if (lane == 0 && f < n) {
        heads[f] = head;
        if (links) atomicAdd(&s_cnt[0], __popcll(links));
        if (objs) atomicAdd(&s_cnt[1], __popcll(objs));
    }
    __syncthreads();
    if (threadIdx.x < 2 && s_cnt[threadIdx.x]) atomicAdd(&totals[1 + threadIdx.x], s_cnt[threadIdx.x]);
}

__global__ void __launch_bounds__(OT_THREADS)
track_resolve_kernel(const int32_t* __restrict__ src, int32_t* __restrict__ dst, int total) {
    const int i = blockIdx.x * OT_THREADS + threadIdx.x;
    if (i < total) dst[i] = src[src[i]];
}

// exclusive scan of the head counts over the frames, one workgroup: a thread sums a run of frames, the runs' sums are scanned in LDS
__global__ void __launch_bounds__(OT_SCAN_THREADS)
track_number_kernel(const unsigned long long* __restrict__ heads, int n, int32_t* __restrict__ base, int32_t* __restrict__ totals) {
    __shared__ int s_sum[OT_SCAN_THREADS];
    const int t = threadIdx.x, chunk = (n + OT_SCAN_THREADS - 1) / OT_SCAN_THREADS;
    const int lo = min(t * chunk, n), hi = min(lo + chunk, n);
    int sum = 0;
    for (int f = lo; f < hi; ++f) sum += __popcll(heads[f]);
    s_sum[t] = sum;
    __syncthreads();
    for (int d = 1; d < OT_SCAN_THREADS; d <<= 1) {
        const int add = t >= d ? s_sum[t - d] : 0;
        __syncthreads();
        s_sum[t] += add;
        __syncthreads();
    }
    int run = s_sum[t] - sum;
    for (int f = lo; f < hi; ++f) {
        base[f] = run;
        run += __popcll(heads[f]);
    }
    if (t == OT_SCAN_THREADS - 1) totals[0] = s_sum[t];
}

__device__ __forceinline__ int track_number(const unsigned long long* heads, const int32_t* base, int fr, int lr) {
    return base[fr] + __popcll(heads[fr] & ((1ull << lr) - 1ull)) + 1;
}

__global__ void __launch_bounds__(OT_THREADS)
track_heads_kernel(const int32_t* __restrict__ best, const unsigned long long* __restrict__ heads, const int32_t* __restrict__ base,
                   int n, int K, int32_t* __restrict__ tracks, int max_tracks) {
    const int lane = threadIdx.x & (CGS_WAVE - 1);
    const int f = blockIdx.x * OT_WAVES + threadIdx.x / CGS_WAVE;
    if (f >= n || lane >= K || !((heads[f] >> lane) & 1ull)) return;
    const int t = track_number(heads, base, f, lane);
    if (t > max_tracks) return;
    int32_t* row = tracks + (int64_t)(t - 1) * CGS_OBJ_TRACK_FIELDS;
    row[0] = f;
    row[1] = lane + 1;
    row[4] = best[(((int64_t)f * 2 + 0) * K + lane) * 4 + 2];
}

__global__ void __launch_bounds__(OT_THREADS)
track_table_kernel(const int32_t* __restrict__ best, const int32_t* __restrict__ root, const unsigned long long* __restrict__ heads,
                   const int32_t* __restrict__ base, const int32_t* __restrict__ prev, int n, int K, int32_t* __restrict__ track,
                   int32_t* __restrict__ tracks, int max_tracks, int32_t* __restrict__ totals) {
    __shared__ int s_len[OT_WAVES];
    const int lane = threadIdx.x & (CGS_WAVE - 1), wave = threadIdx.x / CGS_WAVE;
    const int f = blockIdx.x * OT_WAVES + wave;
    const bool in = f < n && lane < K;
    const int area = in ? best[(((int64_t)f * 2 + 0) * K + lane) * 4 + 2] : 0;
    int t = 0, len = 0;
    if (area > 0) {
        const int r = root[(int64_t)f * K + lane], fr = r / K, lr = r - fr * K;
        t = track_number(heads, base, fr, lr);
        len = f - fr + 1;
        if (tracks && t <= max_tracks) {
            int32_t* row = tracks + (int64_t)(t - 1) * CGS_OBJ_TRACK_FIELDS;
            atomicAdd(row + 2, 1);
            atomicAdd(row + 3, area);
            atomicMin(row + 4, area);
            atomicMax(row + 5, area);
            if (prev[(int64_t)f * K + lane] > 0) {
                const int32_t* link = best + (((int64_t)(f - 1) * 2 + 1) * K + lane) * 4;
                atomicAdd(row + 6, link[1]);
                atomicAdd(row + 7, link[2] + link[3] - link[1]);
            }
        }
    }
    if (in) track[(int64_t)f * K + lane] = t;
    len = px_wave_max(len);
    if (lane == 0) s_len[wave] = len;
    __syncthreads();
    if (threadIdx.x == 0) {
        const int longest = max(max(s_len[0], s_len[1]), max(s_len[2], s_len[3]));
        if (longest > 0) atomicMax(totals + 3, longest);
    }
}

__global__ void __launch_bounds__(OT_THREADS)
track_paint_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ track, int64_t total, int hw, int K,
                   int32_t* __restrict__ track_labels, uint8_t* __restrict__ rgb) {
    const int64_t i = (int64_t)blockIdx.x * OT_THREADS + threadIdx.x;
    if (i >= total || (!track_labels && !rgb)) return;
    const int l = labels[i];
    const int t = (l >= 1 && l <= K) ? track[(i / hw) * K + l - 1] : 0;
    if (track_labels) track_labels[i] = t;
    if (rgb) {
        const uint32_t hsh = (uint32_t)t * 2654435761u;
#pragma unroll
        for (int c = 0; c < 3; ++c) rgb[3 * i + c] = t ? (uint8_t)(64u + ((hsh >> (8 * c)) & 255u) * 191u / 255u) : (uint8_t)0;
    }
}

// Identity switches of a prediction's tracks against the truth's: a lane is one truth object (f, q).  Gaps are not bridged.
__global__ void __launch_bounds__(OT_THREADS)
track_switches_kernel(const int32_t* __restrict__ truth_prev, const int32_t* __restrict__ pred_track, const int32_t* __restrict__ mb,
                      const int32_t* __restrict__ iou_milli, int T, int n, int K, int32_t* __restrict__ counts) {
    __shared__ int s_cnt[CGS_OBJ_MATCH_MAX_IOU * 3];
    const int lane = threadIdx.x & (CGS_WAVE - 1);
    const int f = blockIdx.x * OT_WAVES + threadIdx.x / CGS_WAVE;
    const bool in = f < n && lane < K;
    if (threadIdx.x < 3 * T) s_cnt[threadIdx.x] = 0;
    __syncthreads();
    int inter = 0, uni = 1, trk = 0, inter0 = 0, uni0 = 1, trk0 = -1;
    bool linked = false;
    if (in) {
        const int32_t* row = mb + (((int64_t)f * 2 + 1) * K + lane) * 4;                // (pred partner, inter, area_t, area_p)
        const int p = row[0];
        inter = row[1];
        uni = row[2] + row[3] - row[1];
        if (p >= 1 && p <= K) trk = pred_track[(int64_t)f * K + p - 1];
        const int q0 = f > 0 ? truth_prev[(int64_t)f * K + lane] : 0;
        if (q0 >= 1 && q0 <= K) {
            linked = true;
            const int32_t* row0 = mb + (((int64_t)(f - 1) * 2 + 1) * K + q0 - 1) * 4;
            const int p0 = row0[0];
            inter0 = row0[1];
            uni0 = row0[2] + row0[3] - row0[1];
            if (p0 >= 1 && p0 <= K) trk0 = pred_track[(int64_t)(f - 1) * K + p0 - 1];
        }
    }
    for (int k = 0; k < T; ++k) {
        const int m = iou_milli[k];
        const bool cov = in && inter > 0 && 1000 * inter >= m * uni;
        const bool cont = cov && linked && inter0 > 0 && 1000 * inter0 >= m * uni0;
        const unsigned long long b0 = __ballot(cov), b1 = __ballot(cont), b2 = __ballot(cont && trk != trk0);
        if (lane == 0) {
            if (b0) atomicAdd(&s_cnt[3 * k + 0], __popcll(b0));
            if (b1) atomicAdd(&s_cnt[3 * k + 1], __popcll(b1));
            if (b2) atomicAdd(&s_cnt[3 * k + 2], __popcll(b2));
        }
    }
    __syncthreads();
    if (threadIdx.x < 3 * T && s_cnt[threadIdx.x]) atomicAdd(&counts[threadIdx.x], s_cnt[threadIdx.x]);
}

// ---- bridged gaps (cgs_objects_track_gap) ---------------------------------------------------------------------------------------------
// Level 1 is the path above, untouched.  `prepare` then turns its result into what the levels and the table need: gap (0 / 1), each
// link's (inter, union) beside its object, and per frame the 64-bit word of open tails (objects without a successor) next to the link
// kernel's word of heads, which is the word of open heads.  Level g >= 2 is one launch of track_level_kernel; the heads words it leaves
// are the tracks' heads, so resolve, number, heads and paint run as they are, and a table kernel that reads `gap` replaces the table.
constexpr int OT_STRIDE = OT_MAX_K + 1;               // objects_match.hip, "Bank conflicts": the same table, the same two scans
constexpr int OT_CELLS = OT_MAX_K * OT_STRIDE;
static_assert(OT_CELLS % 4 == 0 && CGS_OBJ_MAX_SIDE == CGS_WAVE, "a row is one wave-wide ballot");

struct GapLayout {
    int64_t tails, link, words;
};
__host__ __device__ inline GapLayout gap_layout(int64_t n, int64_t K) {
    GapLayout o;
    o.tails = (layout(n, K).words + 1) & ~(int64_t)1;                    // 64-bit words
    o.link = o.tails + 2 * n;
    o.words = o.link + 2 * n * K;
    return o;
}

__global__ void __launch_bounds__(OT_THREADS)
track_gap_prepare_kernel(const int32_t* __restrict__ best, const int32_t* __restrict__ prev, int n, int K, int32_t* __restrict__ gap,
                         int32_t* __restrict__ link, unsigned long long* __restrict__ tails, int32_t* __restrict__ gap_links, int levels,
                         int32_t* __restrict__ extra, int64_t extra_words) {
    const int64_t step = (int64_t)gridDim.x * OT_THREADS;
    for (int64_t i = (int64_t)blockIdx.x * OT_THREADS + threadIdx.x; i < extra_words; i += step) extra[i] = 0;
    if (blockIdx.x == 0 && threadIdx.x < levels) gap_links[threadIdx.x] = 0;
    const int lane = threadIdx.x & (CGS_WAVE - 1);
    const int f = blockIdx.x * OT_WAVES + threadIdx.x / CGS_WAVE;
    const bool in = f < n && lane < K;
    bool open = false;
    if (in) {
        const int32_t* own = best + (((int64_t)f * 2 + 0) * K + lane) * 4;          // (partner in f + 1, inter, own area, partner's area)
        const int64_t i = (int64_t)f * K + lane;
        const int p = prev[i];
        gap[i] = p > 0;
        if (p > 0) {
            const int32_t* row = best + (((int64_t)(f - 1) * 2 + 1) * K + lane) * 4;
            link[2 * i] = row[1];
            link[2 * i + 1] = row[2] + row[3] - row[1];
        }
        const int q = f + 1 < n ? own[0] : 0;
        open = own[2] > 0 && !(q >= 1 && q <= K && prev[(int64_t)(f + 1) * K + q - 1] == lane + 1);
    }
    const unsigned long long word = __ballot(open);
    if (lane == 0 && f < n) tails[f] = word;
}

// One workgroup, one frame pair (a, a + g): objects_match_kernel's count and its two scans over the open tails of a and the open heads
// of a + g, every other label read as 0.  The words of frame a + g's heads and frame a's tails belong to this workgroup alone within
// the launch.  A pair with no open tail or no open head has nothing to link and reads no pixel.
//
// carried labels (MC, cgs_objects_track_mc).  The workgroup first stages frame a's labels in LDS, a byte per cell, already clamped and
// masked, and the g tables bwd[f - 1] .. bwd[a] (2 bytes a block).  A lane then walks its 16 cells q = (y, x) of frame f back along
// them (cgs_temporal_smooth_mc's path for k < 0: each step reads the table at the clamped cell; the 16 walks run side by side, so a
// step's LDS latency is paid once, not 16 times) and takes the staged label at q + m_g, 0 outside the grid, into a second plane W: a
// gather, so the count below is unchanged -- its "area of a" is now the number of cells that hold the carried label.
// The vector is constant over a block's 8 cells, so a carried run is not cut where the source run was whole.  Every read is bounded for
// any int8 field: the table index comes from a clamped cell, the label index is checked, |m| <= 9 * 128.
// At g = 1 with MC the pair is counted over every object of both frames (no words of open ends exist yet) and, instead of linking, the
// workgroup writes slot a of `best` as objects_match_kernel would: side 0 (partner, inter, TRUE own area, partner's area), side 1
// (partner, inter, own area, CARRIED area of the partner), so that the link kernel's row[2] + row[3] - row[1] is the union compared
// and every reader of best[f][0][l][2] still finds the object's area.  The true areas are counted while frame a is staged.
constexpr int OT_SIDE = CGS_TEMPORAL_SIDE;
constexpr int OT_BLOCKS = OT_SIDE / CGS_TEMPORAL_BLOCK;
constexpr int OT_MAX_LEVELS = CGS_OBJ_TRACK_MAX_GAP + 1;
constexpr int OT_ROWS = OT_SIDE / OT_WAVES;             // rows of a frame per lane
static_assert(OT_SIDE == CGS_OBJ_MAX_SIDE && CGS_TEMPORAL_BLOCK == 8 && OT_MAX_K < 256, "a staged label is a byte, a block 8 cells");

template <bool MC>
__global__ void __launch_bounds__(OT_THREADS)
track_level_kernel(const int32_t* __restrict__ labels, const int8_t* __restrict__ bwd, int h, int w, int K, int g, int iou,
                   int32_t* __restrict__ prev, int32_t* __restrict__ gap, int32_t* __restrict__ root, int32_t* __restrict__ link,
                   unsigned long long* __restrict__ heads, unsigned long long* __restrict__ tails, int32_t* __restrict__ totals,
                   int32_t* __restrict__ best) {
    __shared__ __attribute__((aligned(16))) int s_I[OT_CELLS];           // [tail - 1][head - 1], row stride 65
    __shared__ int s_A[2][OT_MAX_K];                                     // area of the tails, of the heads
    __shared__ int s_best[2][OT_MAX_K];
    __shared__ int s_true[MC ? OT_MAX_K : 1];                            // MC, g = 1: the areas of frame a's objects where they are
    __shared__ uint8_t s_L[MC ? OT_SIDE * OT_SIDE : 1];                  // MC: frame a's labels, clamped and masked
    __shared__ uint16_t s_m[MC ? OT_MAX_LEVELS : 1][OT_BLOCKS * OT_BLOCKS];      // MC: [j] = bwd[f - j - 1], dy | dx << 8
    __shared__ uint8_t s_W[MC ? OT_SIDE * OT_SIDE : 1];                  // MC: the carried labels, W of the header
    const int a = blockIdx.x, f = a + g;
    const bool pairs = MC && g == 1;                                     // level 1 of the motion path: all objects, rows of `best`
    const unsigned long long all = K >= 64 ? ~0ull : (1ull << K) - 1ull;
    const unsigned long long tmask = pairs ? all : tails[a], hmask = pairs ? all : heads[f];
    if (!tmask || !hmask) return;                                        // uniform over the workgroup
    const int x = threadIdx.x & (CGS_WAVE - 1), wave = threadIdx.x / CGS_WAVE;
    const bool live = x < w;
    const int64_t fa = (int64_t)a * h * w, ff = (int64_t)f * h * w;
    const unsigned long long upto = (2ull << x) - 1ull;

    for (int j = threadIdx.x; j < OT_CELLS / 4; j += OT_THREADS) reinterpret_cast<int4*>(s_I)[j] = make_int4(0, 0, 0, 0);
    if (threadIdx.x < 2 * OT_MAX_K) (&s_A[0][0])[threadIdx.x] = 0;
    if (MC && threadIdx.x < OT_MAX_K) s_true[threadIdx.x] = 0;
    __syncthreads();

    if constexpr (MC) {                                                  // h = w = 64 here: every lane is live
#pragma unroll
        for (int k = 0; k < (OT_MAX_LEVELS * OT_BLOCKS * OT_BLOCKS + OT_THREADS - 1) / OT_THREADS; ++k) {
            const int i = threadIdx.x + k * OT_THREADS;
            if (i < g * OT_BLOCKS * OT_BLOCKS) {
                const int8_t* m = bwd + ((int64_t)(f - 1 - (i >> 6)) * (OT_BLOCKS * OT_BLOCKS) + (i & 63)) * 2;
                s_m[i >> 6][i & 63] = (uint16_t)((uint32_t)(uint8_t)m[0] | ((uint32_t)(uint8_t)m[1] << 8));
            }
        }
        int pa[OT_ROWS];                                                 // all of a lane's loads in flight before the first is used
#pragma unroll
        for (int r = 0; r < OT_ROWS; ++r) pa[r] = labels[fa + (wave + OT_WAVES * r) * OT_SIDE + x];
#pragma unroll
        for (int r = 0; r < OT_ROWS; ++r) {
            const int y = wave + OT_WAVES * r, p = pa[r];
            const int pc = (p >= 1 && p <= K && ((tmask >> (p - 1)) & 1ull)) ? p : 0;
            s_L[y * OT_SIDE + x] = (uint8_t)pc;
            if (pairs) {                                                 // one add per run, as below
                const int left = __shfl_up(pc, 1, CGS_WAVE);
                const unsigned long long starts = __ballot(x == 0 || pc != left);
                const bool last = x == CGS_WAVE - 1 || ((starts >> (x + 1)) & 1ull);
                if (last && pc) atomicAdd(&s_true[pc - 1], x - (63 - __clzll((long long)(starts & upto))) + 1);
            }
        }
        __syncthreads();
        // the walk, all 16 rows of a lane side by side: a step is one dependent LDS read per row, and the rows do not wait for each other
        int my[OT_ROWS], mx[OT_ROWS];
#pragma unroll
        for (int r = 0; r < OT_ROWS; ++r) my[r] = mx[r] = 0;
        for (int j = 0; j < g; ++j) {
#pragma unroll
            for (int r = 0; r < OT_ROWS; ++r) {
                const int qy = min(max(wave + OT_WAVES * r + my[r], 0), OT_SIDE - 1), qx = min(max(x + mx[r], 0), OT_SIDE - 1);
                const uint32_t v = s_m[j][(qy >> 3) * OT_BLOCKS + (qx >> 3)];
                my[r] += (int)(int8_t)(v & 255u);
                mx[r] += (int)(int8_t)(v >> 8);
            }
        }
#pragma unroll
        for (int r = 0; r < OT_ROWS; ++r) {                              // W of cell (y, x): read back below by this same lane
            const int y = wave + OT_WAVES * r, sy = y + my[r], sx = x + mx[r];
            s_W[y * OT_SIDE + x] = (sy >= 0 && sy < OT_SIDE && sx >= 0 && sx < OT_SIDE) ? s_L[sy * OT_SIDE + sx] : (uint8_t)0;
        }
    }

    int pn = 0, tn = 0;
    if (live && wave < h) {
        if (!MC) pn = labels[fa + wave * w + x];
        tn = labels[ff + wave * w + x];
    }
    for (int y = wave; y < h; y += OT_WAVES) {
        int p = pn;
        const int t = tn;
        if (live && y + OT_WAVES < h) {
            if (!MC) pn = labels[fa + (y + OT_WAVES) * w + x];
            tn = labels[ff + (y + OT_WAVES) * w + x];
        }
        if constexpr (MC) p = (int)s_W[y * OT_SIDE + x];                   // the carried label: clamped and masked when it was staged
        const int pc = (p >= 1 && p <= K && ((tmask >> (p - 1)) & 1ull)) ? p : 0;
        const int tc = (t >= 1 && t <= K && ((hmask >> (t - 1)) & 1ull)) ? t : 0;
        const int key = live ? ((pc << 8) | tc) : -1;
        const int left = __shfl_up(key, 1, CGS_WAVE);
        const unsigned long long starts = __ballot(x == 0 || key != left);
        const bool last = x == CGS_WAVE - 1 || ((starts >> (x + 1)) & 1ull);
        if (live && last && key != 0) {
            const int len = x - (63 - __clzll((long long)(starts & upto))) + 1;
            if (pc) atomicAdd(&s_A[0][pc - 1], len);
            if (tc) atomicAdd(&s_A[1][tc - 1], len);
            if (pc && tc) atomicAdd(&s_I[(pc - 1) * OT_STRIDE + tc - 1], len);
        }
    }
    __syncthreads();

    const int side = wave & 1;                                           // waves 0 and 1 scan, 2 and 3 only keep the barriers
    int n_other = 64 - __clzll((long long)(side ? tmask : hmask));
    if constexpr (MC) {                                                  // the largest number on the other side that holds a cell
        const unsigned long long present = __ballot(s_A[side ^ 1][x] > 0);
        n_other = present ? 64 - __clzll((long long)present) : 0;
    }
    const int own_step = side ? 1 : OT_STRIDE, other_step = side ? OT_STRIDE : 1;
    const int own_area = s_A[side][x];
    const int* other_areas = s_A[side ^ 1];
    int bi = 0, bu = 1, bj = 0, ba = 0;
    if (wave < 2) {
        for (int j = 0; j < n_other; ++j) {
            const int inter = s_I[x * own_step + j * other_step], oa = other_areas[j];
            const int uni = own_area + oa - inter;
            if (inter > 0 && inter * bu > bi * uni) {
                bi = inter;
                bu = uni;
                bj = j + 1;
                ba = oa;
            }
        }
        s_best[side][x] = bj;
    }
    if (pairs) {                                                         // slot a of `best`; the link kernel decides
        if (wave < 2 && x < K) {
            int32_t* row = best + (((int64_t)a * 2 + side) * K + x) * 4;
            row[0] = bj;
            row[1] = bi;
            row[2] = side ? own_area : s_true[x];
            row[3] = ba;
        }
        return;
    }
    __syncthreads();
    if (wave >= 2) return;
    const bool linked = bj > 0 && s_best[side ^ 1][bj - 1] == x + 1 && 1000 * bi >= iou * bu;       // the same on both ends of a pair
    if (linked && side) {
        const int64_t i = (int64_t)f * K + x;
        prev[i] = bj;
        gap[i] = g;
        root[i] = a * K + bj - 1;
        link[2 * i] = bi;
        link[2 * i + 1] = bu;
    }
    const unsigned long long closed = __ballot(linked);
    if (x == 0 && closed) {
        if (side) {
            heads[f] = hmask & ~closed;
            atomicAdd(&totals[1], __popcll(closed));
        } else {
            tails[a] = tmask & ~closed;
        }
    }
}

// track_table_kernel with links of any gap: the link's sums lie beside the object, a bridged link adds to the track's extras, and the
// links are counted by gap.
__global__ void __launch_bounds__(OT_THREADS)
track_gap_table_kernel(const int32_t* __restrict__ best, const int32_t* __restrict__ root, const unsigned long long* __restrict__ heads,
                       const int32_t* __restrict__ base, const int32_t* __restrict__ gap, const int32_t* __restrict__ link, int n, int K,
                       int levels, int32_t* __restrict__ track, int32_t* __restrict__ tracks, int32_t* __restrict__ extra, int max_tracks,
                       int32_t* __restrict__ totals, int32_t* __restrict__ gap_links) {
    __shared__ int s_len[OT_WAVES];
    __shared__ int s_gap[CGS_OBJ_TRACK_MAX_GAP + 1];
    const int lane = threadIdx.x & (CGS_WAVE - 1), wave = threadIdx.x / CGS_WAVE;
    const int f = blockIdx.x * OT_WAVES + wave;
    const bool in = f < n && lane < K;
    if (threadIdx.x < levels) s_gap[threadIdx.x] = 0;
    __syncthreads();
    const int area = in ? best[(((int64_t)f * 2 + 0) * K + lane) * 4 + 2] : 0;
    int t = 0, len = 0, g = 0;
    if (area > 0) {
        const int64_t i = (int64_t)f * K + lane;
        const int r = root[i], fr = r / K, lr = r - fr * K;
        t = track_number(heads, base, fr, lr);
        len = f - fr + 1;
        g = gap[i];
        if (t <= max_tracks) {
            if (tracks) {
                int32_t* row = tracks + (int64_t)(t - 1) * CGS_OBJ_TRACK_FIELDS;
                atomicAdd(row + 2, 1);
                atomicAdd(row + 3, area);
                atomicMin(row + 4, area);
                atomicMax(row + 5, area);
                if (g > 0) {
                    atomicAdd(row + 6, link[2 * i]);
                    atomicAdd(row + 7, link[2 * i + 1]);
                }
            }
            if (extra && g > 1) {
                atomicAdd(extra + 2 * (int64_t)(t - 1), 1);
                atomicAdd(extra + 2 * (int64_t)(t - 1) + 1, g - 1);
            }
        }
    }
    if (in) track[(int64_t)f * K + lane] = t;
    for (int k = 1; k <= levels; ++k) {
        const unsigned long long b = __ballot(g == k);
        if (lane == 0 && b) atomicAdd(&s_gap[k - 1], __popcll(b));
    }
    len = px_wave_max(len);
    if (lane == 0) s_len[wave] = len;
    __syncthreads();
    if (threadIdx.x < levels && s_gap[threadIdx.x]) atomicAdd(gap_links + threadIdx.x, s_gap[threadIdx.x]);
    if (threadIdx.x == 0) {
        const int longest = max(max(s_len[0], s_len[1]), max(s_len[2], s_len[3]));
        if (longest > 0) atomicMax(totals + 3, longest);
    }
}

inline unsigned blocks_for(int64_t items, int per) { return (unsigned)((items + per - 1) / per); }

}  // namespace

extern "C" int64_t cgs_objects_track_scratch_bytes(int32_t n, int32_t max_objects) {
    if (n < 1 || max_objects < 1) return 0;
    const unsigned __int128 words = (unsigned __int128)n * (7u + 10u * (unsigned __int128)max_objects) + 4u;       // layout().words
    return words * 4u > (unsigned __int128)INT64_MAX ? INT64_MAX : (int64_t)(words * 4u);        // saturates: no buffer is that large
}

extern "C" int cgs_objects_track(const int32_t* labels, int32_t n, int32_t h, int32_t w, int32_t max_objects, int32_t iou_milli,
                                 int32_t max_tracks, int32_t* prev, int32_t* track, int32_t* totals, int32_t* tracks,
                                 int32_t* track_labels, uint8_t* rgb, void* scratch, int64_t scratch_bytes, cgs_stream_t stream_) {
    if (!labels || !prev || !track || !totals || !scratch || n < 1 || h < 1 || w < 1 || max_objects < 1 || max_tracks < 1 ||
        iou_milli < 1 || iou_milli > 1000 || ((uintptr_t)labels & 3u) || ((uintptr_t)prev & 3u) || ((uintptr_t)track & 3u) ||
        ((uintptr_t)totals & 3u) || ((uintptr_t)tracks & 3u) || ((uintptr_t)track_labels & 3u) || ((uintptr_t)scratch & 7u) ||
        scratch_bytes < cgs_objects_track_scratch_bytes(n, max_objects))
        return CGS_ERR_BADARG;
    if (h > CGS_OBJ_MAX_SIDE || w > CGS_OBJ_MAX_SIDE || max_objects > OT_MAX_K || n > CGS_OBJ_TRACK_MAX_FRAMES) return CGS_ERR_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    const int K = max_objects, hw = h * w;
    const Layout o = layout(n, K);
    int32_t* s = static_cast<int32_t*>(scratch);
    int32_t *milli = s + o.milli, *counts = s + o.counts, *best = s + o.best, *root_a = s + o.root_a, *root_b = s + o.root_b,
            *base = s + o.base;
    unsigned long long* heads = reinterpret_cast<unsigned long long*>(s + o.heads);
    const unsigned frames4 = blocks_for(n, OT_WAVES);

    const int64_t words = tracks ? (int64_t)max_tracks * CGS_OBJ_TRACK_FIELDS : 0;
    const int64_t want_blocks = (words + OT_THREADS - 1) / OT_THREADS;
    const unsigned init_blocks = (unsigned)(want_blocks < 1 ? 1 : want_blocks > 4096 ? 4096 : want_blocks);
    hipLaunchKernelGGL(track_init_kernel, dim3(init_blocks), dim3(OT_THREADS), 0, stream, tracks, words, totals, milli, (int)iou_milli);
    CGS_HIP_CHECK_LAUNCH();
    if (n > 1) {
        const int rc = cgs_objects_match(labels, labels + hw, n - 1, h, w, K, milli, 1, counts, best, stream_);
        if (rc != CGS_OK) return rc;
    }
    const int32_t* last = labels + (int64_t)(n - 1) * hw;
    const int rc = cgs_objects_match(last, last, 1, h, w, K, milli, 1, counts + 4 * (int64_t)(n - 1), best + 8 * (int64_t)(n - 1) * K, stream_);
    if (rc != CGS_OK) return rc;
    hipLaunchKernelGGL(track_link_kernel, dim3(frames4), dim3(OT_THREADS), 0, stream, best, (int)n, K, (int)iou_milli, prev, root_a, heads,
                       totals);
    CGS_HIP_CHECK_LAUNCH();
    const int total = n * K;
    for (int reach = 1; reach < n - 1; reach <<= 1) {                     // R rounds, 2^R >= n - 1
        hipLaunchKernelGGL(track_resolve_kernel, dim3(blocks_for(total, OT_THREADS)), dim3(OT_THREADS), 0, stream, root_a, root_b, total);
        CGS_HIP_CHECK_LAUNCH();
        int32_t* swap = root_a;
        root_a = root_b;
        root_b = swap;
    }
    hipLaunchKernelGGL(track_number_kernel, dim3(1), dim3(OT_SCAN_THREADS), 0, stream, heads, (int)n, base, totals);
    CGS_HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(track_heads_kernel, dim3(frames4), dim3(OT_THREADS), 0, stream, best, heads, base, (int)n, K,
                       tracks, tracks ? (int)max_tracks : 0);
    CGS_HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(track_table_kernel, dim3(frames4), dim3(OT_THREADS), 0, stream, best, root_a, heads, base, prev, (int)n, K, track,
                       tracks, (int)max_tracks, totals);
    CGS_HIP_CHECK_LAUNCH();
    const int64_t pixels = (int64_t)n * hw;
    hipLaunchKernelGGL(track_paint_kernel, dim3(blocks_for(pixels, OT_THREADS)), dim3(OT_THREADS), 0, stream, labels, track, pixels, hw, K,
                       track_labels, rgb);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}

extern "C" int cgs_objects_track_switches(const int32_t* truth_prev, const int32_t* pred_track, const int32_t* match_best,
                                          const int32_t* iou_milli, int32_t T, int32_t n, int32_t max_objects, int32_t* counts,
                                          cgs_stream_t stream_) {
    if (!truth_prev || !pred_track || !match_best || !iou_milli || !counts || T < 1 || T > CGS_OBJ_MATCH_MAX_IOU || n < 1 ||
        max_objects < 1 || ((uintptr_t)truth_prev & 3u) || ((uintptr_t)pred_track & 3u) || ((uintptr_t)match_best & 3u) ||
        ((uintptr_t)iou_milli & 3u) || ((uintptr_t)counts & 3u))
        return CGS_ERR_BADARG;
    if (max_objects > OT_MAX_K || n > CGS_OBJ_TRACK_MAX_FRAMES) return CGS_ERR_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    const hipError_t e = hipMemsetAsync(counts, 0, sizeof(int32_t) * 3 * (size_t)T, stream);
    if (e != hipSuccess) return (int)e;
    hipLaunchKernelGGL(track_switches_kernel, dim3(blocks_for(n, OT_WAVES)), dim3(OT_THREADS), 0, stream, truth_prev, pred_track,
                       match_best, iou_milli, (int)T, (int)n, (int)max_objects, counts);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}

extern "C" int64_t cgs_objects_track_gap_scratch_bytes(int32_t n, int32_t max_objects, int32_t max_gap) {
    if (n < 1 || max_objects < 1 || max_gap < 0 || max_gap > CGS_OBJ_TRACK_MAX_GAP) return 0;
    // gap_layout().words: layout().words rounded up to even, then 2 n + 2 n K
    const unsigned __int128 N = (unsigned __int128)n, K = (unsigned __int128)max_objects;
    const unsigned __int128 words = ((N * (7u + 10u * K) + 4u + 1u) & ~(unsigned __int128)1) + 2u * N + 2u * N * K;
    return words * 4u > (unsigned __int128)INT64_MAX ? INT64_MAX : (int64_t)(words * 4u);
}

namespace {

// What cgs_objects_track_gap and cgs_objects_track_mc launch once their arguments are checked; bwd NULL: no motion.
// Launches: init, match or the level-1 count (n > 1), self-match, link, prepare, min(G, n - 1) levels, R x resolve, number, heads,
// table, paint: 8 + R + (n > 1) + min(G, n - 1), a function of n and G alone.
int track_gap_run(const int32_t* labels, const int8_t* bwd, int32_t n, int32_t h, int32_t w, int32_t max_objects, int32_t iou_milli,
                  int32_t max_gap, int32_t max_tracks, int32_t* prev, int32_t* gap, int32_t* track, int32_t* totals, int32_t* gap_links,
                  int32_t* tracks, int32_t* tracks_extra, int32_t* track_labels, uint8_t* rgb, void* scratch, cgs_stream_t stream_) {
    hipStream_t stream = (hipStream_t)stream_;
    const int K = max_objects, hw = h * w, levels = max_gap + 1;
    const Layout o = layout(n, K);
    const GapLayout go = gap_layout(n, K);
    int32_t* s = static_cast<int32_t*>(scratch);
    int32_t *milli = s + o.milli, *counts = s + o.counts, *best = s + o.best, *root_a = s + o.root_a, *root_b = s + o.root_b,
            *base = s + o.base, *link = s + go.link;
    unsigned long long* heads = reinterpret_cast<unsigned long long*>(s + o.heads);
    unsigned long long* tails = reinterpret_cast<unsigned long long*>(s + go.tails);
    const unsigned frames4 = blocks_for(n, OT_WAVES);

    const int64_t words = tracks ? (int64_t)max_tracks * CGS_OBJ_TRACK_FIELDS : 0;
    const int64_t want_blocks = (words + OT_THREADS - 1) / OT_THREADS;
    const unsigned init_blocks = (unsigned)(want_blocks < 1 ? 1 : want_blocks > 4096 ? 4096 : want_blocks);
    hipLaunchKernelGGL(track_init_kernel, dim3(init_blocks), dim3(OT_THREADS), 0, stream, tracks, words, totals, milli, (int)iou_milli);
    CGS_HIP_CHECK_LAUNCH();
    if (n > 1 && bwd) {                                                   // level 1 along the field: slots 0 .. n - 2 of `best`
        hipLaunchKernelGGL(track_level_kernel<true>, dim3((unsigned)(n - 1)), dim3(OT_THREADS), 0, stream, labels, bwd, (int)h, (int)w, K, 1,
                           (int)iou_milli, prev, gap, root_a, link, heads, tails, totals, best);
        CGS_HIP_CHECK_LAUNCH();
    } else if (n > 1) {
        const int rc = cgs_objects_match(labels, labels + hw, n - 1, h, w, K, milli, 1, counts, best, stream_);
        if (rc != CGS_OK) return rc;
    }
    const int32_t* last = labels + (int64_t)(n - 1) * hw;
    const int rc = cgs_objects_match(last, last, 1, h, w, K, milli, 1, counts + 4 * (int64_t)(n - 1), best + 8 * (int64_t)(n - 1) * K, stream_);
    if (rc != CGS_OK) return rc;
    hipLaunchKernelGGL(track_link_kernel, dim3(frames4), dim3(OT_THREADS), 0, stream, best, (int)n, K, (int)iou_milli, prev, root_a, heads,
                       totals);
    CGS_HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(track_gap_prepare_kernel, dim3(frames4), dim3(OT_THREADS), 0, stream, best, prev, (int)n, K, gap, link, tails,
                       gap_links, levels, tracks_extra, tracks_extra ? 2 * (int64_t)max_tracks : (int64_t)0);
    CGS_HIP_CHECK_LAUNCH();
    for (int g = 2; g <= levels && g <= n - 1; ++g) {                     // a level with no frame pair launches nothing
        if (bwd)
            hipLaunchKernelGGL(track_level_kernel<true>, dim3((unsigned)(n - g)), dim3(OT_THREADS), 0, stream, labels, bwd, (int)h, (int)w, K,
                               g, (int)iou_milli, prev, gap, root_a, link, heads, tails, totals, best);
        else
            hipLaunchKernelGGL(track_level_kernel<false>, dim3((unsigned)(n - g)), dim3(OT_THREADS), 0, stream, labels, bwd, (int)h, (int)w, K,
                               g, (int)iou_milli, prev, gap, root_a, link, heads, tails, totals, best);
        CGS_HIP_CHECK_LAUNCH();
    }
    const int total = n * K;
    for (int reach = 1; reach < n - 1; reach <<= 1) {                     // R rounds, 2^R >= n - 1: a bridged root points further back
        hipLaunchKernelGGL(track_resolve_kernel, dim3(blocks_for(total, OT_THREADS)), dim3(OT_THREADS), 0, stream, root_a, root_b, total);
        CGS_HIP_CHECK_LAUNCH();
        int32_t* swap = root_a;
        root_a = root_b;
        root_b = swap;
    }
    hipLaunchKernelGGL(track_number_kernel, dim3(1), dim3(OT_SCAN_THREADS), 0, stream, heads, (int)n, base, totals);
    CGS_HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(track_heads_kernel, dim3(frames4), dim3(OT_THREADS), 0, stream, best, heads, base, (int)n, K,
                       tracks, tracks ? (int)max_tracks : 0);
    CGS_HIP_CHECK_LAUNCH();
    hipLaunchKernelGGL(track_gap_table_kernel, dim3(frames4), dim3(OT_THREADS), 0, stream, best, root_a, heads, base, gap, link, (int)n, K,
                       levels, track, tracks, tracks_extra, (int)max_tracks, totals, gap_links);
    CGS_HIP_CHECK_LAUNCH();
    const int64_t pixels = (int64_t)n * hw;
    hipLaunchKernelGGL(track_paint_kernel, dim3(blocks_for(pixels, OT_THREADS)), dim3(OT_THREADS), 0, stream, labels, track, pixels, hw, K,
                       track_labels, rgb);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}

}  // namespace

extern "C" int cgs_objects_track_gap(const int32_t* labels, int32_t n, int32_t h, int32_t w, int32_t max_objects, int32_t iou_milli,
                                     int32_t max_gap, int32_t max_tracks, int32_t* prev, int32_t* gap, int32_t* track, int32_t* totals,
                                     int32_t* gap_links, int32_t* tracks, int32_t* tracks_extra, int32_t* track_labels, uint8_t* rgb,
                                     void* scratch, int64_t scratch_bytes, cgs_stream_t stream_) {
    if (!labels || !prev || !gap || !track || !totals || !gap_links || !scratch || n < 1 || h < 1 || w < 1 || max_objects < 1 ||
        max_tracks < 1 || iou_milli < 1 || iou_milli > 1000 || max_gap < 0 || max_gap > CGS_OBJ_TRACK_MAX_GAP ||
        ((uintptr_t)labels & 3u) || ((uintptr_t)prev & 3u) || ((uintptr_t)gap & 3u) || ((uintptr_t)track & 3u) ||
        ((uintptr_t)totals & 3u) || ((uintptr_t)gap_links & 3u) || ((uintptr_t)tracks & 3u) || ((uintptr_t)tracks_extra & 3u) ||
        ((uintptr_t)track_labels & 3u) || ((uintptr_t)scratch & 7u) ||
        scratch_bytes < cgs_objects_track_gap_scratch_bytes(n, max_objects, max_gap))
        return CGS_ERR_BADARG;
    if (h > CGS_OBJ_MAX_SIDE || w > CGS_OBJ_MAX_SIDE || max_objects > OT_MAX_K || n > CGS_OBJ_TRACK_MAX_FRAMES) return CGS_ERR_UNSUPPORTED;
    return track_gap_run(labels, nullptr, n, h, w, max_objects, iou_milli, max_gap, max_tracks, prev, gap, track, totals, gap_links, tracks,
                         tracks_extra, track_labels, rgb, scratch, stream_);
}

// The scratch is cgs_objects_track_gap's: the carried labels live in LDS.
extern "C" int64_t cgs_objects_track_mc_scratch_bytes(int32_t n, int32_t max_objects, int32_t max_gap) {
    return cgs_objects_track_gap_scratch_bytes(n, max_objects, max_gap);
}

extern "C" int cgs_objects_track_mc(const int32_t* labels, const int8_t* bwd, int32_t n, int32_t h, int32_t w, int32_t max_objects,
                                    int32_t iou_milli, int32_t max_gap, int32_t max_tracks, int32_t* prev, int32_t* gap, int32_t* track,
                                    int32_t* totals, int32_t* gap_links, int32_t* tracks, int32_t* tracks_extra, int32_t* track_labels,
                                    uint8_t* rgb, void* scratch, int64_t scratch_bytes, cgs_stream_t stream_) {
    if (!labels || (!bwd && n != 1) || !prev || !gap || !track || !totals || !gap_links || !scratch || n < 1 || h < 1 || w < 1 ||
        max_objects < 1 || max_tracks < 1 || iou_milli < 1 || iou_milli > 1000 || max_gap < 0 || max_gap > CGS_OBJ_TRACK_MAX_GAP ||
        ((uintptr_t)labels & 3u) || ((uintptr_t)prev & 3u) || ((uintptr_t)gap & 3u) || ((uintptr_t)track & 3u) ||
        ((uintptr_t)totals & 3u) || ((uintptr_t)gap_links & 3u) || ((uintptr_t)tracks & 3u) || ((uintptr_t)tracks_extra & 3u) ||
        ((uintptr_t)track_labels & 3u) || ((uintptr_t)scratch & 7u) ||
        scratch_bytes < cgs_objects_track_mc_scratch_bytes(n, max_objects, max_gap))
        return CGS_ERR_BADARG;
    if (h != OT_SIDE || w != OT_SIDE || max_objects > OT_MAX_K || n > CGS_OBJ_TRACK_MAX_FRAMES) return CGS_ERR_UNSUPPORTED;
    return track_gap_run(labels, bwd, n, h, w, max_objects, iou_milli, max_gap, max_tracks, prev, gap, track, totals, gap_links, tracks,
                         tracks_extra, track_labels, rgb, scratch, stream_);
}
