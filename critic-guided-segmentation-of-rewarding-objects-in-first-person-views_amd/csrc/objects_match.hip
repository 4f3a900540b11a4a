// From two label maps to matched objects: every predicted object of a frame intersected with every truth object, the pair of largest
// IoU per object from both sides, and per IoU threshold the number of objects with a match (cgs_objects_match, include/cgs_hip.h).
// One workgroup of four waves takes one frame of at most 64 x 64 pixels; the K x K intersection table and the two area vectors live in
// LDS, everything is integer and the only atomics are LDS integer adds, so the result does not depend on the order of anything below.
//
//   1. count     a lane is a column and a wave takes the rows wave, wave + 4, ... (as objects.hip).  A label outside 1..K counts as 0
//                here.  One __ballot of "my (pred, truth) pair differs from my left neighbour's" gives the row's run boundaries; the
//                last lane of a run adds the run's length to area_p, area_t and the (p, t) cell, whichever exist -- one LDS add per run
//                and target, so a full frame of one object against itself is 64 adds per target, not 4096.  Lanes at and beyond w carry
//                a pair no pixel can have and add nothing: the run before them ends at w - 1, and lane 0 always starts a run, so the
//                end of one row and the start of the next never form one.  Each lane also keeps the largest raw label it saw.
//   2. match     wave 0 takes the predicted side, wave 1 the truth side; a lane is one object of its side and scans the objects of the
//                other side in ascending order, keeping the pair of largest IoU (inter_a union_b > inter_b union_a: at most 2^12 2^13,
//                exact in int32; strictly larger only, so ties stay with the smallest number).  An object has a match at threshold m
//                exactly when its best pair reaches m, so the T counts are T ballots and popcounts of 1000 inter >= m union.
//
// Bank conflicts: the table's row stride is padded from 64 to 65 words.  The predicted side reads I[lane][j] (bank (lane + j) mod 32,
// distinct within each half wave), the truth side I[j][lane] (consecutive words); at stride 64 the first would be one bank for all
// lanes.  Padding serves both scans with one layout and keeps the index a multiply-add; a rotated start would need a wrap per step
// and would make "ties go to the smallest number" a second comparison.
//
// LDS: 64 x 65 + 2 x 64 + 8 words = 16.8 KiB, so the 32-wave limit (eight workgroups per CU), not LDS, bounds occupancy.
#include "pixel_common.h"

namespace {

constexpr int OM_THREADS = 256;
constexpr int OM_WAVES = OM_THREADS / CGS_WAVE;
constexpr int OM_MAX_SIDE = CGS_OBJ_MAX_SIDE;         // a row is one wave-wide ballot
constexpr int OM_MAX_K = CGS_OBJ_MATCH_MAX_OBJECTS;   // a lane is an object in step 2
constexpr int OM_STRIDE = OM_MAX_K + 1;               // see "Bank conflicts" above
constexpr int OM_CELLS = OM_MAX_K * OM_STRIDE;        // 4160, a multiple of 4
static_assert(OM_MAX_K == CGS_WAVE && OM_MAX_SIDE == CGS_WAVE && OM_CELLS % 4 == 0, "one lane per column and per object");

__global__ void __launch_bounds__(OM_THREADS)
objects_match_kernel(const int32_t* __restrict__ pred, const int32_t* __restrict__ truth, int h, int w, int K,
                     const int32_t* __restrict__ iou_milli, int T, int32_t* __restrict__ counts, int32_t* __restrict__ best) {
    __shared__ __attribute__((aligned(16))) int s_I[OM_CELLS];          // [p - 1][t - 1], row stride 65
    __shared__ int s_A[2][OM_MAX_K];                                    // area_p, area_t
    __shared__ int s_max[OM_WAVES][2];
    const int x = threadIdx.x & (CGS_WAVE - 1), wave = threadIdx.x / CGS_WAVE;
    const bool live = x < w;
    const int64_t frame = (int64_t)blockIdx.x * h * w;
    const unsigned long long upto = (2ull << x) - 1ull;                // bits 0..x

    for (int j = threadIdx.x; j < OM_CELLS / 4; j += OM_THREADS) reinterpret_cast<int4*>(s_I)[j] = make_int4(0, 0, 0, 0);
    if (threadIdx.x < 2 * OM_MAX_K) (&s_A[0][0])[threadIdx.x] = 0;
    __syncthreads();

    // 1. count, one add per run and target; the next row's labels are requested before this row's adds
    int pmax = 0, tmax = 0, pn = 0, tn = 0;
    if (live && wave < h) {
        pn = pred[frame + wave * w + x];
        tn = truth[frame + wave * w + x];
    }
    for (int y = wave; y < h; y += OM_WAVES) {
        const int p = pn, t = tn;
        if (live && y + OM_WAVES < h) {
            pn = pred[frame + (y + OM_WAVES) * w + x];
            tn = truth[frame + (y + OM_WAVES) * w + x];
        }
        pmax = max(pmax, p);                                             // p = t = 0 in the lanes at and beyond w
        tmax = max(tmax, t);
        const int pc = (p >= 1 && p <= K) ? p : 0, tc = (t >= 1 && t <= K) ? t : 0;
        const int key = live ? ((pc << 8) | tc) : -1;
        const int left = __shfl_up(key, 1, CGS_WAVE);
        const unsigned long long starts = __ballot(x == 0 || key != left);      // bit 0 is always set
        const bool last = x == CGS_WAVE - 1 || ((starts >> (x + 1)) & 1ull);
        if (live && last && key != 0) {
            const int len = x - (63 - __clzll((long long)(starts & upto))) + 1;
            if (pc) atomicAdd(&s_A[0][pc - 1], len);
            if (tc) atomicAdd(&s_A[1][tc - 1], len);
            if (pc && tc) atomicAdd(&s_I[(pc - 1) * OM_STRIDE + tc - 1], len);
        }
    }
    pmax = px_wave_max(pmax);
    tmax = px_wave_max(tmax);
    if (x == 0) {
        s_max[wave][0] = pmax;
        s_max[wave][1] = tmax;
    }
    __syncthreads();

    // 2. match: wave 0 the predicted objects against the truth objects, wave 1 the other way round
    if (wave >= 2) return;
    const int side = wave;
    pmax = max(max(s_max[0][0], s_max[1][0]), max(s_max[2][0], s_max[3][0]));
    tmax = max(max(s_max[0][1], s_max[1][1]), max(s_max[2][1], s_max[3][1]));
    const int n_own = min(side ? tmax : pmax, K), n_other = min(side ? pmax : tmax, K);
    const int own_step = side ? 1 : OM_STRIDE, other_step = side ? OM_STRIDE : 1;
    const int own_area = s_A[side][x];
    const int* other_areas = s_A[side ^ 1];
    const bool active = x < n_own;
    int bi = 0, bu = 1, bj = 0, ba = 0;                                  // the best pair: inter, union, number, area of the other
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
    int32_t* cnt = counts + (int64_t)blockIdx.x * (2 + 2 * T);
    if (x == 0 && side == 0) {
        cnt[0] = pmax;
        cnt[1] = tmax;
    }
    for (int k = 0; k < T; ++k) {
        const int m = iou_milli[k];
        const unsigned long long hit = __ballot(active && bi > 0 && 1000 * bi >= m * bu);
        if (x == 0) cnt[2 + 2 * k + side] = __popcll(hit);
    }
    if (best && x < K) {
        int32_t* row = best + (((int64_t)blockIdx.x * 2 + side) * K + x) * 4;
        row[0] = active ? bj : 0;
        row[1] = active ? bi : 0;
        row[2] = active ? own_area : 0;
        row[3] = active ? ba : 0;
    }
}

}  // namespace

extern "C" int cgs_objects_match(const int32_t* pred, const int32_t* truth, int32_t n, int32_t h, int32_t w, int32_t max_objects,
                                 const int32_t* iou_milli, int32_t T, int32_t* counts, int32_t* best, cgs_stream_t stream_) {
    if (!pred || !truth || !iou_milli || !counts || n < 1 || h < 1 || w < 1 || max_objects < 1 || T < 1 ||
        T > CGS_OBJ_MATCH_MAX_IOU || ((uintptr_t)pred & 3u) || ((uintptr_t)truth & 3u) || ((uintptr_t)iou_milli & 3u) ||
        ((uintptr_t)counts & 3u) || ((uintptr_t)best & 3u))
        return CGS_ERR_BADARG;
    if (h > OM_MAX_SIDE || w > OM_MAX_SIDE || max_objects > OM_MAX_K) return CGS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(objects_match_kernel, dim3((unsigned)n), dim3(OM_THREADS), 0, (hipStream_t)stream_, pred, truth, (int)h, (int)w,
                       (int)max_objects, iou_milli, (int)T, counts, best);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}
