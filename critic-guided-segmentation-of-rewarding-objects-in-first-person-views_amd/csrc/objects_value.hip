// The value of an object (cgs_objects_ablate, cgs_objects_select; the rule is their header comment in include/cgs_hip.h): the batch of
// "this frame without object k" images that the critic is asked about, built where the frames and the labels are, and the selection
// that drops the objects that fail a value threshold and renumbers the rest.  Both are integer or pure selection throughout, so the
// result does not depend on the order in which anything below happens.
//
// ablate_kernel: one workgroup of four waves per frame of the range.
//   1. stage     the frame's 12288 bytes as 768 16-byte pieces, three a thread (piece c = thread + 256 j: a wave's loads and stores are
//                1 KiB contiguous), kept in registers for every row; with the mean fill also written to LDS.  The labels become ONE-HOT
//                64-bit words in LDS, D[cell] = 1 << (label - 1) for a label in 1..K and 0 otherwise -- not bytes: the grow test then
//                costs two passes per FRAME instead of a window scan per row, and "is this cell replaced in row k" is bit k - 1
//   2. mean      (fill mode 2) channel sums and count over the cells of label 0, or over all cells when there are none: a per-thread
//                partial over 16 cells, a wave reduction, one LDS atomic per wave and figure
//   3. grow      D[y][x] |= its neighbours within R along x, then along y, in place (read to registers, barrier, write): the OR over
//                the clipped (2R+1)^2 square, for all 64 objects at once
//   4. rows      a piece holds the bytes of at most 6 cells; their 6 words stay in registers as 32-bit halves.  Row k takes bit k - 1 of
//                each, spreads the 6 bits to a 16-bit byte mask by the piece's phase (16 c mod 3), the byte mask to four 32-bit word masks,
//                and writes (frame & ~mask) | (fill & mask) with one 16-byte store.  About 40 vector instructions per 16-byte store: the
//                kernel is bound by its writes, 12 KiB a row
// LDS: 32 KiB (D) + 12 KiB (frame bytes, mean fill) + 32 B = 44 KiB, three workgroups per CU.
//
// select_kernel: one workgroup per frame.  Wave 0 makes the remap table: lane j speaks for old label j + 1, one ballot of "kept and
// scored", new label = 1 + popcount of the kept lanes below.  Everything else is a gather through the 65-entry table in LDS.
#include "cgs_common.h"

namespace {

constexpr int VAL_THREADS = 256;
constexpr int VAL_SIDE = 64;
constexpr int VAL_CELLS = VAL_SIDE * VAL_SIDE;
constexpr int VAL_BYTES = VAL_CELLS * 3;                 // 12288 = 768 pieces of 16 bytes
constexpr int VAL_PIECES = VAL_BYTES / 16 / VAL_THREADS; // 3 a thread
constexpr int VAL_CELLS_PER_THREAD = VAL_CELLS / VAL_THREADS;   // 16: rows wave, wave + 4, ... of column lane
constexpr int VAL_MAX_GROW = CGS_OBJ_VALUE_MAX_GROW;
constexpr int VAL_FIELDS = 8;

__device__ __forceinline__ uint32_t spread4(uint32_t nibble) {
    // bit i of the nibble -> 0xFF in byte i: the 16 partial products of the multiply land on 16 different bits, so nothing carries
    return ((nibble * 0x00204081u) & 0x01010101u) * 0xFFu;
}

__global__ void __launch_bounds__(VAL_THREADS)
ablate_kernel(const uint8_t* __restrict__ frames, const int32_t* __restrict__ labels, const int32_t* __restrict__ offsets, int f0,
              int max_objects, int grow, int fill_mode, uint32_t fill_rgb, const uint8_t* __restrict__ fill, int64_t fill_stride,
              int64_t rows_total, uint8_t* __restrict__ out, int32_t* __restrict__ row_frame, int32_t* __restrict__ row_label) {
    __shared__ unsigned long long s_D[VAL_CELLS];
    __shared__ uint4 s_frame[VAL_BYTES / 16];
    __shared__ int s_sum[8];                          // S_r, S_g, S_b, N over label 0; the same over all cells
    const int f = f0 + (int)blockIdx.x, tid = threadIdx.x, x = tid & (CGS_WAVE - 1), wave = tid / CGS_WAVE;
    const int64_t base = (int64_t)offsets[f] - (int64_t)offsets[f0];
    const int rows = min(max(offsets[f + 1] - offsets[f], 0), max_objects);      // (the same for every thread: a uniform exit)
    if (rows == 0) return;
    const uint4* src = reinterpret_cast<const uint4*>(frames + (int64_t)f * VAL_BYTES);
    const int32_t* lab = labels + (int64_t)f * VAL_CELLS;

    // 1. stage
    uint4 own[VAL_PIECES];
#pragma unroll
    for (int j = 0; j < VAL_PIECES; ++j) own[j] = src[tid + VAL_THREADS * j];
    int raw[VAL_CELLS_PER_THREAD];
#pragma unroll
    for (int i = 0; i < VAL_CELLS_PER_THREAD; ++i) {
        raw[i] = lab[tid + VAL_THREADS * i];
        s_D[tid + VAL_THREADS * i] = (raw[i] >= 1 && raw[i] <= max_objects) ? 1ull << (raw[i] - 1) : 0ull;
    }
    if (fill_mode == 2) {
#pragma unroll
        for (int j = 0; j < VAL_PIECES; ++j) s_frame[tid + VAL_THREADS * j] = own[j];
        if (tid < 8) s_sum[tid] = 0;
    }
    __syncthreads();

    // 2. mean
    uint32_t colour = fill_rgb;                        // R | G << 8 | B << 16
    if (fill_mode == 2) {
        const uint8_t* bytes = reinterpret_cast<const uint8_t*>(s_frame);
        int part[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < VAL_CELLS_PER_THREAD; ++i) {
            const int cell = tid + VAL_THREADS * i, bg = raw[i] == 0;
#pragma unroll
            for (int ch = 0; ch < 3; ++ch) {
                const int v = bytes[3 * cell + ch];
                part[ch] += bg ? v : 0;
                part[4 + ch] += v;
            }
            part[3] += bg;
        }
        part[7] = VAL_CELLS_PER_THREAD;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            int v = part[q];
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, CGS_WAVE);
            if (x == 0) atomicAdd(&s_sum[q], v);
        }
        __syncthreads();
        const int o = s_sum[3] > 0 ? 0 : 4, N = s_sum[o + 3];                    // N = 4096 when no cell has label 0
        colour = 0;
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) colour |= (uint32_t)((2 * s_sum[o + ch] + N) / (2 * N)) << (8 * ch);   // at most 255: S <= 255 N
    }

    // 3. grow, along x and then along y
    if (grow > 0) {
        unsigned long long acc[VAL_CELLS_PER_THREAD];
#pragma unroll
        for (int i = 0; i < VAL_CELLS_PER_THREAD; ++i) {
            const int y = wave + 4 * i;
            unsigned long long v = 0ull;
            for (int d = -grow; d <= grow; ++d)
                if (x + d >= 0 && x + d < VAL_SIDE) v |= s_D[y * VAL_SIDE + x + d];
            acc[i] = v;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < VAL_CELLS_PER_THREAD; ++i) s_D[(wave + 4 * i) * VAL_SIDE + x] = acc[i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < VAL_CELLS_PER_THREAD; ++i) {
            const int y = wave + 4 * i;
            unsigned long long v = 0ull;
            for (int d = -grow; d <= grow; ++d)
                if (y + d >= 0 && y + d < VAL_SIDE) v |= s_D[(y + d) * VAL_SIDE + x];
            acc[i] = v;
        }
        __syncthreads();
#pragma unroll
        for (int i = 0; i < VAL_CELLS_PER_THREAD; ++i) s_D[(wave + 4 * i) * VAL_SIDE + x] = acc[i];
        __syncthreads();
    }

    // 4. rows.  Piece c starts at byte 16 c = channel p of cell q0, p = 16 c mod 3 = c mod 3; byte i lies in cell q0 + (p + i) / 3, and
    // the piece's last byte lies in cell q0 + 5, so q0 + 5 <= 4095 for every piece
    uint32_t lo[VAL_PIECES][6], hi[VAL_PIECES][6], pat[VAL_PIECES][6];
    uint4 fillv[VAL_PIECES];
#pragma unroll
    for (int j = 0; j < VAL_PIECES; ++j) {
        const int c = tid + VAL_THREADS * j, q0 = (16 * c) / 3, p = (16 * c) % 3;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
            const unsigned long long v = s_D[q0 + q];
            lo[j][q] = (uint32_t)v;
            hi[j][q] = (uint32_t)(v >> 32);
            const int s = 3 * q - p;                                             // the cell's first byte in the piece, -2 .. 15
            pat[j][q] = (s >= 0 ? 7u << s : 7u >> -s) & 0xFFFFu;
        }
        if (fill_mode == 1) {
            fillv[j] = reinterpret_cast<const uint4*>(fill + (int64_t)f * fill_stride)[c];
        } else {
            // byte i is channel (p + i) mod 3: the 12-byte period R G B R G B R G B R G B, rotated by p, then its first 4 bytes again
            const uint32_t r = colour & 255u, g = (colour >> 8) & 255u, b = (colour >> 16) & 255u;
            const uint32_t c0 = p == 0 ? r : (p == 1 ? g : b), c1 = p == 0 ? g : (p == 1 ? b : r), c2 = p == 0 ? b : (p == 1 ? r : g);
            const uint32_t w0 = c0 | c1 << 8 | c2 << 16 | c0 << 24, w1 = c1 | c2 << 8 | c0 << 16 | c1 << 24,
                           w2 = c2 | c0 << 8 | c1 << 16 | c2 << 24;
            fillv[j] = make_uint4(w0, w1, w2, w0);
        }
    }
    if (tid < rows && base + tid >= 0 && base + tid < rows_total) {
        row_frame[base + tid] = f;
        row_label[base + tid] = tid + 1;
    }
    for (int k = 0; k < rows; ++k) {
        const int64_t row = base + k;
        if (row < 0 || row >= rows_total) continue;                              // offsets that do not fit the output write nothing
        uint4* dst = reinterpret_cast<uint4*>(out + row * VAL_BYTES);
        const int sh = k & 31;
#pragma unroll
        for (int j = 0; j < VAL_PIECES; ++j) {
            uint32_t sel = 0;
#pragma unroll
            for (int q = 0; q < 6; ++q) {
                const uint32_t word = k < 32 ? lo[j][q] : hi[j][q];              // k is uniform: no divergence
                sel |= ((word >> sh) & 1u) ? pat[j][q] : 0u;
            }
            const uint32_t m0 = spread4(sel & 15u), m1 = spread4((sel >> 4) & 15u), m2 = spread4((sel >> 8) & 15u),
                           m3 = spread4((sel >> 12) & 15u);
            dst[tid + VAL_THREADS * j] = make_uint4((own[j].x & ~m0) | (fillv[j].x & m0), (own[j].y & ~m1) | (fillv[j].y & m1),
                                                    (own[j].z & ~m2) | (fillv[j].z & m2), (own[j].w & ~m3) | (fillv[j].w & m3));
        }
    }
}

__global__ void __launch_bounds__(VAL_THREADS)
select_kernel(const int32_t* __restrict__ labels, const int32_t* __restrict__ table, const int32_t* __restrict__ kept,
              const uint8_t* __restrict__ keep, int cells, int max_objects, int32_t* __restrict__ out_labels,
              int32_t* __restrict__ out_table, int32_t* __restrict__ out_kept, uint8_t* __restrict__ mask, int32_t* __restrict__ unscored) {
    __shared__ int s_map[CGS_WAVE + 1];
    __shared__ int s_kept;
    const int f = blockIdx.x, tid = threadIdx.x, K = max_objects;
    const int have = max(kept[f], 0), limit = min(have, K);
    if (tid < CGS_WAVE) {
        const bool on = tid < limit && keep[(int64_t)f * K + tid] != 0;
        const unsigned long long m = __ballot(on);
        s_map[tid + 1] = on ? 1 + __popcll(m & ((1ull << tid) - 1ull)) : 0;
        if (tid == 0) {
            s_map[0] = 0;
            s_kept = __popcll(m);
            out_kept[f] = __popcll(m);
            unscored[f] = have - limit;
        }
    }
    __syncthreads();
    const int64_t frame = (int64_t)f * cells;
    for (int p = tid; p < cells; p += VAL_THREADS) {
        const int l = labels[frame + p];
        const int now = (l >= 1 && l <= K) ? s_map[l] : 0;
        out_labels[frame + p] = now;
        mask[frame + p] = now != 0;
    }
    // every entry of the new table is written exactly once: a row below kept' by the one old row that moves there, the rest zeroed
    const int64_t tab = (int64_t)f * K * VAL_FIELDS;
    for (int j = tid; j < K * VAL_FIELDS; j += VAL_THREADS) {
        const int r = j / VAL_FIELDS, field = j & (VAL_FIELDS - 1), now = s_map[r + 1];
        if (now) out_table[tab + (int64_t)(now - 1) * VAL_FIELDS + field] = table[tab + j];
        if (r >= s_kept) out_table[tab + j] = 0;
    }
}

}  // namespace

extern "C" int cgs_objects_ablate(const uint8_t* frames, const int32_t* labels, const int32_t* offsets, int32_t n, int32_t f0, int32_t f1,
                                  int32_t max_objects, int32_t grow, int32_t fill_mode, uint32_t fill_rgb, const uint8_t* fill,
                                  int64_t fill_stride, int64_t rows, uint8_t* out, int32_t* row_frame, int32_t* row_label,
                                  cgs_stream_t stream_) {
    if (!frames || !labels || !offsets || !out || !row_frame || !row_label || n < 1 || f0 < 0 || f1 <= f0 || f1 > n || rows < 1 ||
        max_objects < 1 || grow < 0 || fill_mode < 0 || fill_mode > 2 || (fill_mode == 1) != (fill != nullptr) ||
        (fill_stride != 0 && fill_stride != VAL_BYTES) || (fill_rgb >> 24) || ((uintptr_t)frames & 15u) || ((uintptr_t)out & 15u) ||
        ((uintptr_t)fill & 15u) || ((uintptr_t)labels & 3u) || ((uintptr_t)offsets & 3u) || ((uintptr_t)row_frame & 3u) ||
        ((uintptr_t)row_label & 3u))
        return CGS_ERR_BADARG;
    if (max_objects > CGS_OBJ_VALUE_MAX_OBJECTS || grow > VAL_MAX_GROW) return CGS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(ablate_kernel, dim3((unsigned)(f1 - f0)), dim3(VAL_THREADS), 0, (hipStream_t)stream_, frames, labels, offsets,
                       (int)f0, (int)max_objects, (int)grow, (int)fill_mode, fill_rgb, fill, fill_stride, rows, out, row_frame, row_label);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}

extern "C" int cgs_objects_select(const int32_t* labels, const int32_t* table, const int32_t* kept, const uint8_t* keep, int32_t n,
                                  int32_t h, int32_t w, int32_t max_objects, int32_t* out_labels, int32_t* out_table, int32_t* out_kept,
                                  uint8_t* mask, int32_t* unscored, cgs_stream_t stream_) {
    if (!labels || !table || !kept || !keep || !out_labels || !out_table || !out_kept || !mask || !unscored || n < 1 || h < 1 || w < 1 ||
        max_objects < 1 || ((uintptr_t)labels & 3u) || ((uintptr_t)table & 3u) || ((uintptr_t)kept & 3u) || ((uintptr_t)out_labels & 3u) ||
        ((uintptr_t)out_table & 3u) || ((uintptr_t)out_kept & 3u) || ((uintptr_t)unscored & 3u))
        return CGS_ERR_BADARG;
    if (h > VAL_SIDE || w > VAL_SIDE || max_objects > CGS_OBJ_VALUE_MAX_OBJECTS) return CGS_ERR_UNSUPPORTED;
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)n), dim3(VAL_THREADS), 0, (hipStream_t)stream_, labels, table, kept, keep, (int)(h * w),
                       (int)max_objects, out_labels, out_table, out_kept, mask, unscored);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}
