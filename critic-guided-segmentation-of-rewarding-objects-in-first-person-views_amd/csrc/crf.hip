// Two-label fully-connected CRF (Krähenbühl & Koltun, NIPS 2011) with Potts compatibility, exact mean field: the
// `-crf` post-processing of main.py:1226-1263 (SimpleCRF densecrf(I, P, param)), without the permutohedral lattice.
//
// Model (include/cgs_hip.h, cgs_dense_crf2): per frame of N = h*w pixels, positions p = (x, y) and uint8 colours c,
//   kB(i,j) = exp(-|p_i-p_j|^2 / 2 alpha^2 - |c_i-c_j|^2 / 2 beta^2),  kG(i,j) = exp(-|p_i-p_j|^2 / 2 gamma^2)   (j = i included)
//   n_i = (sum_j k(i,j) + 1e-20)^-1/2 per kernel,  U_l = -ln P_l,  d = a_1 - a_0,  Q1 = sigmoid(d)
//   d = (U_0 - U_1) + sum_k w_k n_i (2 sum_j k(i,j) n_j Q1(j) - S_i),   S_i = sum_j k(i,j) n_j.
//
// Launch plan over a chunk of frames (every launch covers every frame of the chunk):
//   bilateral<PASS_NORM>       row sums of kB (and the separable kG ones) -> nB, nG; dU = U0 - U1; vB = nB Q1, vG = nG Q1 of the start
//   gauss_rows                 T(x,y) = sum_x' g(x-x') vG(x',y) (and the same of nG at the first iteration)
//   bilateral<PASS_FIRST>      sum_j kB vB and S^B in one sweep, the column pass of kG, S^G; the first update
//   gauss_rows, bilateral<PASS_ITER>  once per further iteration (sum_j kB vB only)
// The bilateral sum is the cost (N^2 pairs per pass).  A workgroup owns 1024 pixels i of one frame (4 per lane, as two float2 so the
// compiler can use packed fp32 math) and sweeps j in LDS tiles.  Every sum of a pixel is accumulated by one lane in a fixed order (per
// 64-pixel block, then block after block): deterministic, and independent of which other frames share the launch.
#include "cgs_common.h"

#include <algorithm>

namespace {

constexpr int CRF_THREADS = 256;
constexpr int CRF_PIX = 4;                                  // pixels i per lane
constexpr int CRF_IBLOCK = CRF_THREADS * CRF_PIX;           // pixels i per workgroup
constexpr int CRF_TJ = 1024;                                // pixels j per LDS tile (32 KB)
constexpr int CRF_MAX_PIXELS = 16384;
constexpr int CRF_CHUNK_PIXELS = 1 << 22;                   // frames per call chunk: scratch of 10 floats per pixel (160 MB)
constexpr float LOG2E = 1.4426950408889634f;

enum { PASS_NORM = 0, PASS_FIRST = 1, PASS_ITER = 2 };

typedef float f2 __attribute__((ext_vector_type(2)));

struct CrfScratch {                 // [chunk pixels] each
    float* nB;                      // bilateral normalisation n^B
    float* nG;                      // spatial normalisation n^G
    float* sB;                      // S^B_i = sum_j kB n^B_j
    float* sG;                      // S^G_i
    float* dU;                      // U_0 - U_1
    float* vB[2];                   // n^B Q1, ping-pong (a pass reads all j of one buffer and writes the other)
    float* vG;                      // n^G Q1
    float* tQ;                      // row pass of the spatial kernel over vG
    float* tN;                      // row pass over n^G (first iteration only)
};

struct CrfScales {
    float sa;                       // log2e / (2 alpha^2): kB spatial part, exp2 argument per squared pixel distance
    float cs;                       // sqrt(log2e / (2 beta^2)): colour pre-scale
    float sg;                       // log2e / (2 gamma^2)
    float w1, w2;
};

__device__ __forceinline__ float sigmoidf_(float d) { return 1.0f / (1.0f + expf(-d)); }

// unary difference U_0 - U_1 with U_l = -ln P_l in fp32 (P_0 = 1 - P_1 in fp32); +-inf at P_1 = 1 / 0 pins the label
__device__ __forceinline__ float unary_diff(float p1) {
    const float p0 = 1.0f - p1;
    return (-logf(p0)) - (-logf(p1));
}

// sum_{t < len} exp2(-sg (c - t)^2) v[t * stride]  (one axis of the separable spatial kernel; fixed order)
__device__ __forceinline__ float gauss_axis(const float* v, int len, int stride, int c, float sg) {
    float acc = 0.f;
    for (int t = 0; t < len; ++t) {
        const float d = (float)(c - t);
        acc = fmaf(__builtin_amdgcn_exp2f(-sg * d * d), v[(long)t * stride], acc);
    }
    return acc;
}

__device__ __forceinline__ float gauss_axis_ones(int len, int c, float sg) {
    float acc = 0.f;
    for (int t = 0; t < len; ++t) {
        const float d = (float)(c - t);
        acc += __builtin_amdgcn_exp2f(-sg * d * d);
    }
    return acc;
}

// T(x, y) = sum_x' g(x - x') vG(x', y); with `both`, also the same filter of n^G into tN.
__global__ void __launch_bounds__(256) crf_gauss_rows(int nframes, int h, int w, CrfScales s, CrfScratch ws, int both) {
    const long total = (long)nframes * h * w;
    const long p = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= total) return;
    const int x = (int)(p % w);
    const long row0 = p - x;
    ws.tQ[p] = gauss_axis(ws.vG + row0, w, 1, x, s.sg);
    if (both) ws.tN[p] = gauss_axis(ws.nG + row0, w, 1, x, s.sg);
}

// One sweep of the bilateral all-pairs sum for 1024 pixels i of frame blockIdx.y, plus the per-pixel epilogue of the pass.
//   PASS_NORM:  acc0 = sum_j kB                     -> nB, nG, dU, start state
//   PASS_FIRST: acc0 = sum_j kB vB_j, acc1 = sum_j kB nB_j (= S^B)   -> update
//   PASS_ITER:  acc0 = sum_j kB vB_j                -> update
template <int PASS>
__global__ void __launch_bounds__(CRF_THREADS) crf_bilateral(const uint8_t* __restrict__ frames, const float* __restrict__ p1, int h, int w,
                                                             CrfScales s, CrfScratch ws, int src, int last, uint8_t* __restrict__ labels,
                                                             float* __restrict__ q1) {
    constexpr bool TWO = PASS == PASS_FIRST;
    __shared__ float4 recC[CRF_TJ];     // (c0', c1', c2', v)   colours pre-scaled by sqrt(log2e / 2 beta^2)
    __shared__ float4 recP[CRF_TJ];     // (x, y, x^2 + y^2, v2) integer-valued: the squared distance below is exact in fp32
    const int N = h * w;
    const long fbase = (long)blockIdx.y * N;
    const uint8_t* img = frames + fbase * 3;
    const float* vsrc = ws.vB[src];

    // the lane's four pixels: i = blockbase + tid + k * 256; out-of-range lanes compute on pixel N-1 and store nothing
    int pix[CRF_PIX];
    f2 xm2[2], ym2[2], pp[2], c0[2], c1[2], c2[2];
#pragma unroll
    for (int k = 0; k < CRF_PIX; ++k) {
        const int i = blockIdx.x * CRF_IBLOCK + (int)threadIdx.x + k * CRF_THREADS;
        pix[k] = i;
        const int ic = i < N ? i : N - 1;
        const float x = (float)(ic % w), y = (float)(ic / w);
        xm2[k >> 1][k & 1] = -2.f * x;
        ym2[k >> 1][k & 1] = -2.f * y;
        pp[k >> 1][k & 1] = x * x + y * y;
        c0[k >> 1][k & 1] = s.cs * (float)img[(long)ic * 3 + 0];
        c1[k >> 1][k & 1] = s.cs * (float)img[(long)ic * 3 + 1];
        c2[k >> 1][k & 1] = s.cs * (float)img[(long)ic * 3 + 2];
    }
    const f2 sa2 = {s.sa, s.sa};
    f2 acc0[2] = {{0.f, 0.f}, {0.f, 0.f}}, acc1[2] = {{0.f, 0.f}, {0.f, 0.f}};

    for (int j0 = 0; j0 < N; j0 += CRF_TJ) {
        const int len = min(CRF_TJ, N - j0);
        const int len64 = (len + 63) & ~63;
        __syncthreads();                // the previous tile's readers are done
        for (int t = threadIdx.x; t < len64; t += CRF_THREADS) {
            const int j = j0 + t;
            float4 rc = f4zero(), rp = f4zero();
            if (t < len) {
                const float x = (float)(j % w), y = (float)(j / w);
                rc = make_float4(s.cs * (float)img[(long)j * 3 + 0], s.cs * (float)img[(long)j * 3 + 1], s.cs * (float)img[(long)j * 3 + 2],
                                 PASS == PASS_NORM ? 1.f : vsrc[fbase + j]);
                rp = make_float4(x, y, x * x + y * y, TWO ? ws.nB[fbase + j] : 0.f);
            }                           // padding: v = v2 = 0 adds exactly nothing
            recC[t] = rc;
            recP[t] = rp;
        }
        __syncthreads();
        for (int b = 0; b < len64; b += 64) {
            f2 part0[2] = {{0.f, 0.f}, {0.f, 0.f}}, part1[2] = {{0.f, 0.f}, {0.f, 0.f}};
#pragma unroll 8
            for (int t = b; t < b + 64; ++t) {
                const float4 rc = recC[t], rp = recP[t];
#pragma unroll
                for (int g = 0; g < 2; ++g) {
                    // |p_i - p_j|^2 = |p_i|^2 + |p_j|^2 - 2 x_i x_j - 2 y_i y_j: integers < 2^16, exact
                    f2 dsq = pp[g] + rp.z;
                    dsq = xm2[g] * rp.x + dsq;
                    dsq = ym2[g] * rp.y + dsq;
                    const f2 d0 = c0[g] - rc.x, d1 = c1[g] - rc.y, d2 = c2[g] - rc.z;
                    f2 e = sa2 * dsq;
                    e = d0 * d0 + e;
                    e = d1 * d1 + e;
                    e = d2 * d2 + e;
                    f2 k;
                    k.x = __builtin_amdgcn_exp2f(-e.x);
                    k.y = __builtin_amdgcn_exp2f(-e.y);
                    part0[g] = k * rc.w + part0[g];
                    if (TWO) part1[g] = k * rp.w + part1[g];
                }
            }
#pragma unroll
            for (int g = 0; g < 2; ++g) {
                acc0[g] += part0[g];
                if (TWO) acc1[g] += part1[g];
            }
        }
    }

    // ---- per-pixel epilogue
    const float* tq = ws.tQ + fbase;
    const float* tn = ws.tN + fbase;
#pragma unroll
    for (int k = 0; k < CRF_PIX; ++k) {
        const int i = pix[k];
        if (i >= N) continue;
        const long gi = fbase + i;
        const int x = i % w, y = i / w;
        const float a0 = acc0[k >> 1][k & 1];
        float nb, ng, q;
        if (PASS == PASS_NORM) {
            nb = 1.0f / sqrtf(a0 + 1e-20f);
            ng = 1.0f / sqrtf(gauss_axis_ones(w, x, s.sg) * gauss_axis_ones(h, y, s.sg) + 1e-20f);
            const float pr = p1[gi];
            const float du = unary_diff(pr);
            ws.nB[gi] = nb;
            ws.nG[gi] = ng;
            ws.dU[gi] = du;
            q = sigmoidf_(du);                              // softmax(-U)
            if (last) labels[gi] = pr > 1.0f - pr ? 1 : 0;  // zero iterations: the argmax of P, ties to label 0
        } else {
            nb = ws.nB[gi];
            ng = ws.nG[gi];
            const float gq = gauss_axis(tq + x, h, w, y, s.sg);     // column pass of the spatial kernel
            float sb, sg;
            if (TWO) {
                sb = acc1[k >> 1][k & 1];
                sg = gauss_axis(tn + x, h, w, y, s.sg);
                ws.sB[gi] = sb;
                ws.sG[gi] = sg;
            } else {
                sb = ws.sB[gi];
                sg = ws.sG[gi];
            }
            const float d = ws.dU[gi] + s.w1 * nb * (2.f * a0 - sb) + s.w2 * ng * (2.f * gq - sg);
            q = sigmoidf_(d);
            if (last) labels[gi] = d > 0.f ? 1 : 0;         // ties to label 0
        }
        ws.vB[src ^ 1][gi] = nb * q;
        ws.vG[gi] = ng * q;
        if (last && q1) q1[gi] = q;
    }
}

}  // namespace

extern "C" int cgs_dense_crf2(const uint8_t* frames, const float* p1, int32_t n, int32_t h, int32_t w, const cgs_crf_params* prm,
                              uint8_t* labels, float* q1_or_null, cgs_stream_t stream_) {
    if (!frames || !p1 || !prm || !labels || n < 1 || h < 1 || w < 1) return CGS_ERR_BADARG;
    const cgs_crf_params P = *prm;
    if (!(P.alpha > 0.f) || !(P.beta > 0.f) || !(P.gamma > 0.f) || P.iterations < 0 || !(P.w_bilateral == P.w_bilateral) ||
        !(P.w_gaussian == P.w_gaussian))
        return CGS_ERR_BADARG;
    if ((long)h * w > CRF_MAX_PIXELS) return CGS_ERR_UNSUPPORTED;
    hipStream_t stream = (hipStream_t)stream_;
    const int N = h * w;
    const int chunk = (int)std::max(1L, std::min({(long)n, (long)CRF_CHUNK_PIXELS / N, 32768L}));     // grid.y <= 32768
    const size_t per = (size_t)chunk * N;
    float* base = nullptr;
    hipError_t e = hipMallocAsync((void**)&base, 10 * per * sizeof(float), stream);
    if (e != hipSuccess) return (int)e;
    CrfScratch ws;
    ws.nB = base;
    ws.nG = base + per;
    ws.sB = base + 2 * per;
    ws.sG = base + 3 * per;
    ws.dU = base + 4 * per;
    ws.vB[0] = base + 5 * per;
    ws.vB[1] = base + 6 * per;
    ws.vG = base + 7 * per;
    ws.tQ = base + 8 * per;
    ws.tN = base + 9 * per;
    CrfScales sc;
    sc.sa = LOG2E / (2.f * P.alpha * P.alpha);
    sc.cs = sqrtf(LOG2E / (2.f * P.beta * P.beta));
    sc.sg = LOG2E / (2.f * P.gamma * P.gamma);
    sc.w1 = P.w_bilateral;
    sc.w2 = P.w_gaussian;
    int rc = CGS_OK;
    for (int f0 = 0; f0 < n && rc == CGS_OK; f0 += chunk) {
        const int nf = std::min(chunk, n - f0);
        const long off = (long)f0 * N;
        const uint8_t* fr = frames + off * 3;
        const float* pr = p1 + off;
        uint8_t* lab = labels + off;
        float* q = q1_or_null ? q1_or_null + off : nullptr;
        const dim3 grid((unsigned)((N + CRF_IBLOCK - 1) / CRF_IBLOCK), (unsigned)nf);
        const unsigned rows_grid = (unsigned)(((long)nf * N + 255) / 256);
        hipLaunchKernelGGL(crf_bilateral<PASS_NORM>, grid, dim3(CRF_THREADS), 0, stream, fr, pr, h, w, sc, ws, 1, P.iterations == 0 ? 1 : 0,
                           lab, q);
        int src = 0;                    // PASS_NORM wrote vB[1 ^ 1] = vB[0]
        for (int it = 1; it <= P.iterations; ++it) {
            hipLaunchKernelGGL(crf_gauss_rows, dim3(rows_grid), dim3(256), 0, stream, nf, h, w, sc, ws, it == 1 ? 1 : 0);
            const int last = it == P.iterations ? 1 : 0;
            if (it == 1)
                hipLaunchKernelGGL(crf_bilateral<PASS_FIRST>, grid, dim3(CRF_THREADS), 0, stream, fr, pr, h, w, sc, ws, src, last, lab, q);
            else
                hipLaunchKernelGGL(crf_bilateral<PASS_ITER>, grid, dim3(CRF_THREADS), 0, stream, fr, pr, h, w, sc, ws, src, last, lab, q);
            src ^= 1;
        }
        const hipError_t le = hipGetLastError();
        if (le != hipSuccess) rc = (int)le;
    }
    e = hipFreeAsync(base, stream);
    if (rc == CGS_OK && e != hipSuccess) rc = (int)e;
    return rc;
}
