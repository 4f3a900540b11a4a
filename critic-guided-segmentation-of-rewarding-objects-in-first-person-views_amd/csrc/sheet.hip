// The PNG sheet of the mask-training loop (Handler.segmentation_training's debug grid, main.py:465-496), one launch per sheet.
//
// A sheet is [7 x 64, 64 n, 3] uint8: two black rows of tiles (the label band: the text is drawn on the host), then A, B,
// replaced = A (1 - Z) + Z B, injected = B (1 - Z) + Z A and Z on all three channels; image i fills columns 64 i .. 64 i + 63
// (include/cgs_hip.h).  A tile row is 192 B = 12 x 16 B and a sheet row 192 n B, so with a 16-byte aligned base every tile row of the
// sources and of the sheet starts on a 16-byte boundary.
//
// Launch: blockIdx.y = the pixel row y of the tiles (0..63), one lane per 16-byte piece p of that row across the sheet (12 n pieces).
// The lane loads its piece of A and of B (16 B each) and the six mask values its bytes belong to, and stores seven pieces: two of
// zeros, A, B, the two mixes and Z.  Neighbouring lanes store neighbouring 16 bytes, every output byte is written exactly once.
//
// Byte rule: np.uint8(255 * v) with every operation of v rounded to fp32 on its own, in the reference's operand order -- the
// __f*_rn intrinsics keep hipcc from contracting a product and a sum into an FMA, which would change 1.8e-4 of the bytes.
#include "cgs_common.h"

namespace {

constexpr int SHEET_TILE = 64;
constexpr int SHEET_PIECES = SHEET_TILE * 3 / 16;    // 16-byte pieces per tile row (12)
constexpr int SHEET_THREADS = 256;

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// np.uint8(255 * v): one fp32 product, truncated (v in [0, 1] up to rounding; clamped so that the conversion is defined)
__device__ __forceinline__ uint32_t sheet_byte(float v) {
    return (uint32_t)(int)fminf(fmaxf(__fmul_rn(255.0f, v), 0.0f), 255.0f);
}

__global__ void __launch_bounds__(SHEET_THREADS)
sheet_compose_kernel(const u32x4* __restrict__ A, const u32x4* __restrict__ B, const float* __restrict__ Z, int n,
                     u32x4* __restrict__ out) {
    const int pieces = SHEET_PIECES * n;                               // per sheet row
    const int p = blockIdx.x * SHEET_THREADS + threadIdx.x;
    if (p >= pieces) return;
    const int y = blockIdx.y;
    const int i = p / SHEET_PIECES, j = p - i * SHEET_PIECES;
    const size_t row = (size_t)i * SHEET_TILE + y;                     // tile row of image i
    const u32x4 a = A[row * SHEET_PIECES + j], b = B[row * SHEET_PIECES + j];
    // byte m of the piece is byte 16 j + m of the tile row: pixel x0 + (r + m) / 3 with x0 = 16 j / 3, r = 16 j % 3 = j % 3;
    // (r + 15) / 3 = 5, so the piece touches pixels x0 .. x0 + 5 <= 63
    const int x0 = 16 * j / 3, r = j % 3;
    const float* z = Z + row * SHEET_TILE + x0;
    float zv[6], omz[6];
#pragma unroll
    for (int t = 0; t < 6; ++t) {
        zv[t] = z[t];
        omz[t] = __fsub_rn(1.0f, zv[t]);
    }
    u32x4 rep, inj, zz;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        uint32_t wr = 0, wi = 0, wz = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int t = (r + 4 * k + q) / 3;
            const float fa = __fdiv_rn((float)((a[k] >> (8 * q)) & 0xFFu), 255.0f);
            const float fb = __fdiv_rn((float)((b[k] >> (8 * q)) & 0xFFu), 255.0f);
            const float vr = __fadd_rn(__fmul_rn(fa, omz[t]), __fmul_rn(zv[t], fb));     // A * (1 - Z) + Z * B
            const float vi = __fadd_rn(__fmul_rn(fb, omz[t]), __fmul_rn(zv[t], fa));     // B * (1 - Z) + Z * A
            wr |= sheet_byte(vr) << (8 * q);
            wi |= sheet_byte(vi) << (8 * q);
            wz |= sheet_byte(zv[t]) << (8 * q);
        }
        rep[k] = wr;
        inj[k] = wi;
        zz[k] = wz;
    }
    // uint8(255 * (k / 255.0f)) == k for all 256 byte values in fp32: the A and B rows are the frames
    const u32x4 zero = {0u, 0u, 0u, 0u};
    const size_t band = (size_t)SHEET_TILE * pieces;                   // pieces of one row of tiles
    u32x4* dst = out + (size_t)y * pieces + p;
    dst[0] = zero;
    dst[band] = zero;
    dst[2 * band] = a;
    dst[3 * band] = b;
    dst[4 * band] = rep;
    dst[5 * band] = inj;
    dst[6 * band] = zz;
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int cgs_sheet_compose(const uint8_t* A, const uint8_t* B, const float* Z, int32_t n, uint8_t* out, cgs_stream_t stream) {
    if (!A || !B || !Z || !out || n < 1 || n > CGS_SHEET_MAX_N || !aligned16(A) || !aligned16(B) || !aligned16(out) ||
        ((uintptr_t)Z & 3u))
        return CGS_ERR_BADARG;
    const int pieces = SHEET_PIECES * n;
    const dim3 grid((unsigned)((pieces + SHEET_THREADS - 1) / SHEET_THREADS), SHEET_TILE);
    hipLaunchKernelGGL(sheet_compose_kernel, grid, dim3(SHEET_THREADS), 0, (hipStream_t)stream, reinterpret_cast<const u32x4*>(A),
                       reinterpret_cast<const u32x4*>(B), Z, n, reinterpret_cast<u32x4*>(out));
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}
