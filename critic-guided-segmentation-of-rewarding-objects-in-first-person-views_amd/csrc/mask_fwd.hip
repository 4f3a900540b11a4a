// The mask head forward in ONE kernel (round 3): see mask_fwd_body.h, which holds the body (shared with the fused decoder + mask head forward of tail.hip).
#include "mask_fwd_body.h"

namespace {
unsigned long long* g_maskfwd_stamps = nullptr;
}

#ifdef CGS_DEBUG_STAMPS
extern "C" int dbg_maskfwd_stamps(unsigned long long* stamps) { g_maskfwd_stamps = stamps; return CGS_OK; }
#endif

template <int SRC>     // SRC_U8C3 / SRC_F32C3
__global__ void __launch_bounds__(256, SRC == SRC_U8C3 ? 2 : 1) mask_fwd_kernel(MaskFwdParams P) {     // (fp32 frames: 9 more staging registers per pixel group than uint8 -- at two workgroups per SIMD they spilled 16 VGPRs)
    cgs_kernarg_prefetch<sizeof(MaskFwdParams)>();
    __shared__ __attribute__((aligned(16))) float4 stage4[kMaskStageF4];
    __shared__ float win[kMaskWinFloats];      // [slot][window element][quad column]: lane-contiguous, conflict-free
    __shared__ float zred[8];
    mask_fwd_body<SRC, false, false>(P, stage4, win, zred, [] {});
}

// training form of the mask head forward: h [n,64,64,16], z [n,64,64], zpart [mask_train_partials(n)][2]
int mask_train_partials(int n) { return n; }
int mask_train_launch(int n, int img_kind, const void* img, const float* o0, const float* w0, const float* b0, const float* w2,
                      const float* b2, float* h, float* z, float* zpart, const float* w0_pack, hipStream_t st) {
    if (n <= 0) return CGS_OK;
    MaskFwdParams P{img, o0, w0, b0, w2, b2, h, z, zpart, n, g_maskfwd_stamps, w0_pack};
    if (img_kind == CGS_SRC_U8) hipLaunchKernelGGL(mask_fwd_kernel<SRC_U8C3>, dim3(n), dim3(256), 0, st, P);
    else hipLaunchKernelGGL(mask_fwd_kernel<SRC_F32C3>, dim3(n), dim3(256), 0, st, P);
    CGS_HIP_CHECK_LAUNCH();
    return CGS_OK;
}
