/*
 * cgs_hip.h -- C ABI of libcgs_hip.so: the MI355X (gfx950) kernels behind the Hourglass
 * (encoder + critic head + decoder/mask head) training and inference path.
 *
 * The reference (ndrwmlnk/critic-guided-segmentation-...) has no FFI/plugin boundary: its hot
 * path is ordinary PyTorch module calls.  Each entry point below therefore names the reference
 * lines whose ATen dispatches it replaces.  Conventions:
 *   - plain pointers and sizes only; every pointer is DEVICE memory unless marked "host";
 *   - the caller owns every buffer (inputs, outputs, saved-for-backward side buffers, slabs);
 *     the library never allocates, frees or retains pointers across calls;
 *   - every call enqueues on the given hipStream_t and never synchronises it (graph-capturable);
 *   - return value: 0 = CGS_OK, CGS_ERR_* (< 0) for argument errors, a positive hipError_t otherwise.
 *   - activations are NHWC fp32; images are NHWC uint8 or NHWC fp32 (3 channels);
 *   - conv weights are HWIO fp32  w[ky][kx][ci][co]  (checkpoints stay OIHW; the host permutes);
 *     input-channel order of a two-source conv is (source A channels, then source B channels),
 *     i.e. the reference's torch.cat((skip, upsampled), 1) / torch.cat((X, upsampled), 1).
 */
#ifndef CGS_HIP_H
#define CGS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* cgs_stream_t; /* hipStream_t */

enum { CGS_OK = 0, CGS_ERR_UNSUPPORTED = -1, CGS_ERR_BADARG = -2 };
enum { CGS_SRC_F32 = 0, CGS_SRC_U8 = 1, CGS_SRC_MIX = 2 };

/* CGS_SRC_MIX (features.0 only): `src_a` points to this HOST struct; the source image n of the launch is computed in the
 * tile loader and never stored: n < n_a: A[n](1-Z[n]) + Z[n] B[n] (replaced), n >= n_a: B(1-Z) + Z A of A-image n - n_a
 * (injected) -- main.py:395,406.  a, b: uint8 [n_a,64,64,3]; z: fp32 [n_a,64,64] (all device pointers).            */
typedef struct {
    const uint8_t* a;
    const uint8_t* b;
    const float* z;
    int32_t n_a;
    int32_t reserved;
} cgs_mix_src;
enum { CGS_ACT_NONE = 0, CGS_ACT_RELU = 1, CGS_ACT_LRELU = 2, CGS_ACT_SIGMOID = 3 };

/* Dropout on a tensor = Philox4x32-10 keep-mask keyed by (seed; base + element/4, site, *step).
 * p == 0 disables it.  `step` points to a device-resident counter so that a captured graph
 * draws fresh masks on every replay; forward and backward of one step read the same value.
 * `base` (in units of 4 floats) is added to the element index: a call that works on a slice of a
 * larger batch buffer passes the slice's offset so that forward and backward launches that slice
 * the batch differently still draw identical masks for identical images. */
typedef struct {
    float p;
    uint32_t site;
    uint64_t seed;
    const uint64_t* step; /* device; may be NULL when p == 0 */
    uint32_t base;
    uint32_t reserved;
} cgs_dropout;

/* One 3x3, stride-1, pad-1 convolution of the Hourglass (nets.py:170-183, 480-490). */
typedef struct {
    int32_t n;      /* images */
    int32_t h, w;   /* conv output size before pooling (= size of source A) */
    int32_t ca;     /* channels of source A (direct / skip input) */
    int32_t cb;     /* channels of source B (nearest-upsampled low-res input); 0 = none */
    int32_t co;     /* output channels */
    int32_t src_a;  /* CGS_SRC_F32 | CGS_SRC_U8 (uint8 image, /255 fused into the loader) | CGS_SRC_MIX (see cgs_mix_src) */
    int32_t ups;    /* source B scale: 2 (source is h/2 x w/2) or 4 (source is 1x1, h = w = 4) */
    int32_t act;    /* CGS_ACT_* applied after bias */
    int32_t pool;   /* 1: fused 2x2/2 max-pool after the activation */
    cgs_dropout drop_a; /* dropout applied to source A while loading (nets.py:179,183) */
} cgs_conv_desc;

/* ---- convolution forward ------------------------------------------------------------
 * Replaces Conv2d + ReLU/LeakyReLU/Sigmoid + MaxPool2d + Upsample + cat + Dropout of
 * NewCritic.forward (nets.py:197-205) and UnetDecoder.forward (nets.py:500-521).
 *   out   : [n, h, w, co]  (pool=0)  or [n, h/2, w/2, co] (pool=1)
 *   amask : pool=1 only, may be NULL.  uint32 [n, h/2, w/2, co/8]: one nibble per channel =
 *           index (0..3, row-major in the 2x2 window, first maximum wins) of the pooled
 *           element, or 0xF when the pooled value is <= 0 (ReLU gradient is zero there).
 *           For the mask layer (h=w=64, ca=16, co=1, sigmoid, pool=0) the same slot optionally receives, as floats
 *           [n*4][2], the per-workgroup partial sums (sum |z|, sum z^2) that cgs_phase2_losses consumes.         */
int cgs_conv3x3_fwd(const cgs_conv_desc* d, const void* src_a, const float* src_b,
                    const float* w_hwio, const float* bias, float* out, uint32_t* amask,
                    cgs_stream_t stream);

/* ---- convolution backward, data -----------------------------------------------------
 * Replaces the convolution_backward(input) + max_pool2d/threshold/upsample/cat/dropout backward
 * nodes autograd builds for the layer (loss.backward(), main.py:198,462).
 *   dy      : gradient w.r.t. the layer output: [n,h,w,co], or [n,h/2,w/2,co] + amask when pool=1
 *             (the pre-pool gradient is re-expanded on the fly, ReLU mask included).
 *   d_a     : [n,h,w,ca] gradient w.r.t. source A, or NULL to skip.  Fused epilogue:
 *             d_a = conv_bwd * dropout_mask(drop_a) * act'(src_a_post) + addend
 *               src_a_post/src_a_act: optional (may be NULL/NONE) post-activation values of source A
 *               and the activation that produced them (LeakyReLU for masker.0 -> masker.2);
 *               addend: optional [n_addend,h,w,ca] gradient already accumulated for source A (skip
 *               connection), added for images < n_addend; may alias d_a.
 *   d_b     : gradient w.r.t. source B at ITS resolution ([n,h/2,w/2,cb] or [n,cb] for ups=4), i.e. the
 *             nearest-upsample backward (2x2 / 4x4 sum) is fused; NULL to skip.            */
int cgs_conv3x3_bwd_data(const cgs_conv_desc* d, const float* dy, const uint32_t* amask,
                         const float* w_hwio, const float* src_a_post, int32_t src_a_act,
                         const float* addend, int32_t n_addend, float* d_a, float* d_b,
                         cgs_stream_t stream);

/* ---- mask head backward in one pass (nets.py:488-491 backward: masker.2 and masker.0) ----------------
 * dzpre [n,64,64] (gradient w.r.t. the pre-sigmoid mask), h [n,64,64,16] (saved masker.0 output, post-LeakyReLU).
 *   d_o0 [n,32,32,8]  = upsample-backward of conv_bwd_data(d_h; w_m0) restricted to the 8 decoder channels, where
 *                       d_h = LeakyReLU'(h) * conv_bwd_data(dzpre; w_m2) is rebuilt on the fly from the 1-channel
 *                       dzpre (never read from memory) and the nearest-upsample in front of masker.0 is folded into
 *                       its weights (one stride-2 4x4 convolution on the matrix cores);
 *   d_h  [n,64,64,16] : optional copy of that intermediate (NULL: never stored);
 *   slab_m2 : optional [cgs_mask_head_bwd_slabs(n)][145]  partial masker.2 weight+bias gradients,
 *   slab_m0 : optional [cgs_mask_head_bwd_slabs(n)][1600] partial masker.0 weight+bias gradients (needs slab_m2, x =
 *             the masker.0 image input [n,64,64,3] of kind src_a, and o0 [n,32,32,8]); both in the slab layout of
 *             cgs_conv3x3_bwd_weight for those layers, to be summed by cgs_reduce_slabs().
 * cgs_mask_head_bwd_slabs() returns 0 when this build cannot produce the slabs (the caller then passes NULL, asks for
 * d_h and runs cgs_conv3x3_bwd_weight for the two layers).                                                      */
int cgs_mask_head_bwd_slabs(int32_t n);
int cgs_mask_head_bwd(int32_t n, int32_t src_a, const void* x, const float* o0, const float* dzpre, const float* h,
                      const float* w_m2_hwio, const float* w_m0_hwio, float* d_h, float* d_o0, float* slab_m2,
                      float* slab_m0, cgs_stream_t stream);

/* ---- mask head forward for inference (nets.py:488-491 in eval mode) in one pass -----------------------
 * z [n,64,64] = sigmoid(conv3x3(LeakyReLU(conv3x3(cat(x, up(o0)); w_m0, b_m0)); w_m2, b_m2)) without ever storing the
 * 16-channel intermediate (it is needed only by the backward pass).  x [n,64,64,3] of kind src_a (CGS_SRC_U8 / CGS_SRC_F32), o0 [n,32,32,8].
 * Since round 5 this is the training forward's kernel (cgs_mask_train_fwd) storing nothing but z: masker.0 and masker.2 on the
 * matrix cores from registers; z is bit-identical to the training forward's.  (cgs_mask_infer_fwd_tile: the earlier tile
 * kernel -- masker.0 into an LDS tile, masker.2 + sigmoid on that tile.)  cgs_mask_infer_fwd_packed: the same with
 * masker.0's per-lane weight registers w_m0_pack [40][64] as cgs_tail_dec_fwd_pack / cgs_tail_dec_fwd_dec0 build them (NULL: gathered
 * per workgroup).  Returns CGS_ERR_UNSUPPORTED in the VALU fallback build (use two cgs_conv3x3_fwd calls).          */
int cgs_mask_infer_fwd(int32_t n, int32_t src_a, const void* x, const float* o0, const float* w_m0_hwio,
                       const float* b_m0, const float* w_m2_hwio, const float* b_m2, float* z,
                       cgs_stream_t stream);
int cgs_mask_infer_fwd_packed(int32_t n, int32_t src_a, const void* x, const float* o0, const float* w_m0_hwio,
                       const float* b_m0, const float* w_m2_hwio, const float* b_m2, float* z, const float* w_m0_pack,
                       cgs_stream_t stream);
int cgs_mask_infer_fwd_tile(int32_t n, int32_t src_a, const void* x, const float* o0, const float* w_m0_hwio,
                            const float* b_m0, const float* w_m2_hwio, const float* b_m2, float* z, cgs_stream_t stream);

/* Training form of the same pass (nets.py:488-491 in train mode; replaces masker.0's and masker.2's separate forwards): also
 * stores h [n,64,64,16] = LeakyReLU(masker.0) ONCE from the on-chip tile (the backward pass needs it) and leaves, per tile,
 * (sum |z|, sum z^2) for the L1 / L2 mask losses of main.py:421-429 in zpart [2 * cgs_mask_train_fwd_partials(n)].
 * h is never re-read to compute z (the stand-alone masker.2 forward read all 134 MB of it at n = 512).              */
int cgs_mask_train_fwd_partials(int32_t n);
int cgs_mask_train_fwd(int32_t n, int32_t src_a, const void* x, const float* o0, const float* w_m0_hwio,
                       const float* b_m0, const float* w_m2_hwio, const float* b_m2, float* h, float* z,
                       float* zpart, cgs_stream_t stream);
/* The same with masker.0's per-lane weight registers (40 x 64 floats) taken from w_m0_pack instead of rebuilt by every workgroup;
 * cgs_tail_dec_fwd_pack -- the launch before it on the training path -- builds them in one spare workgroup (w_m0_pack = NULL: as above). */
int cgs_mask_train_fwd_packed(int32_t n, int32_t src_a, const void* x, const float* o0, const float* w_m0_hwio, const float* b_m0,
                              const float* w_m2, const float* b_m2, float* h, float* z, float* zpart, const float* w_m0_pack,
                              cgs_stream_t stream);

/* Same contract with fp16 OPERANDS for the masker.0 GEMM (v_mfma_f32_16x16x16_f16, fp32 accumulate; masker.2 stays
 * fp32): BASELINE config 4 ("-process inference-only, fp16 conv kernels").  Opt-in: z differs from the fp32 result by
 * about 1e-3 absolute; never used by training.                                                                  */
int cgs_mask_infer_fwd_f16(int32_t n, int32_t src_a, const void* x, const float* o0, const float* w_m0_hwio,
                           const float* b_m0, const float* w_m2_hwio, const float* b_m2, float* z,
                           cgs_stream_t stream);

/* ---- fused fp16 inference path (BASELINE config 4; csrc/hconv.hip): the three 64x64 / 32x32 convolutions of the eval-mode forward
 * (nets.py:170-176, 516-517) with fp16 activations / weights and fp32 accumulation on v_mfma_f32_16x16x32_f16.  cgs_f16_enc0_fwd:
 * uint8 frames [n,64,64,3] -> e0 fp16 [n,32,32,8] (conv + ReLU + MaxPool2d(2)); cgs_f16_enc1_fwd: e0 -> e1 fp32 [n,16,16,8] (the
 * 16x16-and-smaller layers stay on the fp32 tail kernels); cgs_f16_dec0_fwd: cat(e0, nearest-up(o1 fp32 [n,16,16,8])) -> o0 fp16
 * [n,32,32,8]; cgs_mask_infer_fwd_f16o: cgs_mask_infer_fwd_f16 reading that fp16 o0.  Weights / bias: the layer's HWIO fp32 parameters.
 * Opt-in precision (engine.infer(fp16=True)); never used by training.                                                              */
int cgs_f16_enc0_fwd(int32_t n, const uint8_t* x_u8, const float* w_hwio, const float* bias, void* e0_f16, cgs_stream_t stream);
int cgs_f16_enc1_fwd(int32_t n, const void* e0_f16, const float* w_hwio, const float* bias, float* e1_f32, cgs_stream_t stream);
int cgs_f16_dec0_fwd(int32_t n, const void* e0_f16, const float* o1_f32, const float* w_hwio, const float* bias, void* o0_f16,
                     cgs_stream_t stream);
int cgs_mask_infer_fwd_f16o(int32_t n, int32_t src_a, const void* x, const void* o0_f16, const float* w_m0_hwio, const float* b_m0,
                            const float* w_m2_hwio, const float* b_m2, float* z, cgs_stream_t stream);
/* config 5 (build-defined 128x128 variant, hourglass128.py; chfak 1): features.0 on the same kernel in bfloat16 -- x: uint8 frames
 * (x_is_f32 = 0) or fp32 frames [n,128,128,3] (the replaced / injected mixes, main.py:642-670) -> e0 bf16 [n,64,64,8]; codes (optional):
 * the MaxPool2d argmax bytes [n,64,64,8] of the training forward (cgs_bf16_pool_expand reads them).                                    */
int cgs_bf16_enc0_fwd(int32_t n, const void* x, int32_t x_is_f32, const float* w_hwio, const float* bias, void* e0_bf16, uint8_t* codes,
                      cgs_stream_t stream);
/* The 128x128 layers of config 5's training step at chfak 1 on the whole-strip kernel in bfloat16 (csrc/hconv.hip, h5conv_kernel), with the
 * step's element-wise neighbours fused; w_hwio / bias = the layer's fp32 master parameters [9][ci][co] / [co]:
 *   cgs_bf16_mask0_fwd      hm bf16 [n,128,128,16] = LeakyReLU(conv3x3(cat(frames uint8 / 255, nearest-up2(o0 bf16 [n,64,64,8]))))
 *   cgs_bf16_mask2_fwd      Z fp32 [n,128,128]     = Sigmoid(conv3x3(hm))
 *   cgs_bf16_enc0_bwd_data  d frames fp32 [n,128,128,3] from d features.0 bf16 [n,128,128,8]
 *   cgs_bf16_mask2_bwd_data d (masker.0 pre-activation) bf16 [n,128,128,16] = conv3x3^T(dz fp32 [n,128,128]) x LeakyReLU'(hm)
 *   cgs_bf16_mask0_bwd_data d o0 bf16 [n,64,64,8] = 2x2 cell sums of conv3x3^T(dhm) over the upsampled source's channels             */
int cgs_bf16_mask0_fwd(int32_t n, const uint8_t* x_u8, const void* o0_bf16, const float* w_hwio, const float* bias, void* hm_bf16,
                       cgs_stream_t stream);
int cgs_bf16_mask2_fwd(int32_t n, const void* hm_bf16, const float* w_hwio, const float* bias, float* z, cgs_stream_t stream);
int cgs_bf16_enc0_bwd_data(int32_t n, const void* dy_bf16, const float* w_hwio, float* dx, cgs_stream_t stream);
int cgs_bf16_enc0_bwd_data_pooled(int32_t n, const void* dp_bf16, const void* addend_bf16, const uint8_t* codes, const float* w_hwio, float* dx,
                                  cgs_stream_t stream);      /* the same from dP bf16 [n,64,64,8] (+ addend) and the forward argmax bytes */
/* features.0's data gradient on the two mixes AND cgs_mix_bwd in one pass over n A-images: dp / codes = the pooled gradient bf16 [2n,64,64,8] /
 * argmax bytes of the 2 n mix images [replaced | injected], a_u8 / b_u8 the frames [n,128,128,3], z the mask [n,128,128] ->
 * dzpre [n,128,128] (the gradient at the mask's pre-Sigmoid value, regularisers l1s / l2s as cgs_mix_bwd); no d mix tensor in memory.       */
/* features.0 forward / weight gradient on the VIRTUAL mixes (main.py:395,406): the 2 n images [replaced | injected] are formed from the frame pairs
 * a_u8 / b_u8 [n,128,128,3] and the mask z [n,128,128] while a tile is staged (cgs_mix_fwd's formula); the fp32 mixes are
 * never written: cgs_mix_fwd(.., mixed = NULL, zpart) then leaves only the partial sums of |Z| and Z^2 the loss needs.  Outputs as
 * cgs_bf16_enc0_fwd / cgs_bf16_hwgrad_pooled on 2 n materialised images (slab rows: cgs_bf16_hwgrad_slabs(2 n, 128, 3, 0, 8)).                     */
int cgs_bf16_enc0_fwd_mix(int32_t n, const uint8_t* a_u8, const uint8_t* b_u8, const float* z, const float* w_hwio, const float* bias, void* e0_bf16,
                          uint8_t* codes, cgs_stream_t stream);
int cgs_bf16_hwgrad_pooled_mix(int32_t n, const uint8_t* a_u8, const uint8_t* b_u8, const float* z, const void* dp, const uint8_t* codes, float* slab,
                               cgs_stream_t stream);
int cgs_bf16_enc0_bwd_mix(int32_t n, const void* dp_bf16, const uint8_t* codes, const float* w_hwio, const uint8_t* a_u8, const uint8_t* b_u8,
                          const float* z, float l1s, float l2s, float* dzpre, cgs_stream_t stream);
int cgs_bf16_mask2_bwd_data(int32_t n, const float* dz, const void* hm_bf16, const float* w_hwio, void* dhm_bf16, cgs_stream_t stream);
int cgs_bf16_mask0_bwd_data(int32_t n, const void* dhm_bf16, const float* w_hwio, void* do0_bf16, cgs_stream_t stream);
/* The 64x64 layers of the same step: features.3 forward (src_a = e0 bf16 [n,64,64,8] -> e1 bf16 [n,32,32,8] + argmax bytes) and data gradient
 * (src_a = dy bf16 [n,64,64,8] -> d e0); dec_model.0 forward (cat(src_a = e0, nearest-up2(src_b = o1 bf16 [n,32,32,8])) -> o0 [n,64,64,8]) and
 * its data gradients (src_a = d o0 [n,64,64,8] -> skip gradient [n,64,64,8] / cell-summed low-resolution gradient [n,32,32,8]).  bias NULL
 * for the data gradients.                                                                                                            */
enum { CGS_H5_ENC1_FWD = 1, CGS_H5_ENC1_BWD_DATA = 2, CGS_H5_DEC0_FWD = 3, CGS_H5_DEC0_BWD_SKIP = 4, CGS_H5_DEC0_BWD_LOW = 5,
       CGS_H5_ENC1_BWD_DATA_POOLED = 6, /* src_a = dP bf16 [n,32,32,8], src_b = addend or NULL, codes = the forward argmax bytes (read) */
       /* the 32x32 level: features.6 forward (e1 bf16 [n,32,32,8] -> e2 FP32 [n,16,16,8] + argmax bytes: the tail kernels' input), its data
        * gradient from the pooled gradient (as 6, one level down), dec_model.1 forward (cat(e1, nearest-up2(o2 bf16 [n,16,16,8])) -> o1) and
        * its data gradients (skip: bf16 [n,32,32,8]; low: cell sums, FP32 [n,16,16,8])                                                  */
       CGS_H5_ENC2_FWD = 7, CGS_H5_ENC2_BWD_DATA_POOLED = 8, CGS_H5_DEC1_FWD = 9, CGS_H5_DEC1_BWD_SKIP = 10, CGS_H5_DEC1_BWD_LOW = 11,
       CGS_H5_DEC1_FWD_F32B = 12 /* as 9 with src_b = o2 in FP32 [n,16,16,8] (the tail kernel's output: no bf16 copy) */ };
int cgs_bf16_h5conv(int32_t which, int32_t n, const void* src_a, const void* src_b, const float* w_hwio, const float* bias, void* out,
                    uint8_t* codes, cgs_stream_t stream);
/* Weight + bias gradient of the large-map layers of config 5 at chfak 1 (csrc/hwgrad.hip; same arithmetic as cgs_bf16_conv3x3_bwd_weight):
 * (hw, ca, cb, co) = (128,3,0,8) features.0, (128,3,8,16) masker.0, (128,16,0,1) masker.2, (64,8,0,8) features.3, (64,8,8,8) dec_model.0,
 * (32,8,0,8) features.6, (32,8,8,8) dec_model.1.
 * cgs_bf16_hwgrad_slabs: slab rows written for n images (0: not a dedicated shape).  a_kind: 0 bf16 [n,hw,hw,ca], 1 uint8 / 2 fp32 frames
 * [n,hw,hw,3]; src_b bf16 [n,hw/2,hw/2,cb] (nearest-upsampled x2); dy bf16 [n,hw,hw,co], or fp32 [n,hw,hw] when co == 1.              */
int cgs_bf16_hwgrad_slabs(int32_t n, int32_t hw, int32_t ca, int32_t cb, int32_t co);
int cgs_bf16_hwgrad(int32_t n, int32_t hw, int32_t ca, int32_t cb, int32_t co, int32_t a_kind, const void* src_a, const void* src_b,
                    const void* dy, float* slab, cgs_stream_t stream);
/* features.0 (hw 128, ca 3) / features.3 (hw 64, ca 8) / features.6 (hw 32, ca 8) with dY given as the pooled gradient dp bf16 [n,hw/2,hw/2,8] (+ addend or NULL) and the
 * forward pass's argmax bytes (what cgs_bf16_pool_expand would re-expand); slab rows = cgs_bf16_hwgrad_slabs(n, hw, ca, 0, 8).          */
int cgs_bf16_hwgrad_pooled(int32_t n, int32_t hw, int32_t ca, int32_t a_kind, const void* src_a, const void* dp, const void* addend,
                           const uint8_t* codes, float* slab, cgs_stream_t stream);

/* ---- the 16x16-and-smaller layers, image by image inside one workgroup ("tail" kernels, csrc/tail.hip) ------------
 * Replace, for one critic pass / the decoder, the per-layer launches of features.6, features.10 (nets.py:176-183), the
 * critic head features.14 + crit.1 + crit.4 (nets.py:184-194) and dec_model.4/.3/.2/.1 (nets.py:501-513): every
 * intermediate stays in LDS, the convolutions run on the matrix cores, the same tensors as the per-layer entry points are
 * written (so either form feeds the other's backward).  Weight pointers are the kernel-layout (HWIO / k-major) tensors of
 * the flat parameter buffer.  Shapes (NHWC): e1 [n,16,16,8], e2 [n,8,8,8], am2 [n,8,8,1], e3 [n,4,4,16], am3 [n,4,4,2],
 * e4/h1/o4 [n,32], pred [n], o3 [n,4,4,16], o2 [n,8,8,8], o1 [n,16,16,8].                                            */
typedef struct {
    const float *w6, *b6;     /* features.6   [3][3][8][8],  [8]  */
    const float *w10, *b10;   /* features.10  [3][3][8][16], [16] */
    const float *w14, *b14;   /* features.14  [256][32] (k = (y*4+x)*16+c), [32] */
    const float *wl1, *bl1;   /* crit.1       [32][32] k-major, [32] */
    const float *wl2, *bl2;   /* crit.4       [32], [1] */
    const float *wpw, *bpw;   /* dec_model.4  [32][32] k-major, [32]; only read when o4 / d_o4 is given */
} cgs_tail_enc_weights;
typedef struct {
    const float *w3, *b3;     /* dec_model.3  [3][3][48][16], [16] */
    const float *w2, *b2;     /* dec_model.2  [3][3][24][8],  [8]  */
    const float *w1, *b1;     /* dec_model.1  [3][3][16][8],  [8]  */
} cgs_tail_dec_weights;
/* drop_e2 / drop_e3 / drop_h1: Dropout in front of features.10, features.14 and crit.4 (base = first image * 128 / 64 / 8).
 * o4 may be NULL (no decoder follows this pass).                                                                      */
int cgs_tail_enc_fwd(int32_t n, const cgs_tail_enc_weights* w, const float* e1, float* e2, uint32_t* am2, float* e3,
                     uint32_t* am3, float* e4, float* h1, float* pred, float* o4, cgs_dropout drop_e2,
                     cgs_dropout drop_e3, cgs_dropout drop_h1, cgs_stream_t stream);
/* features.3 (cgs_conv3x3_fwd of the 8 -> 8 layer at 32x32: e0 [n,32,32,8] -> e1 [n,16,16,8] + am1, nets.py:173-175) and cgs_tail_enc_fwd in ONE
 * launch, one workgroup per image (round 4): e1 / am1 are written for the backward pass and the decoder as before, the tail stages read
 * the pooled map from the workgroup's LDS tile.  w3 / b3: features.3's HWIO weights and bias.                                          */
int cgs_enc1_tail_fwd(int32_t n, const cgs_tail_enc_weights* w, const float* e0, const float* w3, const float* b3, float* e1,
                      uint32_t* am1, float* e2, uint32_t* am2, float* e3, uint32_t* am3, float* e4, float* h1, float* pred, float* o4,
                      cgs_dropout drop_e2, cgs_dropout drop_e3, cgs_dropout drop_h1, cgs_stream_t stream);
/* The whole critic forward (nets.py:170-194) of an image in one workgroup (round 4): features.0 on uint8 frames x [n,64,64,3] or -- x_is_mix --
 * on the virtual mixes (x = the cgs_mix_src descriptor, as cgs_conv3x3_fwd with CGS_SRC_MIX) -> e0 [n,32,32,8] + am0, then cgs_enc1_tail_fwd.           */
int cgs_critic_fwd_fused(int32_t n, const cgs_tail_enc_weights* w, const void* x, int32_t x_is_mix, const float* w0, const float* b0,
                         float* e0, uint32_t* am0, const float* w3, const float* b3, float* e1, uint32_t* am1, float* e2, uint32_t* am2,
                         float* e3, uint32_t* am3, float* e4, float* h1, float* pred, float* o4, cgs_dropout drop_e2, cgs_dropout drop_e3,
                         cgs_dropout drop_h1, cgs_stream_t stream);
/* The same + (m0_pack != NULL; uint8 frames only, else CGS_ERR_BADARG) one extra workgroup that packs masker.0's HWIO weights w_m0 [9][11][16] into
 * the mask head forward's weight registers m0_pack [40 * 64], as cgs_tail_dec_fwd_pack's spare workgroup does (byte for byte): the launch in front
 * of cgs_dec_mask_fwd on the training path.                                                                                              */
int cgs_critic_fwd_fused_pack(int32_t n, const cgs_tail_enc_weights* w, const void* x, int32_t x_is_mix, const float* w0, const float* b0,
                              float* e0, uint32_t* am0, const float* w3, const float* b3, float* e1, uint32_t* am1, float* e2, uint32_t* am2,
                              float* e3, uint32_t* am3, float* e4, float* h1, float* pred, float* o4, cgs_dropout drop_e2, cgs_dropout drop_e3,
                              cgs_dropout drop_h1, const float* w_m0, float* m0_pack, cgs_stream_t stream);
int cgs_tail_dec_fwd(int32_t n, const cgs_tail_dec_weights* w, const float* e1, const float* e2, const float* e3,
                     const float* o4, float* o3, float* o2, float* o1, cgs_stream_t stream);
/* (round 6, BASELINE config 4: main.py:1130-1151 with fp16 conv kernels) cgs_tail_enc_fwd in eval mode and cgs_tail_dec_fwd in ONE launch with fp16
 * OPERANDS in every layer but the head's Linear layers (v_mfma_f32_16x16x16_f16, fp32 accumulation), one workgroup per image, storing only what the
 * -process path consumes (nets.py:176-194 + 501-513 in eval mode; csrc/tail_infer.hip): e1 [n,16,16,8] -> pred [n] and o1 [n,16,16,8] (both fp32);
 * the tiles between the layers hold halves and never leave the workgroup.  wd = NULL and o1 = NULL: the critic alone.  Used by the fused fp16
 * inference path (engine.infer(fp16=True)) and by config 5's inference.                                                                        */
int cgs_tail_infer_h16(int32_t n, const cgs_tail_enc_weights* we, const cgs_tail_dec_weights* wd, const float* e1, float* pred, float* o1,
                       cgs_stream_t stream);
/* cgs_tail_dec_fwd + (m0_pack != NULL) one extra workgroup that packs masker.0's HWIO weights w_m0 [9][11][16] into the mask head
 * forward's weight registers m0_pack [40 * 64] (cgs_mask_train_fwd_packed).                                                     */
int cgs_tail_dec_fwd_pack(int32_t n, const cgs_tail_dec_weights* w, const float* e1, const float* e2, const float* e3,
                          const float* o4, float* o3, float* o2, float* o1, const float* w_m0, float* m0_pack, cgs_stream_t stream);

/* Backward of the same layers.  cgs_tail_enc_bwd: one critic pass, from dpred [n] to de1 [n,16,16,8] (gradient w.r.t. e1,
 * input of features.3's backward).  dE1 / dE2 / dE3 (skip gradients from the decoder, shapes of e1 / e2 / e3) and d_o4 [n,32]
 * (gradient w.r.t. dec_model.4's output: its backward then runs here too) may be NULL; they are read for images < n_add.
 * Every workgroup writes one slab per convolution: cgs_tail_enc_bwd_slabs(n) slabs of slab10 [1152 + 16] (features.10) and
 * slab6 [576 + 8] (features.6); a NULL slab pointer skips that store (data gradient only).  The head's weight gradients are
 * sums of outer products over the batch: the kernel leaves the per-image vectors in hvec [n,384] (may be NULL:
 * [0,256) dropout(e3) | [256,288) dz4 | [288,320) dh1 | [320,352) dz2 h1 mask | [352] dz2) and cgs_tail_head_wgrad forms them
 * for up to two image ranges (the critic passes of a step; d_o4_k [n_o4_k,32] = that range's decoder gradient or NULL) as one
 * GEMM over the images: cgs_tail_head_wgrad_slabs(n0 + n1) slabs of
 *   slab_head [8192 + 32 + 1024 + 32 + 32 + 1]  (features.14 w,b | crit.1 w,b | crit.4 w,b -- contiguous in the flat buffer)
 *   slab_pw [1024 + 32] (dec_model.4; required when a d_o4 is given).
 * The loss gradient at pred is either given (dpred [n]) or, with dpred = NULL, derived in the kernel from target [n]:
 *   loss_scale * 2 (pred - target)   (MSE terms of main.py:380-411: loss_scale = weight / n), or with bce != 0
 *   loss_scale * (pred - target) / (pred (1 - pred))  (binary cross-entropy, --threshrew);  target = NULL: zero.
 * cgs_tail_dec_bwd: dec_model.1/.2/.3 from do1 [n,16,16,8]: skip gradients dE1/dE2/dE3, d_o4 [n,32], and
 * cgs_tail_dec_bwd_slabs(n) slabs of slab1 [1152 + 8], slab2 [1728 + 8], slab3 [6912 + 16].                          */
int cgs_tail_enc_bwd_slabs(int32_t n);
int cgs_tail_enc_bwd(int32_t n, const cgs_tail_enc_weights* w, const float* e1, const float* e2, const uint32_t* am2,
                     const float* e3, const uint32_t* am3, const float* e4, const float* h1, const float* pred,
                     const float* dpred, const float* target, float loss_scale, int32_t bce, const float* dE1, const float* dE2, const float* dE3, const float* d_o4,
                     int32_t n_add, float* de1, float* hvec, float* slab10, float* slab6,
                     cgs_dropout drop_e2, cgs_dropout drop_e3, cgs_dropout drop_h1, cgs_stream_t stream);
/* The same with dec_model.0's weight gradient (cgs_conv3x3_bwd_weight of that layer over n_r images: skip input e0_r [n_r,32,32,8],
 * low-resolution input o1_r [n_r,16,16,8], output gradient dy_r [n_r,32,32,8], slab_r [nslab_r][1160], nslab_r <= 4 n_r) computed by
 * nslab_r spare workgroups of the launch (slab_r = NULL: none).                                                                    */
int cgs_tail_enc_bwd_rider(int32_t n, const cgs_tail_enc_weights* w, const float* e1, const float* e2, const uint32_t* am2,
                           const float* e3, const uint32_t* am3, const float* e4, const float* h1, const float* pred,
                           const float* dpred, const float* target, float loss_scale, int32_t bce, const float* dE1, const float* dE2,
                           const float* dE3, const float* d_o4, int32_t n_add, float* de1, float* hvec, float* slab10, float* slab6,
                           cgs_dropout drop_e2, cgs_dropout drop_e3, cgs_dropout drop_h1,
                           int32_t n_r, const float* e0_r, const float* o1_r, const float* dy_r, float* slab_r, int32_t nslab_r,
                           cgs_stream_t stream);
/* cgs_tail_enc_bwd_rider AND the data-gradient half of features.3's backward (cgs_conv3x3_bwd_both of the 8 -> 8 layer at 32x32 with ReLU +
 * pool, nets.py:173-175 backward: d e1 re-expanded by the argmax nibbles am1 [n,16,16,1], weights w_enc1 (HWIO [3][3][8][8]), + the decoder's
 * skip gradient addend0 [n_addend,32,32,8] (NULL: none) -> de0 [n,32,32,8]) in ONE launch (round 5): every workgroup continues with the
 * convolution of the image(s) whose tail it just ran, so d e1 never crosses a launch boundary.  That layer's WEIGHT gradient: slab1 != NULL
 * (with e0 [n,32,32,8], the layer's input): formed here too, per workgroup over its own images, slab1 [cgs_tail_enc_bwd_slabs(n)][584] (the
 * partition of the sum over the images differs from cgs_conv3x3_bwd_weight's: equal up to fp32 summation order); slab1 = NULL: left to
 * extra workgroups of the features.0 backward launch that follows (cgs_enc0_bwd_mix_enc1 / cgs_enc0_wgrad_u8_with_head_enc1), which
 * reproduce cgs_conv3x3_bwd_both's slabs bit for bit.  de0 is bit-identical to the two-launch form either way.                     */
int cgs_tail_enc_bwd_enc1(int32_t n, const cgs_tail_enc_weights* w, const float* e1, const float* e2, const uint32_t* am2,
                          const float* e3, const uint32_t* am3, const float* e4, const float* h1, const float* pred,
                          const float* dpred, const float* target, float loss_scale, int32_t bce, const float* dE1, const float* dE2,
                          const float* dE3, const float* d_o4, int32_t n_add, float* de1, float* hvec, float* slab10, float* slab6,
                          cgs_dropout drop_e2, cgs_dropout drop_e3, cgs_dropout drop_h1,
                          int32_t n_r, const float* e0_r, const float* o1_r, const float* dy_r, float* slab_r, int32_t nslab_r,
                          const uint32_t* am1, const float* w_enc1, const float* addend0, int32_t n_addend, float* de0,
                          const float* e0, float* slab1, cgs_stream_t stream);
int cgs_tail_head_wgrad_slabs(int32_t n_total);
int cgs_tail_head_wgrad(int32_t n0, const float* hvec0, const float* e4_0, const float* d_o4_0, int32_t n_o4_0, int32_t n1,
                        const float* hvec1, const float* e4_1, const float* d_o4_1, int32_t n_o4_1, float* slab_head,
                        float* slab_pw, cgs_stream_t stream);
/* cgs_conv3x3_bwd_weight of features.0 on n uint8 frames (slab: cgs_conv3x3_bwd_weight_slabs rows of [224]) and cgs_tail_head_wgrad
 * (same arguments) as ONE launch: the head's small GEMM rides along as extra workgroups.                                        */
int cgs_enc0_wgrad_u8_with_head(int32_t n, const uint8_t* x_u8, const float* dy, const uint32_t* amask, float* slab,
                                int32_t n0, const float* hvec0, const float* e4_0, const float* d_o4_0, int32_t n_o4_0,
                                int32_t n1, const float* hvec1, const float* e4_1, const float* d_o4_1, int32_t n_o4_1,
                                float* slab_head, float* slab_pw, cgs_stream_t stream);
/* The same + features.3's weight gradient over n1w images (cgs_conv3x3_bwd_weight of the 8 -> 8 layer at 32x32 with ReLU + pool: input e0_1
 * [n1w,32,32,8], pooled output gradient dy1 [n1w,16,16,8], argmax nibbles am1, slab1 [nslab1][584], nslab1 = cgs_enc1_wgrad_rider_slabs(n1w))
 * as nslab1 more workgroups (slab1 = NULL: none) -- the weight-gradient half that cgs_tail_enc_bwd_enc1 leaves behind (round 5).        */
int cgs_enc1_wgrad_rider_slabs(int32_t n);
int cgs_enc0_wgrad_u8_with_head_enc1(int32_t n, const uint8_t* x_u8, const float* dy, const uint32_t* amask, float* slab,
                                     int32_t n0, const float* hvec0, const float* e4_0, const float* d_o4_0, int32_t n_o4_0,
                                     int32_t n1, const float* hvec1, const float* e4_1, const float* d_o4_1, int32_t n_o4_1,
                                     float* slab_head, float* slab_pw,
                                     int32_t n1w, const float* e0_1, const float* dy1, const uint32_t* am1, float* slab1, int32_t nslab1,
                                     cgs_stream_t stream);
int cgs_tail_dec_bwd_slabs(int32_t n);
int cgs_tail_dec_bwd(int32_t n, const cgs_tail_dec_weights* w, const float* e1, const float* e2, const float* e3,
                     const float* o4, const float* o3, const float* o2, const float* do1, float* dE1, float* dE2,
                     float* dE3, float* d_o4, float* slab3, float* slab2, float* slab1, cgs_stream_t stream);
/* dec_model.0's data gradient (cgs_conv3x3_bwd_data of the 16 -> 8 layer at 32x32: dy_o0 [n,32,32,8] -> dE0 [n,32,32,8] = the skip
 * gradient at e0, do1 [n,16,16,8] = the cell-summed gradient at o1) and cgs_tail_dec_bwd (which consumes that do1) in ONE launch, one
 * workgroup per image (round 4).  n <= cgs_tail_dec_bwd_slabs(n) (one slab row per image), else CGS_ERR_UNSUPPORTED.               */
int cgs_dec0_tail_dec_bwd(int32_t n, const cgs_tail_dec_weights* w, const float* dy_o0, const float* w0_hwio, float* dE0, const float* e1,
                          const float* e2, const float* e3, const float* o4, const float* o3, const float* o2, float* do1, float* dE1,
                          float* dE2, float* dE3, float* d_o4, float* slab3, float* slab2, float* slab1, cgs_stream_t stream);
/* cgs_tail_dec_fwd_pack and dec_model.0's forward (cgs_conv3x3_fwd of the 16 -> 8 layer at 32x32: cat(e0, nearest-up(o1)) -> o0, linear;
 * nets.py:516-517) in ONE launch, one workgroup per image (round 4; n <= 1024, else CGS_ERR_UNSUPPORTED).                              */
int cgs_tail_dec_fwd_dec0(int32_t n, const cgs_tail_dec_weights* w, const float* e0, const float* e1, const float* e2, const float* e3,
                          const float* o4, float* o3, float* o2, float* o1, const float* w0_hwio, const float* b0, float* o0,
                          const float* w_m0, float* m0_pack, cgs_stream_t stream);
/* cgs_tail_dec_fwd_dec0 and cgs_mask_train_fwd_packed in ONE launch, one workgroup per image (round 7; nets.py:503-521, 488-491): the decoder
 * (dec_model.3 / .2 / .1 / .0 -> o3, o2, o1, o0, all stored) and then the mask head (masker.0 + LeakyReLU + masker.2 + sigmoid -> h [n,64,64,16],
 * z [n,64,64], zpart [n][2]) of the same image, bit-identical to the two launches.  x: uint8 frames [n,64,64,3] (src_a = CGS_SRC_U8); for
 * CGS_SRC_F32 and for n > 1024 the answer is CGS_ERR_UNSUPPORTED and the caller keeps the two launches.  m0_pack [40 * 64] (required) holds
 * masker.0's weight registers, built by an EARLIER launch (cgs_critic_fwd_fused_pack / cgs_tail_dec_fwd_pack).                              */
int cgs_dec_mask_fwd(int32_t n, const cgs_tail_dec_weights* w, const float* e0, const float* e1, const float* e2, const float* e3,
                     const float* o4, float* o3, float* o2, float* o1, const float* w0_hwio, const float* b0, float* o0, int32_t src_a,
                     const void* x, const float* b_m0, const float* w_m2, const float* b_m2, float* h, float* z, float* zpart,
                     const float* m0_pack, cgs_stream_t stream);

/* ---- convolution backward, weights --------------------------------------------------
 * Replaces convolution_backward(weight, bias).  Each workgroup writes one partial "slab"
 *   slab[b][0 .. 9*(ca+cb)*co)  = partial dW (HWIO),  slab[b][9*(ca+cb)*co ..][co] = partial dbias
 * and cgs_reduce_slabs() sums the slabs (deterministic, no float atomics).
 * cgs_conv3x3_bwd_weight_slabs() returns the number of slabs the launch will write (>0) or an error. */
int cgs_conv3x3_bwd_weight_slabs(const cgs_conv_desc* d);
int cgs_conv3x3_bwd_weight(const cgs_conv_desc* d, const void* src_a, const float* src_b,
                           const float* dy, const uint32_t* amask, float* slab,
                           cgs_stream_t stream);

/* ---- both backward halves of a SMALL layer in one launch ------------------------------
 * Same results as cgs_conv3x3_bwd_weight + cgs_conv3x3_bwd_data (identical device code), but the wgrad
 * workgroups and the data-gradient workgroups share one grid, so the two latency-bound halves overlap.
 * Supported: features.3/6/10, features.0 on fp32 input, dec_model.0-3, masker.0 (CGS_ERR_UNSUPPORTED otherwise).
 * d_a / d_b as for cgs_conv3x3_bwd_data (either may be NULL); slab as for cgs_conv3x3_bwd_weight with _both_slabs() slabs. */
int cgs_conv3x3_bwd_both_slabs(const cgs_conv_desc* d);
int cgs_conv3x3_bwd_both(const cgs_conv_desc* d, const void* src_a, const float* src_b, const float* dy,
                         const uint32_t* amask, const float* w_hwio, const float* addend, int32_t n_addend,
                         float* d_a, float* d_b, float* slab, cgs_stream_t stream);

/* One reduction job: dst[i] (+)= sum_{b<nslab} slab[b*stride + i], i < count. */
typedef struct {
    const float* slab;
    float* dst;
    int32_t nslab, stride, count;
    int32_t accumulate; /* 0: overwrite dst, 1: add to dst */
} cgs_reduce_job;
/* jobs: DEVICE array of njobs entries.  If step != NULL, *step is incremented by one (by one thread)
 * -- this is the per-iteration tick that Adam and the dropout masks read. */
int cgs_reduce_slabs(const cgs_reduce_job* jobs, int32_t njobs, int32_t max_count,
                     uint64_t* step, cgs_stream_t stream);

/* Single-GPU tail of a step in one launch: cgs_reduce_slabs, the Adam update (torch.optim.Adam defaults semantics as
 * cgs_adam_flat, grad_scale 1) of every element a job writes -- param / m / v are indexed by (job.dst - grad_base) -- and, when
 * n > 0, the loss values of cgs_phase2_losses (losses[8]; no dpred: the tail backward kernels derive it themselves).  *step is
 * read by every workgroup and advanced by one by the LAST workgroup to finish (ticket: device uint32 [njobs + 2], zero before
 * the first call; the kernel leaves it zero).  param == NULL: reduction, loss values and step tick only -- the data-parallel form:
 * the all-reduce of the gradient follows, then cgs_adam_flat (which reads the advanced *step).                                       */
int cgs_reduce_adam(const cgs_reduce_job* jobs, int32_t njobs, int32_t max_count, uint64_t* step, float* param,
                    const float* grad_base, float* m, float* v, float lr, float beta1, float beta2, float eps,
                    uint32_t* ticket, int32_t n, const float* pred, const float* y, const float* zpart, int32_t nzpart,
                    float lfak, float l1, float l2, int32_t flags, int64_t nz, float* losses, cgs_stream_t stream);

/* ---- features.0 backward of the replaced / injected passes + mix backward in one launch ----------------------
 * (main.py:395,406 backward chained onto convolution_backward of features.0).  n_a A-images; the mixes are images
 * [0,n_a) = replaced, [n_a,2 n_a) = injected (inject != 0).  dy [n_mix,32,32,8] + amask: gradient at features.0's pooled
 * output; slab [cgs_enc0_bwd_mix_slabs(n_mix)][224]: weight-gradient partials (NULL: data path only, frozen critic);
 * mixed [n_mix,64,64,3]: the weight gradient's input if the mixes were materialised, NULL: they are recomputed from a, b, z
 * in the tile loader (as cgs_conv3x3_fwd with CGS_SRC_MIX does).  a, b: uint8 frames [n_a,64,64,3]; z [n_a,64,64]; l1/l2_scale as cgs_mix_bwd.
 * Writes dzpre [n_a,64,64] = what cgs_conv3x3_bwd_data -> cgs_mix_bwd would (bit-identical); the image gradients are
 * never stored.                                                                                                  */
int cgs_enc0_bwd_mix_slabs(int32_t n_mix);
int cgs_enc0_bwd_mix(int32_t n_a, int32_t inject, const float* mixed, const float* dy, const uint32_t* amask,
                     const float* w_hwio, const uint8_t* a, const uint8_t* b, const float* z, float l1_scale,
                     float l2_scale, const float* valuefak_pred, float* dzpre, float* slab, cgs_stream_t stream);
/* The same + features.3's weight gradient over the n_mix mixes (e0_1 [n_mix,32,32,8], dy1 [n_mix,16,16,8], am1, slab1
 * [cgs_enc1_wgrad_rider_slabs(n_mix)][584]; all NULL: none) as extra workgroups of the launch (round 5, see cgs_tail_enc_bwd_enc1). */
int cgs_enc0_bwd_mix_enc1(int32_t n_a, int32_t inject, const float* mixed, const float* dy, const uint32_t* amask,
                          const float* w_hwio, const uint8_t* a, const uint8_t* b, const float* z, float l1_scale,
                          float l2_scale, const float* valuefak_pred, float* dzpre, float* slab,
                          const float* e0_1, const float* dy1, const uint32_t* am1, float* slab1, cgs_stream_t stream);
/* valuefak_pred (may be NULL): -staticnorm '' of main.py:415-418 -- the regulariser terms of A-image i are weighted by
 * (1 - valuefak_pred[i]) (L1) and its square (L2); with cgs_phase2_losses / cgs_reduce_adam the same weighting of the loss
 * VALUES is selected by flag bit 8 (weights from pred[n + i], zpart holding nzpart / n partial pairs per image).        */

/* ---- critic head: 4x4 valid conv + Linear + Linear (nets.py:184-194) -----------------
 *   e3     : [n,4,4,16] pooled embed (dropout `drop_in` fused into the load)
 *   w4     : [256][32]  (k = (y*4+x)*16 + c, HWIO of features.14), b4 [32]
 *   w1     : [32][32]   (k-major: crit.1.weight transposed), b1 [32];  w2 [32], b2 [1]
 *   e4     : [n,32] post-ReLU bottleneck (embeds[4]);  h1 : [n,32] post-ReLU hidden (pre-dropout)
 *   pred   : [n] sigmoid output.
 *   o4     : optional [n,32] = the DECODER's bottleneck 1x1 conv of e4 (nets.py:501, weights w_pw [32][32] k-major and
 *            b_pw [32] of dec_model.4) computed from the e4 row while it is on chip; NULL: not computed
 *            (cgs_pointwise_fwd is the stand-alone form).                                     */
int cgs_head_fwd(int32_t n, const float* e3, const float* w4, const float* b4, const float* w1,
                 const float* b1, const float* w2, const float* b2, cgs_dropout drop_in,
                 cgs_dropout drop_h, float* e4, float* h1, float* pred, const float* w_pw,
                 const float* b_pw, float* o4, cgs_stream_t stream);
/* Backward of the head.  dpred [n]; d_e4_extra / d_e3_extra: optional [n_extra,32] / [n_extra,4,4,16]
 * gradients arriving at e4 / e3 from the decoder (images < n_extra; d_e3_extra may alias d_e3).
 * Writes d_e3 [n,4,4,16] = head gradient (dropout mask applied) + d_e3_extra, and one slab per
 * workgroup: [w4 8192 | b4 32 | w1 1024 | b1 32 | w2 32 | b2 1] = 9313 floats.
 * d_o4 (optional, [n_extra,32]): gradient w.r.t. the decoder bottleneck output o4 instead of (or besides)
 * d_e4_extra: the 1x1 conv's backward runs here too (d e4 += W_pw d_o4) and its weight/bias gradient goes to
 * slab_pw [cgs_head_bwd_slabs(n)][1056] (layout of cgs_pointwise_bwd's slab).                 */
int cgs_head_bwd_slabs(int32_t n);
int cgs_head_bwd(int32_t n, const float* e3, const float* e4, const float* h1, const float* pred,
                 const float* dpred, const float* d_e4_extra, const float* d_e3_extra, int32_t n_extra,
                 const float* w4,
                 const float* w1, const float* w2, cgs_dropout drop_in, cgs_dropout drop_h,
                 float* d_e3, float* slab, const float* d_o4, const float* w_pw, float* slab_pw,
                 cgs_stream_t stream);

/* ---- decoder 1x1 conv on the bottleneck (nets.py:484,501) --------------------------
 *   y[n][o] = sum_k x[n][k] * w[k][o] + b[o],  32 -> 32 (MFMA v_mfma_f32_32x32x2_f32).      */
int cgs_pointwise_fwd(int32_t n, int32_t ci, int32_t co, const float* x, const float* w,
                      const float* b, float* y, cgs_stream_t stream);
int cgs_pointwise_bwd_slabs(int32_t n);
/* dx[n][k] = sum_o dy[n][o] w[k][o];  slab[b] = [dW ci*co | db co] partials. */
int cgs_pointwise_bwd(int32_t n, int32_t ci, int32_t co, const float* x, const float* dy,
                      const float* w, float* dx, float* slab, cgs_stream_t stream);

/* ---- mask replace / inject mix (main.py:395,406) --------------------------------------
 *   rep = A(1-Z) + Z B,  inj = B(1-Z) + Z A  with A,B uint8 NHWC (/255 fused), Z [n,64,64].
 *   mixed : [2n,h,w,3] fp32 (rep images then inj images; inj skipped when inject == 0)
 *   zpart : device float[2 * cgs_mix_fwd_partials(n,hw)]: per-workgroup partial (sum |Z|, sum Z^2),
 *           summed by cgs_phase2_losses (fixed order: no float atomics).  The count is a multiple of n and
 *           partial i covers only pixels of image i / (count / n), at every n (flag bit 8 relies on it). */
int cgs_mix_fwd_partials(int32_t n, int32_t hw);
int cgs_mix_fwd(int32_t n, int32_t hw, const uint8_t* a, const uint8_t* b, const float* z,
                int32_t inject, float* mixed, float* zpart, cgs_stream_t stream);
/* dzpre = (sum_c (B-A)_c (dRep_c - dInj_c) + l1*sign(Z) + 2*l2*Z) * Z(1-Z): the gradient w.r.t. the
 * mask head's pre-sigmoid output, regularisers (main.py:421-429) included. */
int cgs_mix_bwd(int32_t n, int32_t hw, const uint8_t* a, const uint8_t* b, const float* z,
                const float* dmixed, int32_t inject, float l1_scale, float l2_scale,
                float* dzpre, cgs_stream_t stream);
/* The same with -staticnorm '' (main.py:415-418): the regulariser terms of A-image i are weighted by valuefak = 1 - valuefak_pred[i]
 * (L1) and its square (L2); valuefak_pred [n] (the detached critic values of A) may be NULL (= cgs_mix_bwd).  hw = pixels per image. */
int cgs_mix_bwd_weighted(int32_t n, int32_t hw, const uint8_t* a, const uint8_t* b, const float* z, const float* dmixed,
                         int32_t inject, float l1_scale, float l2_scale, const float* valuefak_pred, float* dzpre,
                         cgs_stream_t stream);

/* ---- losses (main.py:380-384,400,411,421-429 and main.py:192-195) --------------------
 * pred layout [4n]: slots [B | A | replaced | injected].  y [n].  zpart/nzpart from cgs_mix_fwd.
 * losses[8] = {critic, replace, inject, l1, l2, total, 0, 0};  dpred [4n] = d total / d pred.
 * flags: bit0 live, bit1 inject, bit2 bce (--threshrew).  nz = n*h*w (mask elements).        */
int cgs_phase2_losses(int32_t n, const float* pred, const float* y, const float* zpart,
                      int32_t nzpart, float lfak, float l1, float l2, int32_t flags, int64_t nz,
                      float* losses, float* dpred, cgs_stream_t stream);
/* phase 1: loss = mse(pred, y) or bce; losses[0] = loss; dpred [n]. */
int cgs_phase1_loss(int32_t n, const float* pred, const float* y, int32_t bce, float* losses,
                    float* dpred, cgs_stream_t stream);

/* ---- Adam, flat (torch.optim.Adam defaults semantics; main.py:178,330-334,463) --------
 * t = *step (already ticked by cgs_reduce_slabs).  grad_scale multiplies the gradient as it is read
 * (1/world_size after a sum all-reduce; 1 otherwise). */
int cgs_adam_flat(int64_t count, float* param, const float* grad, float* m, float* v,
                  const uint64_t* step, float lr, float beta1, float beta2, float eps,
                  float grad_scale, cgs_stream_t stream);

/* ---- layout helpers (module API boundary: the reference hands NCHW fp32 tensors) ------ */
int cgs_nchw_to_nhwc(int32_t n, int32_t c, int32_t hw, const float* src, float* dst, cgs_stream_t stream);
int cgs_nhwc_to_nchw(int32_t n, int32_t c, int32_t hw, const float* src, float* dst, cgs_stream_t stream);
/* Writes the keep-mask multipliers (0 or 1/(1-p)) a dropout descriptor generates for `count` floats
 * (count % 4 == 0): test hook used to feed the SAME masks to the CPU oracle. */
int cgs_dropout_mask(cgs_dropout d, int64_t count, float* out, cgs_stream_t stream);

/* Library / device info: returns the gfx arch string the library was built for. */
/* ---- shape-generic kernels (csrc/gen.hip): model sizes outside the specialised set ---------------------------------
 * NewCritic / UnetDecoder with chfak != 1 (nets.py:166,184,190; the paper's model is chfak = 5) and the legacy `Unet` with its
 * ConvTranspose2d(4,2,1) decoder and LeakyReLU(0.2) (nets.py:356-449).  NHWC fp32 (source A optionally uint8, /255 fused),
 * runtime channel counts, weights in kernel layout (HWIO; [k][n] for GEMMs; [ky][kx][ci][co] for the transposed conv).
 * cgs_gen_conv_pack_weights: HWIO w [9][ca+cb][co] -> the convolution's weight operand wp (cgs_gen_conv_packed_floats floats:
 *   register images [16-channel chunk][tap][4-channel output group][64 lanes], zero for padding, csrc/gen4.hip).  transposed = 1
 *   (cb = 0): w is the HWIO weight [9][co][ca] of the LAYER whose data gradient is wanted (ca = its output channels = dY's, co =
 *   its input channels): wp is then the operand of cgs_gen_conv3x3_bwd_data (taps reversed, channels transposed).
 * cgs_gen_conv3x3_fwd: out = act(conv3x3(cat(A [ca], nearest-up_ups(B [cb])), wp) + bias), hw in {4,8,16,32,64}; pool = 1:
 *   MaxPool2d(2) of it, out [n,hw/2,hw/2,co] and argmax [same] = position 0..3 of the first maximum in bits 0-1 (may be NULL).
 *   transposed = 2 + cgs_gen_conv3x3_fwd_folded: the same layer over cat(A, nearest-up_2(B)) (cb > 0, hw >= 16, no pooling) with B read at
 *   its own resolution: a pixel of parity (py, px) sees B through the 2 x 2 cells around it, its nine taps over the upsampled map sum to four
 *   (weights added per parity by the pack, cgs_gen_conv_packed_floats_folded floats) -- 4 / 9 of the matrix work for B's channels.
 * cgs_gen_gemm: out [m,n] = act(x [m,k] w [k,n] + bias [n] (may be NULL)).
 * cgs_gen_convt4s2_*: ConvTranspose2d(4,2,1) over cat(A, B) [n,h,h,*] -> [n,2h,2h,co]: forward (+bias, act), data gradient
 *   (dy = gradient at the PRE-activation output; da / db may be NULL), weight + bias gradient (dw [16*(ca+cb)*co], dbias [co]). */
int64_t cgs_gen_conv_packed_floats(int32_t ca, int32_t cb, int32_t co);
int64_t cgs_gen_conv_packed_floats_folded(int32_t ca, int32_t cb, int32_t co);
int cgs_gen_conv_pack_weights(int32_t ca, int32_t cb, int32_t co, int32_t transposed, const float* w, float* wp,
                              cgs_stream_t stream);
/* The data gradient's operand for a window of the layer's input channels: w = HWIO [9][ci_layer][co_layer]; wp
 * (cgs_gen_conv_packed_floats(co_layer, 0, ci_n) floats) maps dY to d(input channels [ci_off, ci_off + ci_n)).                   */
int cgs_gen_conv_pack_weights_window(int32_t co_layer, int32_t ci_layer, int32_t ci_off, int32_t ci_n, const float* w, float* wp,
                                     cgs_stream_t stream);

/* All 3x3 layers' operands of one training step in ONE launch (the step packs ~25 of them: weights change at every Adam step).
 * Job i is cgs_gen_conv_pack_weights(ca, cb, co, transposed, w, wp) when ci_layer == 0 and
 * cgs_gen_conv_pack_weights_window(ca, ci_layer, ci_off, co, w, wp) when ci_layer > 0 (transposed must be 1).  jobs: HOST array. */
typedef struct cgs_gen_pack_job {
    const float* w; float* wp;
    int32_t ca, cb, co, transposed, ci_layer, ci_off;
} cgs_gen_pack_job;
int cgs_gen_conv_pack_batch(const cgs_gen_pack_job* jobs, int32_t njobs, cgs_stream_t stream);
int cgs_gen_conv3x3_fwd(int32_t n, int32_t hw, int32_t ca, int32_t cb, int32_t co, int32_t a_is_u8, int32_t ups,
                        int32_t act, float slope, int32_t pool, const void* src_a, const float* src_b, const float* wp,
                        const float* bias, float* out, uint8_t* argmax, cgs_stream_t stream);
int cgs_gen_conv3x3_fwd_folded(int32_t n, int32_t hw, int32_t ca, int32_t cb, int32_t co, int32_t a_is_u8, int32_t act, float slope,
                               const void* src_a, const float* src_b, const float* wp, const float* bias, float* out, cgs_stream_t stream);
/* features.0 of NewCritic at chfak 2 / 3 / 4 / 5 (co = 16 / 24 / 32 / 40; nets.py:170-172) on kernels of their own (csrc/gen_enc0.hip): same
 * tensors as cgs_gen_conv3x3_fwd(hw 64, ca 3, ReLU, pool) -- out [n,32,32,co] + argmax bytes (am may be NULL) -- from x = uint8 (x_is_u8) or
 * fp32 frames [n,64,64,3] and the layer's HWIO weights [9][3][co] (not packed).  CGS_ERR_UNSUPPORTED for other channel counts.          */
int cgs_gen_enc0_fwd(int32_t n, int32_t co, int32_t x_is_u8, const void* x, const float* w_hwio, const float* bias, float* out, uint8_t* am,
                     cgs_stream_t stream);
/* ... and the layer's weight + bias gradient: slab rows [cgs_gen_enc0_bwd_weight_slabs(n, co)][27 co + co] (-> cgs_reduce_slabs) from the frames,
 * the pooled gradient de [n,32,32,co] and the forward pass's argmax bytes (the tensors of cgs_gen_conv3x3_bwd_weight(hw 64, ca 3, cb 0)).   */
int cgs_gen_enc0_bwd_weight_slabs(int32_t n, int32_t co);
int cgs_gen_enc0_bwd_weight(int32_t n, int32_t co, int32_t x_is_u8, const void* x, const float* de, const uint8_t* am, float* slab,
                            cgs_stream_t stream);
/* ... and its data gradient (the image gradient of the mixes): d x [n,64,64,3] from de, am and the layer's raw HWIO weights (the tensors of
 * cgs_gen_conv3x3_bwd_data(hw 64, co, ci 3, dy_argmax)).                                                                                 */
int cgs_gen_enc0_bwd_data(int32_t n, int32_t co, const float* de, const uint8_t* am, const float* w_hwio, float* dx, cgs_stream_t stream);
int cgs_gen_gemm(int32_t m, int32_t k, int32_t n, int32_t act, float slope, const float* x, const float* w,
                 const float* bias, float* out, cgs_stream_t stream);

/* Training pass at chfak != 1 (csrc/gen_train.hip; backward of nets.py:197-212, 494-523 for any channel count).
 * cgs_gen_conv3x3_fwd's argmax byte carries bit 2 (value >= 4) where a ReLU'd pooled value is <= 0: no gradient there.
 * cgs_gen_flip_weights: HWIO w [9][ci][co] -> wflip [9][co][ci] with the taps reversed (the data gradient's kernel in HWIO form:
 *   cgs_gen_conv_pack_weights(co, 0, ci, 0, wflip) == cgs_gen_conv_pack_weights(co, 0, ci, 1, w)).
 * cgs_gen_conv3x3_bwd_data: d_cat [n,hw,hw,ci] = conv3x3(dY, wp) (+ addend [n_addend,hw,hw,ci] for images < n_addend), wp =
 *   cgs_gen_conv_pack_weights(co, 0, ci, transposed = 1, the layer's HWIO weights).  dY is the
 *   gradient at the pre-activation output [n,hw,hw,co], or -- dy_argmax != NULL, a max-pooled ReLU layer -- the gradient dE
 *   [n,hw/2,hw/2,co] at the pooled output with the forward pass's argmax bytes (re-expanded in the tile loader).
 * cgs_gen_conv3x3_bwd_weight: one slab row [9*(ca+cb)*co | co] (HWIO dW, dbias) per image share, cgs_gen_conv3x3_bwd_weight_slabs
 *   rows, to be summed by cgs_reduce_slabs; the layer input is cat(A, nearest-up_ups(B)) as in the forward call.
 * cgs_gen_cat_split: d_cat [n,hw,hw,ca+cb] -> d_a [n,hw,hw,ca] and d_b [n,hw/ups,hw/ups,cb] (sum over each ups x ups cell); either
 *   output may be NULL.
 * cgs_gen_grad_fix: d[i] = (d[i] * dropout multiplier + (i < addend_count ? addend[i] : 0)) * act'(saved[i]) in place; saved (the
 *   layer's stored OUTPUT; NULL: no activation factor), addend and the dropout (p = 0) are optional.
 * cgs_gen_dropout_fwd: out = x * keep-mask / (1 - p) (count % 4 == 0; the mask stream of cgs_dropout_mask).
 * cgs_gen_gemm_ex: out [m,n] (+)= act(sum_k x[m sxm + k sxk] w[k swk + n swn] + bias[n]) -- Linear layers and their gradients.
 * cgs_gen_u8_to_f32: out = x / 255.                                                                                         */
int cgs_gen_flip_weights(int32_t ci, int32_t co, const float* w, float* wflip, cgs_stream_t stream);
int cgs_gen_conv3x3_bwd_data(int32_t n, int32_t hw, int32_t co, int32_t ci, const float* dy, const uint8_t* dy_argmax,
                             const float* wp, const float* addend, int32_t n_addend, float* d_cat, cgs_stream_t stream);
/* d_cat of a layer over cat(A [ca], nearest-up_ups(B [cb])) written straight as d_a [n,hw,hw,ca] (NULL: not wanted) and d_b
 * [n,hw/ups,hw/ups,cb] (sum over each ups x ups cell): cgs_gen_conv3x3_bwd_data + cgs_gen_cat_split without the d_cat tensor; wp as for
 * cgs_gen_conv3x3_bwd_data with ci = ca + cb (ca = 0, d_a = NULL: the operand of a channel window that lies entirely in B,
 * cgs_gen_conv_pack_weights_window).  CGS_ERR_UNSUPPORTED when ca is not a multiple of the kernel's output pass width.          */
int cgs_gen_conv3x3_bwd_data_split(int32_t n, int32_t hw, int32_t co, int32_t ca, int32_t cb, int32_t ups, const float* dy,
                                   const float* wp, float* d_a, float* d_b, cgs_stream_t stream);
/* The second output of cgs_gen_conv3x3_bwd_data_split for ups = 2 alone, computed at the source's resolution: d_b [n,hw/2,hw/2,ci_n] = the gradient of
 * the x2-upsampled input channels [ci_off, ci_off + ci_n) of a layer (HWIO w [9][ci_layer][co_layer]) summed over each 2 x 2 cell, from dy [n,hw,hw,co_layer]
 * read as its space-to-depth view -- 16 (parity block, cell offset) steps per channel and cell instead of 9 taps per pixel + the cell sum (36).
 * hw 16 / 32 / 64, co_layer % 4 == 0; operand: cgs_gen_conv_pack_weights_up2 (cgs_gen_conv_packed_floats_up2(co_layer, ci_n) floats; in
 * cgs_gen_conv_pack_batch: transposed = 3 with ca = co_layer, co = ci_n, ci_layer, ci_off).                                                     */
int64_t cgs_gen_conv_packed_floats_up2(int32_t co_layer, int32_t ci_n);
int cgs_gen_conv_pack_weights_up2(int32_t co_layer, int32_t ci_layer, int32_t ci_off, int32_t ci_n, const float* w, float* wp, cgs_stream_t stream);
int cgs_gen_conv3x3_bwd_data_up2(int32_t n, int32_t hw, int32_t co_layer, int32_t ci_n, const float* dy, const float* wp, float* d_b,
                                 cgs_stream_t stream);
int cgs_gen_conv3x3_bwd_weight_slabs(int32_t n, int32_t ca, int32_t cb, int32_t co);
int cgs_gen_conv3x3_bwd_weight(int32_t n, int32_t hw, int32_t ca, int32_t cb, int32_t co, int32_t a_is_u8, int32_t ups,
                               const void* src_a, const float* src_b, const float* dy, const uint8_t* dy_argmax, float* slab,
                               cgs_stream_t stream);
/* The same slab rows for a layer over cat(A, nearest-up_2(B)) (hw 16 / 32 / 64, cb 16 / 24 / 32 / 40, dY not pooled) with B read at its own
 * resolution: per pixel parity the nine taps over the upsampled map are four folds of B's 2 x 2 cells -- 4 cb instead of 9 cb GEMM rows
 * (csrc/gen_wgrad_fold.h); A's rows and the bias row come from the row-block kernel.  _slabs: rows per layer (<= 0: not supported);
 * CGS_ERR_UNSUPPORTED is returned before anything is launched.                                                                    */
int cgs_gen_conv3x3_bwd_weight_folded_slabs(int32_t n, int32_t hw, int32_t ca, int32_t cb, int32_t co);
int cgs_gen_conv3x3_bwd_weight_folded(int32_t n, int32_t hw, int32_t ca, int32_t cb, int32_t co, int32_t a_is_u8, const void* src_a,
                                      const float* src_b, const float* dy, float* slab, cgs_stream_t stream);
int cgs_gen_cat_split(int32_t n, int32_t hw, int32_t ca, int32_t cb, int32_t ups, const float* d_cat, float* d_a, float* d_b,
                      cgs_stream_t stream);
int cgs_gen_grad_fix(int64_t count, float* d, const float* saved, int32_t act, float slope, const float* addend,
                     int64_t addend_count, cgs_dropout drop, cgs_stream_t stream);
int cgs_gen_dropout_fwd(int64_t count, const float* x, float* out, cgs_dropout drop, cgs_stream_t stream);
int cgs_gen_gemm_ex(int32_t m, int32_t k, int32_t n, const float* x, int64_t sxm, int64_t sxk, const float* w, int64_t swk,
                    int64_t swn, const float* bias, int32_t act, float slope, int32_t accumulate, float* out, cgs_stream_t stream);
/* Split-K form for the long reductions over the batch (X^T dY of the Linear layers, column sums): K share y of nsplit writes its
 * partial product to slab[y][m*n]; the rows are summed in order by cgs_reduce_slabs with the 3x3 layers' slabs
 * (reference: the autograd of nn.Linear, nets.py:187-194, 462-464). */
int cgs_gen_gemm_ex_splitk(int32_t m, int32_t k, int32_t n, const float* x, int64_t sxm, int64_t sxk, const float* w,
                           int64_t swk, int64_t swn, int32_t nsplit, float* slab, cgs_stream_t stream);
int cgs_gen_u8_to_f32(int64_t count, const uint8_t* x, float* out, cgs_stream_t stream);

/* ---- fp16 inference family (csrc/gen_f16.hip): BASELINE config 4, "-process inference-only mask path ... fp16 conv kernels" --------
 * Every layer of the eval-mode forward (nets.py:197-212, 494-523; main.py:1130-1151) with fp16 activations (NHWC) and fp16 weights,
 * fp32 accumulation on v_mfma_f32_16x16x16_f16, runtime channel counts (any chfak).  Opt-in: ~1e-3 absolute in the masks.
 * cgs_gen16_pack_weights: HWIO fp32 w [9][ca+cb][co] -> the kernel's fp16 operand layout (cgs_gen16_packed_weight_halves halves).
 * cgs_gen16_conv3x3_fwd: out = act(conv3x3(cat(A, nearest-up_ups(B))) + bias) (+ MaxPool2d(2)); A uint8 (/255 fused) or fp16
 *   (ca % 4 == 0), B fp16; out fp16, or fp32 when out_is_f32.
 * cgs_gen16_gemm: out [m,n] = act(x [m,k] w [k,n] + bias), x fp16 or fp32, w / bias fp32, out fp16 or fp32.                         */
int64_t cgs_gen16_packed_weight_halves(int32_t ca, int32_t cb, int32_t co);
int cgs_gen16_pack_weights(int32_t ca, int32_t cb, int32_t co, const float* w, void* w16, cgs_stream_t stream);
int cgs_gen16_conv3x3_fwd(int32_t n, int32_t hw, int32_t ca, int32_t cb, int32_t co, int32_t a_is_u8, int32_t ups, int32_t act,
                          float slope, int32_t pool, int32_t out_is_f32, const void* src_a, const void* src_b, const void* w16,
                          const float* bias, void* out, cgs_stream_t stream);
int cgs_gen16_gemm(int32_t m, int32_t k, int32_t n, int32_t act, float slope, int32_t x_is_f16, int32_t out_is_f16, const void* x,
                   const float* w, const float* bias, void* out, cgs_stream_t stream);

/* ---- bfloat16 form of the same family (BASELINE config 5: "128x128x3 frames ... bf16 with MFMA 1x1 pointwise") -----------------------
 * The same kernels with bf16 activations / weights (fp32 accumulation on v_mfma_f32_16x16x16_bf16), additionally at map size 128:
 * the build-defined six-stage 128x128 Hourglass (hourglass128.py; the reference cannot run 128x128 inputs -- nets.py:184,189-190 --
 * so this variant has no reference counterpart: parity unpinned, checked against the build's own fp32 restatement in oracle/).
 * Operand layout and packed size as cgs_gen16_* (cgs_gen16_packed_weight_halves 16-bit words).                                       */
int cgs_genbf16_pack_weights(int32_t ca, int32_t cb, int32_t co, const float* w, void* w16, cgs_stream_t stream);
int cgs_genbf16_conv3x3_fwd(int32_t n, int32_t hw, int32_t ca, int32_t cb, int32_t co, int32_t a_is_u8, int32_t ups, int32_t act,
                            float slope, int32_t pool, int32_t out_is_f32, const void* src_a, const void* src_b, const void* w16,
                            const float* bias, void* out, cgs_stream_t stream);
int cgs_genbf16_gemm(int32_t m, int32_t k, int32_t n, int32_t act, float slope, int32_t x_is_bf16, int32_t out_is_bf16, const void* x,
                     const float* w, const float* bias, void* out, cgs_stream_t stream);

/* ---- bf16 TRAINING of the build-defined 128x128 variant (BASELINE config 5; hourglass128.py; csrc/gen_bf16_train.hip) -------------------
 * No reference counterpart (the reference's 4x4 valid convolution nets.py:184 cannot take 128x128 frames): parity unpinned.
 * cgs_genbf16_conv3x3_fwd_train: cgs_genbf16_conv3x3_fwd with source A bf16 (a_kind 0), uint8 (1) or fp32 (2: the replaced / injected
 *   mixes) and, for pooled layers, codes [n,hw/2,hw/2,co] = the argmax position 0..3 of every pooled element (4: value <= 0).
 * cgs_genbf16_pack_weights_t: the data gradient's operand -- cgs_genbf16_conv3x3_fwd(ca = co_layer, cb = 0, co = ci_layer) on it computes
 *   d cat(A, up(B)) [n,hw,hw,ci_layer] from dY [n,hw,hw,co_layer] (packed size cgs_gen16_packed_weight_halves(co_layer, 0, ci_layer)).
 * cgs_bf16_conv3x3_bwd_weight: slab [cgs_bf16_conv3x3_bwd_weight_slabs(n,hw,ca,cb)][9 (ca+cb) co + co] = per-workgroup partial
 *   (dW in HWIO order | db) of conv3x3(cat(A, up_ups(B))) from dY [n,hw,hw,dy_channels] (bf16; columns >= co zero padding), on
 *   v_mfma_f32_16x16x32_bf16 with K = 32 pixels (operands through ds_read_b64_tr_b16); summed by cgs_reduce_slabs.
 * cgs_bf16_pool_expand: out [n,2hp,2hp,c] = (dp [n,hp,hp,c] (+ addend)) at the argmax position, 0 elsewhere (backward of ReLU + MaxPool2d(2)).
 * cgs_bf16_cat_split: d cat [n,hw,hw,ca+cb] -> dskip [n,hw,hw,ca] (may be NULL) and dlow [n,hw/ups,hw/ups,cb] (cell sums; fp32 when low_is_f32).
 * cgs_bf16_lrelu_bwd: d *= LeakyReLU'(h) in place.  cgs_bf16_convert: rows x c_src -> rows x c_dst (zero pad), fp32 -> bf16 or back.      */
int cgs_genbf16_conv3x3_fwd_train(int32_t n, int32_t hw, int32_t ca, int32_t cb, int32_t co, int32_t a_kind, int32_t ups, int32_t act,
                                  float slope, int32_t pool, int32_t out_is_f32, const void* src_a, const void* src_b, const void* w16,
                                  const float* bias, void* out, uint8_t* codes, cgs_stream_t stream);
int cgs_genbf16_pack_weights_t(int32_t ci_layer, int32_t co_layer, const float* w_hwio, void* w16, cgs_stream_t stream);
/* All bf16 operand copies of a step in one launch: jobs = DEVICE array of njobs entries; transposed = 0: cgs_genbf16_pack_weights(ca, cb, co),
 * 1: cgs_genbf16_pack_weights_t(ca + cb, co) of the layer whose HWIO weights are w.                                                       */
typedef struct cgs_gen16_pack_job {
    const float* w;
    void* out;
    int32_t ca, cb, co, transposed;
} cgs_gen16_pack_job;
int cgs_genbf16_pack_batch(const cgs_gen16_pack_job* jobs, int32_t njobs, cgs_stream_t stream);
int cgs_bf16_conv3x3_bwd_weight_slabs(int32_t n, int32_t hw, int32_t ca, int32_t cb);
int cgs_bf16_conv3x3_bwd_weight(int32_t n, int32_t hw, int32_t ca, int32_t cb, int32_t co, int32_t dy_channels, int32_t a_kind, int32_t ups,
                                const void* src_a, const void* src_b, const void* dy, float* slab, cgs_stream_t stream);
int cgs_bf16_pool_expand(int32_t n, int32_t hp, int32_t c, const void* dp, const void* addend, const uint8_t* codes, void* out,
                         cgs_stream_t stream);
int cgs_bf16_cat_split(int32_t n, int32_t hw, int32_t ca, int32_t cb, int32_t ups, const void* dcat, void* dskip, void* dlow,
                       int32_t low_is_f32, cgs_stream_t stream);
int cgs_bf16_lrelu_bwd(int64_t count, void* d, const void* h, float slope, cgs_stream_t stream);
int cgs_bf16_convert(int64_t rows, int32_t c_src, int32_t c_dst, int32_t to_f32, const void* src, void* dst, cgs_stream_t stream);
int cgs_gen_convt4s2_fwd(int32_t n, int32_t h, int32_t ca, int32_t cb, int32_t co, int32_t act, float slope,
                         const float* a, const float* b, const float* w, const float* bias, float* out,
                         cgs_stream_t stream);
int cgs_gen_convt4s2_bwd_data(int32_t n, int32_t h, int32_t ca, int32_t cb, int32_t co, const float* dy,
                              const float* w, float* da, float* db, cgs_stream_t stream);
int cgs_gen_convt4s2_bwd_weight(int32_t n, int32_t h, int32_t ca, int32_t cb, int32_t co, const float* a,
                                const float* b, const float* dy, float* dw, float* dbias, cgs_stream_t stream);

/* ---- contrastive batch assembly on the device (main.py:344-356, 584-591) ------------------------------------------
 * dst [n,64,64,3] uint8: frame src[idx[i]] of a device-resident uint8 frame set, rolled circularly along the width:
 * dst[i][y][x] = src[idx[i]][y][(x + shift_px) mod 64].  Handler.shift_batch's "left" roll by s pixels is shift_px = s, its
 * "right" roll shift_px = (64 - s) mod 64.  idx: device int64 [n].  cgs_gather_f32: dst[i] = src[idx[i]] (the targets). */
int cgs_gather_roll_u8(const uint8_t* src, const int64_t* idx, int32_t n, int32_t shift_px, uint8_t* dst,
                       cgs_stream_t stream);
int cgs_gather_f32(const float* src, const int64_t* idx, int32_t n, float* dst, cgs_stream_t stream);
/* The contrastive batch assembly of a phase-2 step in one launch (main.py:344-356 + shift_batch main.py:584-591): a [n,64,64,3] =
 * [xpos[idx[0..h)] | xneg[idx[h..n)]] rolled along the width by shift_px pixels (0 <= shift_px < 64), b [n,64,64,3] = xneg[idx[n..2n)] (not
 * rolled), y [n] = [ypos[idx[0..h)] | yneg[idx[h..n)]].  Equal to three cgs_gather_roll_u8 and two cgs_gather_f32 calls.                 */
int cgs_gather_contrastive(const uint8_t* xpos, const uint8_t* xneg, const float* ypos, const float* yneg, const int64_t* idx, int32_t n,
                           int32_t h, int32_t shift_px, uint8_t* a, uint8_t* b, float* y, cgs_stream_t stream);

/* ---- dense-CRF mask refinement (csrc/crf.hip; Handler.crf, main.py:1226-1263) -----------------------------------------------------
 * Two labels, Potts compatibility, the EXACT fully-connected mean field of DenseCRF2D's addPairwiseGaussian(gamma, Potts(w_gaussian)) +
 * addPairwiseBilateral(alpha, beta, frame, Potts(w_bilateral)) with symmetric normalisation and unary -ln P (no permutohedral lattice).
 * frames [n,h,w,3] uint8 (the colours), p1 [n,h,w] fp32: P(label 1), P(label 0) = 1 - p1; p1 of exactly 0 or 1 pins the label.
 * labels [n,h,w] uint8 in {0,1}: label 1 iff a_1 - a_0 > 0 after `iterations` mean-field steps (iterations = 0: iff p1 > 1 - p1).
 * q1_or_null [n,h,w] fp32 (optional): Q(label 1) after the last step.  Frames are independent: a frame's result does not depend on the
 * batch it is in, and the summation order is fixed (bitwise reproducible).  h * w <= 16384, else CGS_ERR_UNSUPPORTED; n >= 1, positive
 * stds and iterations >= 0, else CGS_ERR_BADARG.  Unlike the other entry points this one takes no workspace argument: it allocates its
 * scratch (10 floats per pixel of at most 2^22 pixels) stream-ordered (hipMallocAsync / hipFreeAsync) on `stream`.                      */
typedef struct {
    float w_bilateral, alpha, beta, w_gaussian, gamma;
    int32_t iterations;
} cgs_crf_params;
int cgs_dense_crf2(const uint8_t* frames, const float* p1, int32_t n, int32_t h, int32_t w, const cgs_crf_params* prm, uint8_t* labels,
                   float* q1_or_null, cgs_stream_t stream);

/* ---- evaluation-video frame composition (csrc/video.hip; Handler.eval's video, main.py:1027-1087) ------------------------------------
 * Replaces the host-side frame assembly of main.py:1039-1083: the np.concatenate of the tiles, (frames * 255).astype(np.uint8), the x3
 * F.interpolate (nearest) and the concatenation with the np.tile'd title and legend bands.
 * out [n, H, W, 3] uint8, H = h_top + 192 rows + h_bottom, W = 192 cols: rows 0..h_top-1 = top [h_top, W, 3]; then `rows` rows of
 * `cols` cells, cell (r, c) = cells[r * cols + c] shown x3 nearest; then bottom [h_bottom, W, 3].  Frame i of the chunk shows source
 * frame f0 + i of every cell.  A cell's source is a [>= f0 + n, 64, 64] stack (RGB8: [.., 64, 64, 3]) in device memory:
 *   CGS_VIDEO_RGB8   uint8 RGB frames: the pixel as it is (= uint8(255 (x / 255.0)) for every byte x);
 *   CGS_VIDEO_MASK8  uint8 0/1 mask: GREY 255 m; CODE against the truth y (uint8 0/1 [.., 64, 64]): TP (0,255,0), FN (255,0,0),
 *                    FP (127,127,127), TN (0,0,0) -- main.py:1050-1051 after *255;
 *   CGS_VIDEO_F32 / CGS_VIDEO_F64  fp32 / fp64 map in [0, 1]: GREY uint8(255.0 * (double)v) (truncation; outside [0, 1] clamped);
 * mode CGS_VIDEO_CONST: every pixel uint8(255.0 * value) (src unused; 0.1 gives 25).  CODE needs MASK8.  top / bottom / out 16-byte
 * aligned; flags: CGS_VIDEO_NONTEMPORAL = non-temporal stores.  1 <= n <= 65535, rows * cols <= CGS_VIDEO_MAX_CELLS, else
 * CGS_ERR_BADARG.  `cells` is HOST memory (copied into the launch).                                                                       */
enum { CGS_VIDEO_RGB8 = 0, CGS_VIDEO_MASK8 = 1, CGS_VIDEO_F32 = 2, CGS_VIDEO_F64 = 3 };
enum { CGS_VIDEO_GREY = 0, CGS_VIDEO_CODE = 1, CGS_VIDEO_CONST = 2 };
enum { CGS_VIDEO_MAX_CELLS = 16, CGS_VIDEO_NONTEMPORAL = 1 };
typedef struct {
    const void* src;
    const uint8_t* y;      /* CODE: the truth */
    double value;          /* CONST */
    int32_t kind, mode;
} cgs_video_cell;
int cgs_video_compose(const cgs_video_cell* cells, int32_t rows, int32_t cols, int32_t f0, int32_t n, const uint8_t* top, int32_t h_top,
                      const uint8_t* bottom, int32_t h_bottom, int32_t flags, uint8_t* out, cgs_stream_t stream);

/* ---- -viscritic / -vismasker frame composition (csrc/vis.hip; Handler.visualize's make_video, main.py:818-874) ----------------------
 * Replaces the host loop of main.py:835-870, run once per video: frames[:, sorting] (main.py:820-822), the np.concatenate of the tiles
 * and of the plotbar windows (main.py:839-849, make_plotbar main.py:31-41), cv2.resize x4 INTER_NEAREST (main.py:852), np.uint8, the
 * three PIL draw.text calls (main.py:856-862) and np.array(img).
 * One launch composes frames j0 .. j0 + n - 1 of one video into out [n, H, 256, 3] uint8, H = 4 (64 R + 32 CGS_VIS_VALUES).  Frame j
 * shows source frame p = perm[j] (perm_or_null int32 [N], the video's sorting; null = identity; entries are trusted):
 *   tile 0: X[p] (uint8 [N,64,64,3]) as it is;  tile 1 (R = 2): uint8(float32(X[p]) * masks[p]) -- one IEEE fp32 product per byte,
 *   truncated (main.py:811, 853); masks fp32 [N,64,64] in [0, 1];
 *   plot strip v (32 source rows, v = 0 ground truth, 1 prediction): column c shows index k = j + c - 32 of the PERMUTED sequence; when
 *   0 <= k < N the pixel at source row rows[v][perm[k]] (rows uint8 [CGS_VIS_VALUES, N], make_plotbar's ph - 1 - floor(ph x)) is white,
 *   in column 32 (the current frame) red; everything else black;
 *   every source pixel x4 nearest: out[y][x] = src[y / 4][x / 4];
 *   labels: label_ids int32 [N, 1 + CGS_VIS_VALUES] gives source frame p its cells of atlas (uint8 [n_labels, CGS_VIS_CELL_H,
 *   CGS_VIS_CELL_W], the coverage PIL rendered for each distinct string; an id outside [0, n_labels) draws nothing): first the index
 *   label at (CGS_VIS_INDEX_X, H - 269), then value label v at (CGS_VIS_VALUE_X, CGS_VIS_VALUE_Y + CGS_VIS_VALUE_DY v), each blended
 *   in that order per byte with PIL's v = dst (255 - a) + 255 a + 128; ((v >> 8) + v) >> 8, and clipped at the frame's right edge.
 * out 16-byte aligned; flags: CGS_VIS_NONTEMPORAL = non-temporal stores.  R in {1, 2}, masks required for R = 2, 0 <= j0, 1 <= n,
 * j0 + n <= N, else CGS_ERR_BADARG (nothing is launched).                                                                            */
enum { CGS_VIS_VALUES = 2, CGS_VIS_CELL_W = 64, CGS_VIS_CELL_H = 16, CGS_VIS_NONTEMPORAL = 1 };
enum { CGS_VIS_INDEX_X = 230, CGS_VIS_VALUE_X = 1, CGS_VIS_VALUE_Y = 1, CGS_VIS_VALUE_DY = 15 };
int cgs_vis_compose(const uint8_t* X, const float* masks_or_null, const int32_t* perm_or_null, const uint8_t* rows,
                    const int32_t* label_ids, const uint8_t* atlas, int32_t n_labels, int32_t N, int32_t R, int32_t j0, int32_t n,
                    int32_t flags, uint8_t* out, cgs_stream_t stream);

/* ---- mask-training PNG sheet (csrc/sheet.hip; Handler.segmentation_training's debug grid, main.py:465-496) -----------------------------
 * Replaces the host-side pixels of main.py:470-496: A / B / Z pulled to the host and permuted, the two mixes recomputed in torch on the
 * CPU, seven np.concatenate(viz, axis=1) rows (two of zeros), np.concatenate(vizs, axis=0) and np.uint8(255 * viz).  The text of
 * main.py:497-515 is NOT blended here: it is drawn on the host into the two zero rows (cgs_amd/sheets.py), off the step path.
 * A, B uint8 NHWC [n,64,64,3], Z fp32 [n,64,64] in [0, 1]; out uint8 [7 * 64, 64 n, 3] row-major, image i in columns 64 i .. 64 i + 63.
 * Rows of tiles, top to bottom: zeros, zeros, A, B, replaced = A (1 - Z) + Z B, injected = B (1 - Z) + Z A, Z on all three channels.
 * Every byte is np.uint8(255 * v) with v in fp32: a = float(u8) / 255.0f (a true division), then 1 - Z, both products, the sum and the
 * 255 * each rounded on its own in that operand order (no FMA), then truncated; for the A and B rows that gives back the frame's byte.
 * A, B, out 16-byte aligned; 1 <= n <= CGS_SHEET_MAX_N, else CGS_ERR_BADARG (nothing is launched).                                     */
enum { CGS_SHEET_ROWS = 7, CGS_SHEET_MAX_N = 1 << 20 };
int cgs_sheet_compose(const uint8_t* A, const uint8_t* B, const float* Z, int32_t n, uint8_t* out, cgs_stream_t stream);

/* ---- evaluation scoring (csrc/metrics.hip; Handler.get_iou main.py:1265-1270, the CRF grid's score main.py:1253, the commented
 * threshold grid of main.py:974-975) ---------------------------------------------------------------------------------------------------
 * Integer counts of intersection and union over a whole stack, taken where the data is: only 2 T (2 K) integers go back to the host.
 * Both run on `stream` without synchronising and can be captured in a graph; counts is written (not accumulated into).
 *
 * cgs_iou_curve: v fp32 [px], truth uint8 [px] (non-zero = set), thr fp32 [T] in DEVICE memory, ascending (duplicates allowed),
 * counts int64 [T][2]: counts[t] = (#{truth and on_t}, #{truth or on_t}) with on_t = v > thr[t] (inclusive = 0) or v >= thr[t]
 * (inclusive = 1), compared in fp32 as numpy compares a float32 array with a float32 scalar; a NaN in v is on for no threshold.
 * One pass over v and truth however large T is (two (T+1)-bin histograms of #{t : thr[t] < v}, then suffix sums).  Thresholds that
 * are not ascending give unspecified counts (no fault).  1 <= T <= 1024, px >= 1, inclusive in {0, 1}, v / thr 4-byte and counts
 * 8-byte aligned, else CGS_ERR_BADARG.  Like cgs_dense_crf2 it allocates its scratch (2 (T + 1) 64-bit bins) stream-ordered.
 *
 * cgs_iou_counts: labels uint8 [K][px] (non-zero = on), truth uint8 [px], counts int64 [K][2] = (#{truth and labels_k},
 * #{truth or labels_k}): K stacks scored against one truth in one launch.  K >= 1, px >= 1, counts 8-byte aligned, else
 * CGS_ERR_BADARG; CGS_ERR_UNSUPPORTED when K times the workgroups per stack (at most 1024 below 2^41 pixels) exceeds 2^31 - 1.
 * Neither needs px to be a multiple of anything, nor 16-byte aligned pointers.                                                        */
int cgs_iou_curve(const float* v, const uint8_t* truth, const float* thr, int32_t T, int32_t inclusive, int64_t px, int64_t* counts,
                  cgs_stream_t stream);
int cgs_iou_counts(const uint8_t* labels, const uint8_t* truth, int32_t K, int64_t px, int64_t* counts, cgs_stream_t stream);

/* ---- from masks to objects (csrc/objects.hip; this build's own -objects, no counterpart in the reference) --------------------------------
 * Connected-component labelling of n frames of h x w (contiguous), one workgroup per frame in LDS, with an area filter, the numbering
 * of scipy.ndimage.label and a table of the objects.  Integer throughout: deterministic, bit for bit the raster-scan flood fill.
 * src_kind says when a pixel is on: CGS_OBJ_U8 uint8, non-zero (a bool stack is this); CGS_OBJ_F32_GT fp32, v > thresh (-eval's compare);
 * CGS_OBJ_F32_GE fp32, v >= thresh (-process's compare); compared in fp32, a NaN is off.  connectivity 4 or 8.
 * Per frame: a component is a maximal connected set of on pixels; those with area >= min_area are kept and numbered 1..K in raster
 * order of their first pixel (the smallest y w + x).
 *   labels    int32 [n][h][w] or NULL: the number of the pixel's component, 0 for off pixels and removed components; every kept
 *             component is numbered, also those beyond max_objects
 *   kept_mask uint8 [n][h][w] or NULL: 1 where labels is non-zero
 *   count     int32 [n][2]: (kept, found), found counting the components before the filter
 *   table     int32 [n][max_objects][8] or NULL: row k-1 is object k: area, x0, y0, x1, y1 (inclusive bounds), sum_x, sum_y, first
 *             (the raster index of its first pixel); rows from min(kept, max_objects) on are zero
 * Runs on `stream` without synchronising, allocates nothing, can be captured in a graph.  1 <= h, w <= 64, else CGS_ERR_UNSUPPORTED;
 * src, count not NULL, n >= 1, a valid src_kind and connectivity, min_area >= 1, max_objects >= 1 (also when table is NULL), fp32 src /
 * labels / count / table 4-byte aligned, else CGS_ERR_BADARG (nothing is launched).                                                     */
enum { CGS_OBJ_U8 = 0, CGS_OBJ_F32_GT = 1, CGS_OBJ_F32_GE = 2 };
enum { CGS_OBJ_FIELDS = 8, CGS_OBJ_MAX_SIDE = 64 };
int cgs_objects_label(const void* src, int32_t src_kind, float thresh, int32_t n, int32_t h, int32_t w, int32_t connectivity,
                      int32_t min_area, int32_t max_objects, int32_t* labels, uint8_t* kept_mask, int32_t* count, int32_t* table,
                      cgs_stream_t stream);

/* ---- mask clean-up (csrc/clean.hip; this build's own --clean / --overlay-clean, no counterpart in the reference) -------------------------
 * The standard steps between a soft mask and its objects, for n frames of h x w (contiguous), one workgroup per frame, the frame as 64
 * bit rows in LDS.  Integer or pure selection throughout: deterministic, bit for bit.  The stages, in this fixed order:
 *   on     src_kind, thresh and NaN exactly as in cgs_objects_label (CGS_OBJ_U8, CGS_OBJ_F32_GT, CGS_OBJ_F32_GE; a NaN is off)
 *   hyst   (hyst != 0; fp32 sources only) a `connectivity`-connected (4 or 8) component of the on pixels is kept only when at least
 *          one of its pixels is strong: v > strong for _GT, v >= strong for _GE, compared in fp32
 *   open   by open_r, then close by close_r (each 0..CGS_CLEAN_MAX_RADIUS, 0: off).  Opening is erosion then dilation, closing dilation
 *          then erosion; a step over radius r is r iterations of the 8-neighbour step for CGS_CLEAN_SQUARE (the (2r+1)^2 square) and
 *          of the 4-neighbour step for CGS_CLEAN_CROSS (the diamond).  Dilation reads everything outside the frame as off, erosion
 *          reads it as ON (scipy's binary_dilation(border_value=0), binary_erosion(border_value=1)): a mask cut by the frame's edge is
 *          not eaten from the edge, opening stays anti-extensive and closing extensive, and both are idempotent
 *   fill   (fill_area 1..4096; 0: off) a hole is a component of OFF pixels at the complementary connectivity (4 when connectivity is
 *          8, 8 when it is 4) that has no pixel in the first or last row or column; a hole of at most fill_area pixels is turned on.
 *          fill_area = 4096 is scipy.ndimage.binary_fill_holes with the complementary structure
 *   out    uint8 [n][h][w], 0 / 1
 *   gated  fp32 [n][h][w] or NULL (fp32 sources with thresh > 0 only): 0 where out is 0; where out is 1, v when v passes the threshold
 *          compare and thresh otherwise (a filled or closed cell, a NaN).  No arithmetic: gated >= thresh reproduces out, and the
 *          soft values of surviving cells keep their bits
 *   counts int32 [n][CGS_CLEAN_FIELDS]: on pixels after the threshold, after hyst, after open, after close, after fill (a stage that
 *          is off repeats the count before it), components dropped by hyst, holes found, holes filled (both 0 with fill off)
 * Runs on `stream` without synchronising, allocates nothing, can be captured in a graph.  src, out, counts not NULL, n >= 1, a valid
 * src_kind, connectivity and shape, radii in 0..4, fill_area in 0..4096, hyst only with an fp32 source, a finite strong and strong >=
 * thresh, gated only with an fp32 source and thresh > 0, fp32 src / gated / counts 4-byte aligned, else CGS_ERR_BADARG; then 1 <= h, w
 * <= 64, else CGS_ERR_UNSUPPORTED.  A refused call launches nothing.                                                                    */
enum { CGS_CLEAN_FIELDS = 8, CGS_CLEAN_MAX_RADIUS = 4 };
enum { CGS_CLEAN_SQUARE = 0, CGS_CLEAN_CROSS = 1 };
int cgs_mask_clean(const void* src, int32_t src_kind, float thresh, int32_t hyst, float strong, int32_t n, int32_t h, int32_t w,
                   int32_t connectivity, int32_t shape, int32_t open_r, int32_t close_r, int32_t fill_area, uint8_t* out, float* gated,
                   int32_t* counts, cgs_stream_t stream);

/* ---- from objects to matches (csrc/objects_match.hip; this build's own -eval -objects --match-iou, no counterpart in the reference) -------
 * Instance matching of two label maps per frame: every predicted object intersected with every truth object, one workgroup per frame,
 * the K x K intersection table and the areas in LDS (K = max_objects).  No floating point and only LDS integer atomics: deterministic,
 * bit for bit.
 *   pred, truth  int32 [n][h][w] (contiguous) as cgs_objects_label writes `labels`: a value <= 0 is background, objects are numbered
 *                from 1.  Hand-made maps are allowed, an object need not be connected.  Objects numbered above K take no part: their
 *                pixels add to no area and no intersection (they still show in pred_max / truth_max); an object <= K keeps its full
 *                area whatever the other map holds under it.
 *   iou_milli    int32 [T] on the device: IoU thresholds in thousandths (the caller keeps them in 500..1000).  The pair (p, t) matches
 *                at m when inter > 0 && 1000 inter >= m (area_p + area_t - inter), compared exactly in int32.
 *   counts       int32 [n][2 + 2 T]: pred_max, truth_max (the largest label of the frame's map, 0 for an empty one), then for each
 *                threshold k the two words matched_pred[k], matched_truth[k] (at 2 + 2 k and 3 + 2 k): the number of p <= K with at
 *                least one matching t <= K, and the same from the truth side.  At 0.5 exactly one object can match two of the other
 *                map, so the two can differ.
 *   best         int32 [n][2][K][4] or NULL.  Side 0, row p - 1: (t, inter, area_p, area_t) of the truth object of largest IoU with p
 *                (exact, by cross-multiplication; ties go to the smallest t), (0, 0, area_p, 0) when p overlaps none.  Side 1, row
 *                t - 1: the same seen from the truth object, (p, inter, area_t, area_p).  Rows from min(max label of that side, K) on
 *                are zero; every row is written.
 * Runs on `stream` without synchronising, allocates nothing, can be captured in a graph.  pred, truth, iou_milli, counts not NULL,
 * n, h, w, max_objects >= 1, 1 <= T <= CGS_OBJ_MATCH_MAX_IOU, every pointer 4-byte aligned, else CGS_ERR_BADARG (nothing is
 * launched); then h, w <= 64 and max_objects <= CGS_OBJ_MATCH_MAX_OBJECTS, else CGS_ERR_UNSUPPORTED.                                   */
enum { CGS_OBJ_MATCH_MAX_OBJECTS = 64, CGS_OBJ_MATCH_MAX_IOU = 16 };
int cgs_objects_match(const int32_t* pred, const int32_t* truth, int32_t n, int32_t h, int32_t w, int32_t max_objects,
                      const int32_t* iou_milli, int32_t T, int32_t* counts, int32_t* best, cgs_stream_t stream);

/* ---- from objects to tracks (csrc/objects_track.hip; this build's own -objects --track-iou, no counterpart in the reference) ------------
 * Objects of one label stack followed from frame to frame.  All integer and deterministic: the only global atomics are integer add /
 * min / max, so every output is bit-reproducible.
 *   labels   int32 [n][h][w] (contiguous) as cgs_objects_label writes it; hand-made maps allowed.  An object of frame f is a label l in
 *            1..K (K = max_objects) with at least one pixel in frame f; labels above K and labels <= 0 take no part.
 *   link     object p of frame f and object q of frame f + 1 are linked at iou_milli = m (1..1000) when q is p's best partner in f + 1,
 *            p is q's best partner in f ("best" is cgs_objects_match's `best`: largest IoU by cross-multiplication, ties to the smallest
 *            number) and inter > 0 && 1000 inter >= m (area_p + area_q - inter) in int32.  Mutual best makes links one-to-one, so
 *            thresholds below 500 are allowed here.
 *   track    a maximal chain of links: consecutive frames, one object per frame.  An object with no link backwards is a head; tracks
 *            are numbered 1..N in the order of their heads, by frame, then by label within the frame.
 *   prev     int32 [n][K]: prev[f][l-1] is the label in frame f - 1 that object l continues; 0 for a head, for f = 0, for no object
 *   track    int32 [n][K]: the object's track number, 0 for a row that is no object (numbers above max_tracks are still handed out)
 *   totals   int32 [4]: tracks N, links, objects, the longest track's length
 *   tracks   int32 [max_tracks][8] or NULL: row t-1 is track t: first_frame, first_label, length, area_sum, area_min, area_max,
 *            inter_sum, union_sum (the last two over the track's links); rows from min(N, max_tracks) on are zero
 *   track_labels  int32 [n][h][w] or NULL: per pixel the track number of the pixel's object, 0 for background and labels above K
 *   rgb      uint8 [n][h][w][3] or NULL: black where track_labels is 0, else with hsh = (uint32) track * 2654435761u channel c is
 *            64 + ((hsh >> 8 c) & 255) * 191 / 255 (integer division): never black
 *   scratch  caller-owned, 8-byte aligned, at least cgs_objects_track_scratch_bytes(n, max_objects) bytes (0 for n or max_objects
 *            < 1); holds nothing between calls
 * The pairs are cgs_objects_match on (labels, labels + h w) with n - 1 frames plus one self-pair of the last frame for its areas; the
 * chains are resolved by pointer doubling, ceil(log2(n - 1)) rounds.  Runs on `stream` without synchronising, allocates nothing, can
 * be captured in a graph; the number of launches depends on n only.  labels, prev, track, totals, scratch not NULL, n, h, w,
 * max_objects, max_tracks >= 1, 1 <= iou_milli <= 1000, int32 pointers 4-byte and scratch 8-byte aligned, scratch_bytes large enough,
 * else CGS_ERR_BADARG (nothing is launched); then h, w <= 64, max_objects <= 64 and n <= CGS_OBJ_TRACK_MAX_FRAMES (which keeps
 * area_sum and union_sum inside int32: 8191 * 2^17 < 2^31), else CGS_ERR_UNSUPPORTED.
 *
 * cgs_objects_track_switches: identity switches of a prediction's tracks against the truth's.  truth_prev int32 [n][K] (`prev` of the
 * truth stack), pred_track int32 [n][K] (`track` of the predicted stack), match_best int32 [n][2][K][4] = cgs_objects_match(pred,
 * truth)'s `best` (its side 1 rows give each truth object's best predicted object), iou_milli int32 [T] on the device, 1 <= T <= 16.
 * counts int32 [T][3], zeroed by the entry itself on the stream, per threshold m: covered = truth objects whose best pair reaches m;
 * continued = truth links q' -> q (frames f - 1, f) with both ends covered; switches = those continued links whose two predicted
 * partners carry different pred_track numbers.  Gaps are NOT bridged: a truth object that is uncovered for a frame ends the
 * comparison there, and the next covered frame starts afresh.  Same K for all three inputs.  NULL or misaligned pointers, T outside
 * 1..16, n or max_objects < 1: CGS_ERR_BADARG; then max_objects > 64 or n > CGS_OBJ_TRACK_MAX_FRAMES: CGS_ERR_UNSUPPORTED.            */
enum { CGS_OBJ_TRACK_FIELDS = 8, CGS_OBJ_TRACK_MAX_FRAMES = 1 << 17 };
int64_t cgs_objects_track_scratch_bytes(int32_t n, int32_t max_objects);
int cgs_objects_track(const int32_t* labels, int32_t n, int32_t h, int32_t w, int32_t max_objects, int32_t iou_milli,
                      int32_t max_tracks, int32_t* prev, int32_t* track, int32_t* totals, int32_t* tracks, int32_t* track_labels,
                      uint8_t* rgb, void* scratch, int64_t scratch_bytes, cgs_stream_t stream);
int cgs_objects_track_switches(const int32_t* truth_prev, const int32_t* pred_track, const int32_t* match_best,
                               const int32_t* iou_milli, int32_t T, int32_t n, int32_t max_objects, int32_t* counts,
                               cgs_stream_t stream);

/* cgs_objects_track_gap: cgs_objects_track that bridges gaps of up to max_gap = G missing frames (0..CGS_OBJ_TRACK_MAX_GAP; 8 is a
 * judgement -- long enough for a hand swinging across an object, short enough that one threshold still means "the same thing" -- not
 * a measured value).  Linking runs in levels g = 1 .. G + 1, all links of a level before any of the next:
 *   level 1     cgs_objects_track's rule and path, unchanged.
 *   level g>=2  for every frame f >= g on its own: the open tails of f - g (objects without a successor from a level < g) against the
 *               open heads of f (objects without a predecessor from a level < g), every other label read as background in both frames;
 *               then the same rule on the two masked frames: best partners among the open objects only, mutual best, inter > 0 &&
 *               1000 inter >= iou_milli union with the inter and union of the two masks g frames apart.  A link closes both ends.
 * So a shorter gap always beats a longer one, and an object that is already taken does not block a bridge (masking comes before the
 * best-partner search).  Within a level frame f touches only the heads of f and the tails of f - g: one launch per level, one
 * workgroup per frame pair, no label stack copied.  A track is a maximal chain of links of any gap, numbered as in cgs_objects_track.
 *   prev       int32 [n][K]: the label in frame f - gap that the object continues, 0 for a head
 *   gap        int32 [n][K]: 0 no link, 1 adjacent, g bridged over g - 1 missing frames
 *   totals     int32 [4]: tracks, links of any gap, objects, the longest span in frames, max(f - first_frame + 1) (without gaps: the
 *              longest length)
 *   gap_links  int32 [max_gap + 1]: the number of links of gap g at index g - 1
 *   tracks     as cgs_objects_track: length counts objects, inter_sum and union_sum run over all links, bridged ones included
 *   tracks_extra  int32 [max_tracks][2] or NULL: bridges (links of gap > 1) and missed (sum of gap - 1); span = length + missed
 *   track, track_labels, rgb  as cgs_objects_track
 *   scratch    8-byte aligned, at least cgs_objects_track_gap_scratch_bytes(n, max_objects, max_gap) bytes (0 for a bad argument)
 * With max_gap = 0 every output shared with cgs_objects_track is bit-identical to it.  8 + R + (n > 1) + min(G, n - 1) launches (a level
 * with no frame pair launches nothing), a function of n and G alone; no synchronisation, nothing allocated, all integer, global atomics
 * add / min / max only.  gap and gap_links not NULL and 4-byte aligned, max_gap in 0..8, else CGS_ERR_BADARG; every other limit and
 * return code is cgs_objects_track's.  For cgs_objects_track_switches pass the truth's prev with the entries of gap != 1 set to 0: it
 * reads prev as "in frame f - 1".                                                                                                      */
enum { CGS_OBJ_TRACK_MAX_GAP = 8 };
int64_t cgs_objects_track_gap_scratch_bytes(int32_t n, int32_t max_objects, int32_t max_gap);
int cgs_objects_track_gap(const int32_t* labels, int32_t n, int32_t h, int32_t w, int32_t max_objects, int32_t iou_milli,
                          int32_t max_gap, int32_t max_tracks, int32_t* prev, int32_t* gap, int32_t* track, int32_t* totals,
                          int32_t* gap_links, int32_t* tracks, int32_t* tracks_extra, int32_t* track_labels, uint8_t* rgb,
                          void* scratch, int64_t scratch_bytes, cgs_stream_t stream);

/* cgs_objects_track_mc: cgs_objects_track_gap with the earlier frame's labels carried along a block motion field before they are
 * intersected, at level 1 and at every gap level.  This comment is the specification.
 *   bwd        int8 [n - 1][8][8][2], components (dy, dx), exactly as cgs_temporal_flow writes its backward field: bwd[g] belongs to
 *              frames g + 1 -> g.  May be NULL only when n == 1 (it is not read then).
 *   path       for a frame pair (a, f), g = f - a >= 1, and a cell q of frame f (cgs_temporal_smooth_mc's path for k < 0): m_0 = (0, 0);
 *              for j = 0 .. g - 1: c = q + m_j with each coordinate clamped into 0..63, m_{j+1} = m_j + bwd[f - j - 1][c.y >> 3][c.x >> 3].
 *   carried    W_{a->f}[q] = L_a[q + m_g] when that cell lies inside the grid, 0 otherwise (L_a: frame a's labels, those outside 1..K
 *              read as 0).  A gather: no cell has two sources, none is undefined.
 *   linking    cgs_objects_track_gap's rule with W_{a->f} where L_a stood.  Level 1: all objects of f - 1 and f, pairs counted over the
 *              cells q as (W[q], L_f[q]), best partner from both sides (largest IoU, ties to the smallest number), mutual best and inter >
 *              0 && 1000 inter >= iou_milli union.  union = carried area + area of the later object - inter, the carried area being the
 *              number of cells of W that hold the label: an object half out of the frame after a pan is compared by the half that is
 *              seen.  Levels g = 2 .. G + 1: the open tails of f - g (carried over g steps) against the open heads of f, every other
 *              label read as 0, level by level.
 *   outputs    prev, gap, track, totals, gap_links, tracks, tracks_extra, track_labels, rgb as cgs_objects_track_gap.  area_sum / area_min
 *              / area_max stay the objects' true areas (counted where the object is); inter_sum / union_sum are those of the links as
 *              decided (with the carried areas).
 *   scratch    cgs_objects_track_mc_scratch_bytes(n, max_objects, max_gap) = cgs_objects_track_gap_scratch_bytes of the same arguments
 * An all-zero field gives cgs_objects_track_gap's outputs bit for bit.  A link (a -> f) depends on the labels of frames a and f and on
 * bwd[a .. f - 1] only.  No read is out of range for any int8 content of bwd or any int32 content of labels (|m| <= 9 * 128); vectors
 * beyond the search range of the flow merely carry further.  Compensated: translation by whole cells, constant over a block of 8 x 8
 * cells.  Not compensated: motion of a fraction of a cell, motion inside a block, occlusion; there is no forward / backward consistency
 * check.  One workgroup per frame pair and level, frame a's labels staged in LDS (a byte per cell); the launches are
 * cgs_objects_track_gap's in number, with the level-1 count in place of cgs_objects_match.  max_gap in 0..8, bwd NULL only when n == 1,
 * and cgs_objects_track_gap's other checks, else CGS_ERR_BADARG; then h == w == 64 (the field is 8 x 8 blocks over 64 x 64 cells),
 * max_objects <= 64, n <= CGS_OBJ_TRACK_MAX_FRAMES, else CGS_ERR_UNSUPPORTED.  A bad argument launches nothing.                        */
int64_t cgs_objects_track_mc_scratch_bytes(int32_t n, int32_t max_objects, int32_t max_gap);
int cgs_objects_track_mc(const int32_t* labels, const int8_t* bwd, int32_t n, int32_t h, int32_t w, int32_t max_objects,
                         int32_t iou_milli, int32_t max_gap, int32_t max_tracks, int32_t* prev, int32_t* gap, int32_t* track,
                         int32_t* totals, int32_t* gap_links, int32_t* tracks, int32_t* tracks_extra, int32_t* track_labels, uint8_t* rgb,
                         void* scratch, int64_t scratch_bytes, cgs_stream_t stream);

/* cgs_objects_track_fill (csrc/objects_fill.hip): the masks that the bridged links of cgs_objects_track_gap / cgs_objects_track_mc jump
 * over.  For every frame m between the two ends of a link of gap >= 2 the link's tail object is carried from its frame to m along the
 * backward vectors the link was decided on, and where it lands on cells without an object it becomes a new object of frame m.  This
 * comment is the specification.
 *   labels     int32 [n][h][w], the stack that was tracked.  bwd int8 [n - 1][8][8][2], the field it was tracked along, or NULL: the
 *              all-zero field (then h, w <= 64; with a field h == w == 64).  K = max_objects <= 64, G = max_gap in 1..8.
 *   prev, gap, track  int32 [n][K] as cgs_objects_track_gap / _mc wrote them for these labels with the same K and a max_gap <= G.  Any
 *              int32 content is allowed: an entry outside the ranges below names nothing.
 *   rule, for frame m and j = 1 .. min(G, m), a = m - j:
 *     spanning   S(m, j) = the labels p in 1..K for which some f in m + 1 .. min(n - 1, a + G + 1) and l in 1..K have
 *                gap[f][l-1] == f - a and prev[f][l-1] == p: the tails in frame a of links that jump over m.
 *     carried    W_{a->m} is cgs_objects_track_mc's carried map with (a, m) for (a, f): labels outside 1..K read as 0, 0 outside the
 *                grid; with bwd NULL it is frame a's labels (those outside 1..K read as 0).  The walk for j + 1 extends the walk for j.
 *     claim      a cell q with labels[m][q] <= 0 is claimed by the smallest j with W_{m-j->m}[q] in S(m, j), for the candidate (j, p), p
 *                that label.  A cell with a positive label is never touched (labels above K block too).  Pure selection per cell.
 *     numbering  base = the largest value of labels[m], at least 0.  The candidates that claimed a cell, ordered by (j, p) ascending,
 *                get the labels base + 1, base + 2, ...; those above K are dropped and their cells stay as they were.
 *   out_labels int32 [n][h][w]: the input value where nothing was written, else the new label.  Must not be `labels`.
 *   out_track  int32 [n][K]: row l-1 is track[m][l-1] when l in 1..K holds a cell of labels[m], track[a][p-1] for a new object, else 0
 *   age        int32 [n][K]: j for a new label, 0 everywhere else
 *   table      int32 [n][K][CGS_OBJ_FIELDS] or NULL: cgs_objects_label's row (area, x0, y0, x1, y1, sum_x, sum_y, first) of every new
 *              object; all other rows are zero
 *   totals     int32 [4], zeroed by the entry on the stream: new objects, their cells, dropped candidates, vanished candidates (in some
 *              S(m, j) but without a claimed cell: carried out of the grid or fully covered)
 * One launch, one workgroup per frame; a frame that no link jumps over is copied.  The frames m - 1 .. m - G are staged as bytes in
 * LDS; no scratch.  All integer; the only global atomics are the integer adds of totals: bit-reproducible.  The inputs are not written.
 * No read or write is out of range for any int32 content of labels, prev, gap, track or any int8 content of bwd.  Runs on `stream`
 * without synchronising, allocates nothing, can be captured in a graph.  Limits of the rule: the mask comes from the tail alone (the
 * head's mask and the forward field are not used), motion is whole-cell block motion, real pixels always win, a frame has K labels.
 * labels, prev, gap, track, out_labels, out_track, age, totals not NULL, n, h, w, max_objects >= 1, max_gap in 1..8, int32 pointers
 * 4-byte aligned, out_labels != labels, else CGS_ERR_BADARG (nothing is launched); then the sizes above, max_objects <= 64 and n <=
 * CGS_OBJ_TRACK_MAX_FRAMES, else CGS_ERR_UNSUPPORTED.                                                                                  */
int cgs_objects_track_fill(const int32_t* labels, const int8_t* bwd, int32_t n, int32_t h, int32_t w, int32_t max_objects,
                           int32_t max_gap, const int32_t* prev, const int32_t* gap, const int32_t* track, int32_t* out_labels,
                           int32_t* out_track, int32_t* age, int32_t* table, int32_t* totals, cgs_stream_t stream);

/* cgs_objects_track_fill_window (csrc/objects_fill.hip): cgs_objects_track_fill for the frames f0 <= m < f1 of a window of n frames, what
 * a stream needs whose window carries halo frames on both sides (cgs_temporal_smooth takes f0, f1 for the same reason).
 *   labels, bwd, n, h, w, max_objects, max_gap, prev, gap, track   as cgs_objects_track_fill: the WHOLE window of n frames
 *   f0, f1     0 <= f0 <= f1 <= n.  Only the frames f0 <= m < f1 get a workgroup.
 *   out_labels int32 [f1 - f0][h][w], out_track, age int32 [f1 - f0][K], table int32 [f1 - f0][K][CGS_OBJ_FIELDS] or NULL: frame m's
 *              outputs of cgs_objects_track_fill at index m - f0
 *   totals     int32 [4], zeroed by the entry on the stream: the four sums over the frames f0 <= m < f1 only
 * Frame m reads the labels of m - G .. m - 1 (and the vectors between them) and the prev / gap rows of m + 1 .. m + G, clipped to
 * 0 .. n - 1, exactly as the whole-stack entry does: f0 = 0, f1 = n gives its outputs bit for bit.  f0 == f1 launches nothing and
 * zeroes totals.  A stream needs the sub-range because dropped / vanished exist only in totals, and a window's totals would include
 * halo frames whose contribution is not final.  The bounded-read guarantees, the argument checks and the limits are those of
 * cgs_objects_track_fill; besides them 0 <= f0 <= f1 <= n, else CGS_ERR_BADARG (nothing is launched).                               */
int cgs_objects_track_fill_window(const int32_t* labels, const int8_t* bwd, int32_t n, int32_t h, int32_t w, int32_t max_objects,
                                  int32_t max_gap, const int32_t* prev, const int32_t* gap, const int32_t* track, int32_t f0, int32_t f1,
                                  int32_t* out_labels, int32_t* out_track, int32_t* age, int32_t* table, int32_t* totals,
                                  cgs_stream_t stream);

/* cgs_objects_appearance, cgs_objects_reid (csrc/objects_reid.hip): an identity layer on top of the tracks.  Tracks that do not overlap
 * in time, lie at most W frames apart and have the same colour histogram are chained into one identity; the tracks themselves, their
 * links and their numbers are not touched.  This comment is the specification.
 *   frames     uint8 [n][h][w][3], the frames the labels were made from; labels int32 [n][h][w]; track int32 [n][K] as cgs_objects_track*
 *              wrote it; tracks int32 [max_tracks][8] and tracks_extra int32 [max_tracks][2] (NULL for a tracker result without gaps);
 *              n_tracks: the tracker's totals[0], read ON THE DEVICE, used as min(max(n_tracks, 0), max_tracks) = N.
 *              1 <= h, w <= 64, K = max_objects <= 64.
 *   bin        a pixel's bin is ((R >> 6) << 4) | ((G >> 6) << 2) | (B >> 6): 64 bins, four levels a channel.  (64 is one lane per bin
 *              of a wave: a judgement, not a tuned value.)
 *   H          object histogram: H[f][l-1][b] = the pixels of frame f with label l in 1..K and bin b.  Labels outside 1..K count nowhere.
 *   S          track histogram: S[t-1][b] = the sum of H[f][l-1][b] over all (f, l) with track[f][l-1] == t, int32; a track number
 *              outside 1..max_tracks counts nowhere.  The track's pixel count is A_t = sum_b S[t-1][b] -- defined from S, not taken from
 *              the table's area_sum, so it does not depend on which tracker entry made the table.
 *   signature  track t is eligible when A_t >= min_area.  Then Q[t-1][b] = floor(S[t-1][b] * 4096 / A_t), computed in 64 bits, stored as
 *              int16, and D_t = sum_b Q[t-1][b], which lies in 4033..4096.  For an ineligible t, Q is all zero and D_t = 0.
 *   time       F_t = the table's first_frame; L_t = F_t + length + missed - 1 with missed from tracks_extra, 0 without it.  (t -> u) is
 *              a candidate pair when both are eligible and L_t < F_u <= L_t + W.  Tracks are numbered by first frame, then label, so the
 *              u of one t are a contiguous range of track numbers, all above t.
 *   similarity s(t, u) = sum_b min(Q_t[b], Q_u[b]).  A candidate pair is admissible when 1000 s >= sim_milli min(D_t, D_u), in
 *              integers: identical histograms score 1.0.
 *   links      succ[t] = the admissible u of largest s, ties to the smallest u; pred[u] = the admissible t of largest s, ties to the
 *              smallest t.  t -> u is a link when succ[t] == u and pred[u] == t.  Links are one to one and run forward in time, so
 *              chains are acyclic and their members do not overlap in time.
 *   identity   a maximal chain of links; identities are numbered from 1 in the order of their first track's number.  A track without a
 *              link is an identity of its own, ineligible tracks included.
 * cgs_objects_appearance: one launch, one workgroup per frame.
 *   track_hist   int32 [max_tracks][64] = S, zeroed by the entry on the stream, or NULL together with track: only H is made then
 *   object_hist  int32 [n][K][64] = H, or NULL: not written
 * frames, labels not NULL, track and track_hist both NULL or both not, at least one output, n, h, w, max_objects >= 1, max_tracks >= 1
 * with track, int32 pointers 4-byte aligned, else CGS_ERR_BADARG (nothing is launched); then h, w <= 64, max_objects <= 64 and n <=
 * CGS_OBJ_REID_MAX_FRAMES (S and Q have n K rows for a full table: the tracker's 2^17 frames would need gigabytes), else
 * CGS_ERR_UNSUPPORTED.  Integer sums in LDS and int32 global atomic adds: bit-reproducible.
 * cgs_objects_reid: n is the number of frames of the stack (first_frame < n), W = window, every output indexed by t - 1.
 *   reid_prev, reid_next  int32 [max_tracks]: the track linked before / behind t, 0 for none
 *   reid_sim   int32 [max_tracks]: the s of the link to reid_prev, else 0
 *   identity   int32 [max_tracks]
 *   signature  int16 [max_tracks][64] = Q, 16-byte aligned
 *   totals     int32 [4]: identities, links, eligible tracks, the most tracks in one identity (0 for N = 0)
 *   The five arrays are zero from row N on.
 *   scratch    caller-owned, 8-byte aligned, at least cgs_objects_reid_scratch_bytes(n, max_tracks) bytes (0 for n or max_tracks < 1);
 *              holds nothing between calls
 * Runs on `stream` without synchronising, allocates nothing; 7 + R launches and memsets, R = ceil(log2(min(n, max_tracks) - 1)) rounds
 * of pointer doubling (a chain has at most n members), a function of n and max_tracks alone.  All integer; global atomics are int32 add
 * / max and one unsigned 64-bit max: bit-reproducible.  No read or write is out of range for any int32 content of track_hist, tracks,
 * tracks_extra or n_tracks (the candidate range comes from a search that is bounded whatever the first column holds, every pair is
 * checked against the rule itself, and a link is only taken towards a larger number); the outputs are the rule's when the first column
 * is non-decreasing over the first N rows, as every tracker entry writes it.  max_tracks >= n K is not required: a truncated
 * table re-identifies the tracks it holds.  Pointers other than tracks_extra not NULL and aligned, n, max_tracks >= 1, sim_milli in
 * 1..1000, window in 1..CGS_OBJ_REID_MAX_WINDOW, min_area >= 1, scratch_bytes large enough, else CGS_ERR_BADARG (nothing is launched);
 * then n <= CGS_OBJ_REID_MAX_FRAMES, else CGS_ERR_UNSUPPORTED.                                                                          */
enum { CGS_OBJ_REID_BINS = 64, CGS_OBJ_REID_MAX_WINDOW = 1024, CGS_OBJ_REID_MAX_FRAMES = 1 << 14 };
int cgs_objects_appearance(const uint8_t* frames, const int32_t* labels, const int32_t* track, int32_t n, int32_t h, int32_t w,
                           int32_t max_objects, int32_t max_tracks, int32_t* track_hist, int32_t* object_hist, cgs_stream_t stream);
int64_t cgs_objects_reid_scratch_bytes(int32_t n, int32_t max_tracks);
int cgs_objects_reid(const int32_t* track_hist, const int32_t* tracks, const int32_t* tracks_extra, const int32_t* n_tracks, int32_t n,
                     int32_t max_tracks, int32_t sim_milli, int32_t window, int32_t min_area, int32_t* reid_prev, int32_t* reid_next,
                     int32_t* reid_sim, int32_t* identity, int32_t* totals, int16_t* signature, void* scratch, int64_t scratch_bytes,
                     cgs_stream_t stream);

/* cgs_objects_ablate, cgs_objects_select (csrc/objects_value.hip): the value of an object, -objects --object-value.  The critic is asked
 * once per object how far its value of the frame falls when that object alone is replaced -- the training rule's A (1 - Z) + Z B with a
 * hard Z -- and the objects that fail a threshold are dropped and the rest renumbered.  This comment is the specification.
 *   frames     uint8 [n][64][64][3]; labels int32 [n][64][64] as cgs_objects_label wrote them; K = max_objects <= 64.
 *   rows       offsets int32 [n + 1], non-decreasing from 0: frame f owns the rows offsets[f] .. offsets[f + 1] - 1 of the whole stack,
 *              row offsets[f] + k - 1 is its object k, k = 1 .. min(offsets[f + 1] - offsets[f], K).  (The caller makes it as the
 *              exclusive prefix sum of min(kept[f], K).)
 *   ablated    R = grow in 0..4.  A_k is the set of cells (y, x) for which some cell (y', x') inside the frame has |y - y'| <= R,
 *              |x - x'| <= R and labels[f][y'][x'] == k: cells of other objects within R of object k are replaced too; a label above K
 *              matches no k.
 *   row        out[y][x][:] = F_f[y][x][:] on A_k and frames[f][y][x][:] elsewhere.
 *   fill       fill_mode 0: F_f is the constant colour fill_rgb = R | G << 8 | B << 16.  1: F_f = the uint8 [64][64][3] frame at fill + f
 *              fill_stride, fill_stride 0 (one frame for all rows) or 12288.  2: F_f is the constant colour c_ch = (2 S_ch + N) / (2 N)
 *              in integer division, S_ch and N the channel sum and the count over the cells of frame f whose label is 0 (any other
 *              label, those above K included, is not background), and over all 4096 cells when there are none.
 * cgs_objects_ablate: the rows of the frames f0 <= f < f1, one launch, one workgroup per frame.
 *   out        uint8 [rows][64][64][3], row_frame, row_label int32 [rows], rows = offsets[f1] - offsets[f0]: row r of the range is row
 *              offsets[f0] + r of the stack; row_frame holds f, row_label k.  A row index outside 0 .. rows - 1 (offsets that do not
 *              fit) is not written, and no read is out of range for any content of labels or offsets.  All offsets are 64-bit.
 * frames, labels, offsets and the outputs not NULL, frames, fill and out 16-byte aligned, int32 pointers 4-byte aligned, n >= 1, 0 <= f0 <
 * f1 <= n, rows >= 1 (an empty range or a range without rows is the caller's to skip: nothing is ever launched with an empty grid),
 * max_objects >= 1, grow >= 0, fill_mode in 0..2, fill given exactly with mode 1, fill_rgb < 2^24, else CGS_ERR_BADARG (nothing is
 * launched); then max_objects <= 64 and grow <= 4, else CGS_ERR_UNSUPPORTED.  Integer and selection only: bit-reproducible.
 * cgs_objects_select: table int32 [n][K][8] (cgs_objects_label's rows), kept int32 [n], keep uint8 [n][K]; frames of h x w <= 64 x 64.
 *   Old label k becomes 1 + #{j < k : keep[f][j - 1] != 0} when k <= min(kept[f], K) and keep[f][k - 1] != 0, and 0 otherwise -- every
 *   label above K included: an object that was never scored is dropped.  The order is kept, so the new numbers are still the raster
 *   order of the first pixel.
 *   out_labels int32 [n][h][w]; out_table int32 [n][K][8]: the kept rows in order, zero rows behind them; out_kept int32 [n];
 *   mask uint8 [n][h][w] = out_labels != 0; unscored int32 [n] = max(kept[f] - K, 0), the objects numbered above K that were dropped.
 * One launch, one workgroup per frame.  Pointers not NULL and aligned, n, h, w, max_objects >= 1, else CGS_ERR_BADARG; then h, w <= 64
 * and max_objects <= 64, else CGS_ERR_UNSUPPORTED.                                                                                       */
enum { CGS_OBJ_VALUE_MAX_OBJECTS = 64, CGS_OBJ_VALUE_MAX_GROW = 4 };
int cgs_objects_ablate(const uint8_t* frames, const int32_t* labels, const int32_t* offsets, int32_t n, int32_t f0, int32_t f1,
                       int32_t max_objects, int32_t grow, int32_t fill_mode, uint32_t fill_rgb, const uint8_t* fill, int64_t fill_stride,
                       int64_t rows, uint8_t* out, int32_t* row_frame, int32_t* row_label, cgs_stream_t stream);
int cgs_objects_select(const int32_t* labels, const int32_t* table, const int32_t* kept, const uint8_t* keep, int32_t n, int32_t h,
                       int32_t w, int32_t max_objects, int32_t* out_labels, int32_t* out_table, int32_t* out_kept, uint8_t* mask,
                       int32_t* unscored, cgs_stream_t stream);

/* ---- the saliency baseline over a threshold grid (csrc/saliency.hip; Handler._saliency_post, main.py:976-1003; this build's own
 * -eval -salience --salience-grid) -----------------------------------------------------------------------------------------------------
 * The baseline's whole post-processing for T thresholds at once, each threshold with its own normaliser as the host form has it.  A
 * pixel of frame f is on at thr[t] when, in float64 with IEEE division and multiplication (no contraction, no fast-math),
 *     min((double) sal / ((double) S + DBL_MIN) * (double) preds[f], 1.0) > thr[t]
 * which numpy 2 evaluates for Handler._saliency_post; the on/off decision, and so every count, is that form's bit for bit.
 *   sal     fp32 [n][64][64]: non-negative or NaN (-0.0 counts as 0); a NaN pixel is on for nothing
 *   preds   fp32 [n]; a frame with preds <= 0 or NaN is on for nothing
 *   truth   uint8 [n][64][64] (non-zero = set) or NULL: then counts is not written
 *   thr     fp64 [T] in DEVICE memory, any order, > 0 (a threshold >= 1 switches everything off; one <= 0 gives unspecified counts)
 *   gscale  fp32 [T] in device memory or NULL.  Not NULL: global mode, S = gscale[t] for every frame (the caller builds
 *           float32(mean * float32(t))).  NULL: per-frame mode, S = the frame's k[t]-th smallest value with NaN sorted last (np.sort)
 *   k       int32 [T] in device memory, read in per-frame mode only, 0..4095 (clamped to that range)
 *   which   index of the threshold whose mask goes to `hard`, or -1 for none
 *   counts  int64 [T][2], zeroed by the entry itself on the stream: (#{truth and on_t}, #{truth or on_t}) over the stack, in the
 *           caller's threshold order; the frames add to it with integer atomics, so the result does not depend on their order
 *   scale   fp32 [n][T]: the S used for each frame and threshold (a NaN comes back as the quiet NaN)
 *   hard    uint8 [n][64][64], 0 / 1, or NULL when which is -1
 * One workgroup per frame: its 4096 values sorted once in LDS with the truth bit riding along, a prefix count of the truth in sorted
 * order, and per threshold a binary search over the sorted positions that evaluates the predicate above at every probe (for preds > 0
 * it is monotone in sal).  Runs on `stream` without synchronising, allocates nothing, can be captured in a graph.
 * 1 <= T <= 1024, n >= 1, h, w >= 1, -1 <= which < T, the pointers above not NULL, fp32 / int32 / hard 4-byte and thr / counts 8-byte
 * aligned, else CGS_ERR_BADARG; then h = w = 64, else CGS_ERR_UNSUPPORTED.  The checks come before anything is launched.              */
int cgs_saliency_sweep(const float* sal, const float* preds, const uint8_t* truth, const double* thr, const float* gscale,
                       const int32_t* k, int32_t T, int32_t n, int32_t h, int32_t w, int32_t which, int64_t* counts, float* scale,
                       uint8_t* hard, cgs_stream_t stream);

/* ---- boundary F and boundary IoU (csrc/boundary.hip; this build's own -eval --boundary-tol, no counterpart in the reference) ---------------
 * How well a mask's outline follows the truth's: per frame the two boundaries, the exact squared Euclidean distance from every pixel to
 * each, and the counts of the boundary F-measure, of boundary IoU (Cheng et al.) and of the Hausdorff distance.  One workgroup per
 * frame in LDS, integer throughout, no atomics: deterministic, bit for bit.
 *   pred      [n][h][w] (contiguous); pred_kind and thresh say when a pixel is on, exactly as cgs_objects_label's src_kind: CGS_OBJ_U8
 *             (a bool stack is this), CGS_OBJ_F32_GT, CGS_OBJ_F32_GE; compared in fp32, a NaN is off
 *   truth     uint8 [n][h][w], non-zero = on
 *   boundary  a pixel is a boundary pixel of a mask when it is on and at least one of its four neighbours is off; everything outside
 *             the frame is off, so a mask cut by the frame edge has its boundary there (the inner boundary of the boundary-IoU code,
 *             not a half-pixel map)
 *   tol2      int32 [T] in DEVICE memory: squared tolerances q, any order; a pixel is within tolerance when d2 <= q.  Values above
 *             2 x 63^2 act as "any distance", negative ones as "none"
 *   counts    int32 [n][4 + 4 T]: pred_px, truth_px (boundary pixels), hd2_pred (the largest squared distance from a predicted boundary
 *             pixel to the truth boundary), hd2_truth (the other way round; both -1 when either boundary is empty), then per tolerance
 *             k at 4 + 4 k: hit_pred (predicted boundary pixels with d2_truth <= q), hit_truth, band_inter = #(P_q & G_q), band_union =
 *             #(P_q | G_q) with P_q the on pixels of pred with d2_pred <= q and G_q the same for the truth.  An empty boundary gives
 *             that side's band as empty and the other side no hits
 *   dist2     int32 [n][2][h][w] or NULL: the squared distance of every pixel to the predicted (plane 0) and the truth boundary
 *             (plane 1); -1 throughout a plane whose boundary is empty
 * Runs on `stream` without synchronising, allocates nothing, can be captured in a graph.  pred, truth, tol2, counts not NULL, n, h, w
 * >= 1, a valid pred_kind, 1 <= T <= CGS_BOUNDARY_MAX_TOL, fp32 pred / tol2 / counts / dist2 4-byte aligned, else CGS_ERR_BADARG
 * (nothing is launched); then h, w <= 64, else CGS_ERR_UNSUPPORTED.                                                                    */
enum { CGS_BOUNDARY_MAX_TOL = 16, CGS_BOUNDARY_MAX_TOL_PX = 128 };
int cgs_boundary_score(const void* pred, int32_t pred_kind, float thresh, const uint8_t* truth, int32_t n, int32_t h, int32_t w,
                       const int32_t* tol2, int32_t T, int32_t* counts, int32_t* dist2, cgs_stream_t stream);

/* ---- frames of any size: the way in and the way out (csrc/fit.hip; this build's own -process -fit) ------------------------------------------
 * The reference's loader stacks the files of a folder and so demands one size, which its network fixes at 64 x 64 (main.py:1126-1127);
 * its writer saves every column at the network's size (main.py:1212-1223).  These two entries stand beside those lines: the first shrinks
 * uint8 frames of any size from 64 to CGS_FIT_MAX_SIDE pixels a side to the network's grid, the second brings a 64 x 64 map back to the
 * frame's size along the frame's own edges.  Both run on `stream` without synchronising, allocate nothing, use no atomics, are
 * deterministic and can be captured in a graph.
 *
 * cgs_fit_down_u8: the exact box average, in integers (a stretch, not a letterbox).
 *   frames  uint8 [n][h][w][3]
 *   out     uint8 [n][64][64][3]
 * On an axis of length L source pixel s covers [64 s, 64 s + 64), output cell o covers [L o, L o + L) and w_L(o, s) is the length of their
 * overlap (0..64; it sums to L over s).  Per channel S = sum_y sum_x w_h(oy, y) w_w(ox, x) v[y][x] and out = (2 S + h w) / (2 h w) in
 * integer division: the box average rounded half up.  For h and w multiples of 64 that is the plain block mean, at h = w = 64 a copy.
 * The rows are read with 16-, 4- or 1-byte loads: the widest for which `frames` and 3 w are both aligned.
 * frames, out not NULL, n, h, w >= 1, else CGS_ERR_BADARG; then 64 <= h, w <= CGS_FIT_MAX_SIDE, else CGS_ERR_UNSUPPORTED.
 *
 * cgs_fit_up_joint: joint bilateral upsampling (Kopf et al. 2007) of a 64 x 64 map to h x w, guided by the frame.
 *   map       [n][64][64]: fp32 (map_kind CGS_FIT_MAP_F32, values in [0, 1]) or uint8 labels (CGS_FIT_MAP_U8: non-zero = 1.0)
 *   guide     uint8 [n][h][w][3]: the frames
 *   low       uint8 [n][64][64][3]: cgs_fit_down_u8 of `guide`
 *   sigma_s   in cells, >= 0.5; sigma_r in colour units of 0..255, > 0
 *   soft      fp32 [n][h][w] or NULL
 *   grey      uint8 [n][h][w] or NULL: (uint8) (soft * 255.0f), the fp32 product truncated
 *   hard      uint8 [n][h][w] or NULL, 0 / 1: soft >= thresh, or soft > thresh when `inclusive` is 0, compared in fp32
 * Pixel (y, x) has the home cell qy0 = ((2 y + 1) 32) / h, qx0 = ((2 x + 1) 32) / w and the taps (qy0 + dy, qx0 + dx), dy, dx in
 * -CGS_FIT_RADIUS .. CGS_FIT_RADIUS, that lie inside the grid; taps outside it are skipped, not clamped.  With fy = ((2 y + 1) 64 -
 * h (2 qy + 1)) / (2 h), fx likewise, ds = fy^2 + fx^2, d2 = |guide[y][x] - low[qy][qx]|^2 (an integer) and d2_min the smallest d2 over
 * the pixel's taps,  w = exp(-(ds / (2 sigma_s^2) + (d2 - d2_min) / (2 sigma_r^2)))  and  soft = sum w m / sum w,  both sums in fp32 in
 * the same tap order.  The difference d2 - d2_min is taken in integers, so no exponent is rounded before it; the tap of d2_min keeps a
 * weight of at least exp(-6.25 / sigma_s^2), so the denominator is never zero.  0 <= soft <= 1 for a map in [0, 1].
 * map, guide, low not NULL, 1 <= n <= 65535, h, w >= 1, a valid map_kind, sigma_s >= 0.5 and sigma_r > 0 and both finite, thresh not a NaN
 * when hard is given, fp32 map / soft 4-byte aligned, else CGS_ERR_BADARG (nothing is launched); then 64 <= h, w <= CGS_FIT_MAX_SIDE,
 * else CGS_ERR_UNSUPPORTED.  With all three outputs NULL nothing is launched.                                                            */
enum { CGS_FIT_SIDE = 64, CGS_FIT_MAX_SIDE = 4096, CGS_FIT_RADIUS = 2, CGS_FIT_MAP_F32 = 0, CGS_FIT_MAP_U8 = 1 };
int cgs_fit_down_u8(const uint8_t* frames, int32_t n, int32_t h, int32_t w, uint8_t* out, cgs_stream_t stream);
int cgs_fit_up_joint(const void* map, int32_t map_kind, const uint8_t* guide, const uint8_t* low, int32_t n, int32_t h, int32_t w,
                     float sigma_s, float sigma_r, float thresh, int32_t inclusive, float* soft, uint8_t* grey, uint8_t* hard,
                     cgs_stream_t stream);

/* ---- a video as the source: masks smoothed along time, the overlay composed (csrc/temporal.hip, csrc/overlay.hip; this build's own
 * -process --source-video) ---------------------------------------------------------------------------------------------------------------
 * The reference reads a folder of stills and writes a PNG per column (main.py:1126-1127, 1212-1223); it has no notion of frame order.
 * These two entries stand beside cgs_fit_*: the first filters the 64 x 64 masks of consecutive frames along time, the second draws a mask
 * on its frame at the frame's own size.  Both run on `stream` without synchronising, allocate nothing, use no atomics, are deterministic
 * and can be captured in a graph.
 *
 * cgs_temporal_smooth: spatio-temporal joint bilateral smoothing of a stack of masks, guided by the shrunk frames.
 *   z       fp32 [n][64][64], values in [0, 1]
 *   low     uint8 [n][64][64][3]: cgs_fit_down_u8 of the frames
 *   out     fp32 [f1 - f0][64][64]: frames f0 <= f < f1 of the smoothed stack
 *   radius  frames each way, 1 .. CGS_TEMPORAL_MAX_RADIUS; sigma_t = radius / 2 (the window is +-2 sigma); sigma_r in colour units, > 0
 * For frame f and cell p the taps are, IN THIS ORDER (the order of both fp32 sums): the centre tap (f, p), weight exactly 1; then k = -radius
 * .. -1, 1 .. radius ascending, and for each k with 0 <= g = f + k < n, dy = -1, 0, 1 (outer) and dx = -1, 0, 1 (inner), the cell p + (dy,
 * dx) of frame g when it lies inside the grid.  A frame outside [0, n) and a cell outside the grid are skipped, not clamped.
 *   w = exp(-(k^2 / (2 sigma_t^2) + (dy^2 + dx^2) / 2 + d2 / (2 sigma_r^2))),  d2 = |low[g][p + (dy, dx)] - low[f][p]|^2 (an integer),
 *   num = fma(w, z[g][p + (dy, dx)], num),  den = den + w,  out = num / den (the IEEE division).
 * The spatial sigma is one cell; one hardware exp2 per tap with the constants folded to base 2.  den >= 1, 0 <= out <= 1, and a stack that
 * is 1.0 wherever a weight is non-zero gives exactly 1.0f.  Motion is not compensated.  The sub-range lets a caller that works in chunks
 * hand over a window (the tail of the chunk before, the chunk, the head of the next) and receive the chunk's frames: with `radius` frames
 * of halo on each side (or the stack's end) the result equals the one-call result bit for bit.
 * z, low, out not NULL, n >= 1, 0 <= f0 < f1 <= n, radius >= 1, sigma_r > 0 and finite, z / out 4-byte aligned, else CGS_ERR_BADARG
 * (nothing is launched); then radius <= CGS_TEMPORAL_MAX_RADIUS, else CGS_ERR_UNSUPPORTED.
 *
 * cgs_overlay_compose: the frames of the overlay video, in integers.
 *   guide     uint8 [n][h][w][3]: the frames
 *   grey      uint8 [n][h][w]: the grey byte of cgs_fit_up_joint
 *   hard      uint8 [n][h][w], zero / non-zero, or NULL: the thresholded mask, for the outline
 *   r, g, b   the tint colour, 0..255 each; alpha256 0..256; thickness 0..CGS_OVERLAY_MAX_OUTLINE
 *   layout    the number of panels k: CGS_OVERLAY_ONLY (overlay), CGS_OVERLAY_SIDE (frame | overlay), CGS_OVERLAY_TRIPLE (frame | overlay |
 *             grey as RGB)
 *   flags     CGS_OVERLAY_NONTEMPORAL = non-temporal stores
 *   out       uint8 [n][h][k w][3]
 * Overlay panel: q = alpha256 grey, out_c = (frame_c (65280 - q) + tint_c q + 32640) / 65280 in integer division.  Outline: E_0 = hard,
 * E_{i+1}[p] = E_i[p] and the E_i of its four neighbours, a neighbour OUTSIDE the frame counting as on; pixel p is on the outline when
 * hard[p] and not E_thickness[p] -- the on pixels within Manhattan distance thickness - 1 of an off pixel -- and is then the tint colour,
 * opaque.  Because the frame's edge counts as on, a mask cut by the frame draws no line along the frame's edge: the opposite of
 * cgs_boundary_score's convention, on purpose (there the edge of the frame is part of an object's outline, here it is not drawn).
 * With hard NULL or thickness 0 there is no outline.  Rows are read and written 16, 4 or 1 bytes at a time: the widest for which guide,
 * grey, out and w are all aligned.
 * guide, grey, out not NULL, 1 <= n <= 65535, h, w >= 1, colour, alpha256, thickness, layout in range, no unknown flag, else CGS_ERR_BADARG
 * (nothing is launched); then 64 <= h, w <= CGS_FIT_MAX_SIDE, else CGS_ERR_UNSUPPORTED.                                                  */
enum { CGS_TEMPORAL_SIDE = 64, CGS_TEMPORAL_MAX_RADIUS = 8 };
enum { CGS_OVERLAY_ONLY = 1, CGS_OVERLAY_SIDE = 2, CGS_OVERLAY_TRIPLE = 3, CGS_OVERLAY_MAX_OUTLINE = 4, CGS_OVERLAY_NONTEMPORAL = 1 };
int cgs_temporal_smooth(const float* z, const uint8_t* low, int32_t n, int32_t f0, int32_t f1, int32_t radius, float sigma_r, float* out,
                        cgs_stream_t stream);
int cgs_overlay_compose(const uint8_t* guide, const uint8_t* grey, const uint8_t* hard, int32_t n, int32_t h, int32_t w, int32_t r,
                        int32_t g, int32_t b, int32_t alpha256, int32_t thickness, int32_t layout, int32_t flags, uint8_t* out,
                        cgs_stream_t stream);

/* ---- tracked objects on the overlay video (csrc/overlay_tracks.hip; -process --source-video --overlay-tracks T) ---------------------------
 * cgs_overlay_compose_tracks: cgs_overlay_compose with a colour per tracked object in place of the one tint, and every object's bounding
 * box and track number drawn on the overlay panel.  Integers throughout, no atomics, deterministic; the frame panel ("side", "triple")
 * and the grey panel are exactly cgs_overlay_compose's.
 *   guide, grey, hard, n, h, w, r, g, b, alpha256, thickness, layout, flags, out   as cgs_overlay_compose; (r, g, b) is the colour of a
 *             pixel without an object
 *   labels    int32 [n][64][64]: cgs_objects_label's labels of the 64 x 64 masks (a value <= 0 is background)
 *   ids       int32 [n][K]: the track number of object l = 1..K of a frame at [l - 1], a value <= 0 meaning none (K = max_objects)
 *   table     int32 [n][K][CGS_OBJ_FIELDS]: cgs_objects_label's table; only area, x0, y0, x1, y1 are read.  A row with area <= 0, or with
 *             a box that is not 0 <= x0 <= x1 <= 63, 0 <= y0 <= y1 <= 63, is no object
 *   font      uint8 [CGS_OVERLAY_FONT_GLYPHS][CGS_OVERLAY_FONT_ROWS]: the digits 0..9, one byte per glyph row, top row first, bit 4 the
 *             leftmost of 5 pixels; read from this pointer, the library holds no digit shapes of its own
 *   boxes     B, the thickness of a box's border, 0..CGS_OVERLAY_MAX_BOXES pixels; 0: no boxes and no numbers
 * Colour of track t >= 1: c_k = 64 + (((t * 2654435761) mod 2^32) >> 8 k & 255) * 191 / 255 for k = 0, 1, 2 (r, g, b) -- the rgb of
 * cgs_objects_track.  Object of pixel (y, x): with (cy, cx) its home cell, ((2 p + 1) 32) / L on an axis of length L, the label
 * labels[cy][cx] when that is in 1..K; when it is above K the pixel has no object; when it is <= 0, the label in 1..K among the cells
 * (c'y, c'x) of the 5 x 5 window around the home cell (CGS_FIT_RADIUS), inside the grid, that minimises in 64 bits
 *   dxn^2 h^2 + dyn^2 w^2,  dxn = (2 x + 1) 64 - (2 c'x + 1) w,  dyn = (2 y + 1) 64 - (2 c'y + 1) h
 * (the squared distance of the pixel's centre and the cell's in cells, over a common denominator), ties to the first in raster order, and
 * no object when the window holds none.  The pixel's colour is that of track ids[f][l - 1] of its object l, (r, g, b) without an object or
 * a track; tint and outline are cgs_overlay_compose's formulas with this colour.
 * Box and number of object l (area > 0, ids[f][l - 1] = t > 0), only with B > 0: cell c of an axis of length L holds the pixels
 * (c L + 31) / 64 .. ((c + 1) L + 31) / 64 - 1 (those whose home cell it is); the rectangle runs from the first pixel of cell x0 to the last
 * of x1, and so in y.  Border: the pixels of the rectangle fewer than B pixels from one of its four sides, colour(t), opaque.  Plate: with
 * s = max(1, min(h, w) / 256) and d the number of decimal digits of t, the s (6 d + 1) x 9 s pixels from the rectangle's top left corner,
 * clipped by the frame and not by the rectangle; digit j (the most significant first) has its glyph's origin at (X0 + s (1 + 6 j), Y0 + s),
 * glyph pixel ((x - ox) / s, (y - oy) / s) of 5 x 7 is black where the font's bit is set, the rest of the plate is colour(t), opaque.
 * Priority at a pixel: a plate (the smallest label first), a border (the smallest label first), the outline, the tint.
 * The search runs only where its answer shows (grey != 0 or an outline pixel).  No read or write is out of range for any int32 content
 * of labels, ids and table.
 * guide, grey, labels, ids, table, font, out not NULL, labels / ids / table 4-byte aligned, 1 <= n <= 65535, h, w >= 1, max_objects >= 1,
 * colour, alpha256, thickness, boxes, layout in range, no unknown flag, else CGS_ERR_BADARG (nothing is launched); then 64 <= h, w <=
 * CGS_FIT_MAX_SIDE and max_objects <= CGS_OVERLAY_MAX_TRACK_OBJECTS, else CGS_ERR_UNSUPPORTED.                                          */
enum { CGS_OVERLAY_MAX_TRACK_OBJECTS = 64, CGS_OVERLAY_MAX_BOXES = 4, CGS_OVERLAY_FONT_GLYPHS = 10, CGS_OVERLAY_FONT_ROWS = 7 };
int cgs_overlay_compose_tracks(const uint8_t* guide, const uint8_t* grey, const uint8_t* hard, const int32_t* labels, const int32_t* ids,
                               const int32_t* table, const uint8_t* font, int32_t n, int32_t h, int32_t w, int32_t max_objects, int32_t r,
                               int32_t g, int32_t b, int32_t alpha256, int32_t thickness, int32_t boxes, int32_t layout, int32_t flags,
                               uint8_t* out, cgs_stream_t stream);

/* cgs_overlay_compose_tracks_carried (csrc/overlay_tracks.hip; -process --source-video --overlay-fill): cgs_overlay_compose_tracks with
 * the objects that cgs_objects_track_fill carried into a frame drawn hatched, so that a carried mask shows as what it is.
 *   age       int32 [n][K]: cgs_objects_track_fill's age.  Object l of frame f is a carried one when age[f][l - 1] > 0; any int32
 *             content is read safely.  Every other argument is cgs_overlay_compose_tracks's.
 * With s = max(1, min(h, w) / 256), the plate scale, pixel (y, x) of the overlay panel is on the stripe when ((x + y) / (2 s)) & 1 == 0.
 *   tint      off the stripe a pixel whose object is a carried one gets no tint: q = 0, the frame's pixel passes through
 *   border    off the stripe a border pixel of a carried object's box is not a border pixel of that object; the lower priorities
 *             (the borders of the later labels, the outline, the tint) then apply
 * Plate, digits, outline and every object with age <= 0 are as in cgs_overlay_compose_tracks, and so are the frame panel and the grey
 * panel.  With every age <= 0 the output is cgs_overlay_compose_tracks's byte for byte, at every access width, layout and box
 * thickness.  age not NULL and 4-byte aligned, else CGS_ERR_BADARG; the other checks are cgs_overlay_compose_tracks's.               */
int cgs_overlay_compose_tracks_carried(const uint8_t* guide, const uint8_t* grey, const uint8_t* hard, const int32_t* labels,
                                       const int32_t* ids, const int32_t* table, const int32_t* age, const uint8_t* font, int32_t n,
                                       int32_t h, int32_t w, int32_t max_objects, int32_t r, int32_t g, int32_t b, int32_t alpha256,
                                       int32_t thickness, int32_t boxes, int32_t layout, int32_t flags, uint8_t* out, cgs_stream_t stream);

/* ---- block-matched motion for the temporal filter (csrc/temporal_motion.hip; -process --source-video --smooth R --smooth-motion S) -------
 * cgs_temporal_smooth looks, for a tap in frame f + k, at the 3 x 3 cells around the cell's own position whatever k is; under a camera pan
 * of a few cells a frame those taps leave the object and the range term switches them off.  These two entries estimate the motion of
 * whole cells between neighbouring frames and let the taps follow it.  Both run on `stream` without synchronising, allocate nothing, use
 * no global atomics, are deterministic and can be captured in a graph.
 *
 * cgs_temporal_flow: one integer vector per block of CGS_TEMPORAL_BLOCK x CGS_TEMPORAL_BLOCK cells and pair of neighbouring frames.
 *   low     uint8 [n][64][64][3]: cgs_fit_down_u8 of the frames
 *   search  S, 1 .. CGS_TEMPORAL_MAX_SEARCH cells each way
 *   fwd     int8 [n - 1][8][8][2], components (dy, dx): fwd[g][by][bx] = the d, |dy|, |dx| <= S, that minimises
 *             SAD(d) = sum over the 64 cells q of block (by, bx) and the colours c of |low[g][q][c] - low[g + 1][q + d][c]|   (an integer)
 *           among the candidates whose displaced block lies entirely inside the grid ((0, 0) always does)
 *   bwd     int8 [n - 1][8][8][2]: the same with frame g + 1 as the source and frame g searched -- not the negation of fwd
 * The candidates are ranked by ascending dy^2 + dx^2, then dy, then dx, and a later one wins only with a strictly smaller SAD: ties go to
 * the smallest motion, a constant frame gives all zeros.  (SAD <= 64 * 765 = 48960 and the rank is below 81: SAD << 7 | rank is one
 * uint32 key and the answer is its minimum.)  A vector depends on its two frames only, so a caller that works in windows gets, pair for
 * pair, the vectors of the one-call run.
 * low, fwd, bwd not NULL, n >= 2, search >= 1, else CGS_ERR_BADARG (nothing is launched); then search <= CGS_TEMPORAL_MAX_SEARCH, else
 * CGS_ERR_UNSUPPORTED.
 *
 * cgs_temporal_smooth_mc: cgs_temporal_smooth with the taps of frame f + k centred where the motion carries the cell.
 *   z, low, n, f0, f1, radius, sigma_r, out   as cgs_temporal_smooth
 *   fwd, bwd  int8 [n - 1][8][8][2] as cgs_temporal_flow writes them (of the same n frames); not read, and may be NULL, when n == 1
 * The path of cell p of frame f: m_0 = (0, 0) and, for j = 0 .. k - 1, q = p + m_j with each coordinate clamped into 0 .. 63,
 *   m_{j+1} = m_j + fwd[f + j][q.y >> 3][q.x >> 3]             (k > 0)
 *   m_{j+1} = m_j + bwd[f - j - 1][q.y >> 3][q.x >> 3]         (k < 0, j = 0 .. |k| - 1)
 * The taps are those of cgs_temporal_smooth IN THE SAME ORDER -- the centre tap (f, p) with weight exactly 1, then k = -radius .. -1, 1 ..
 * radius ascending with 0 <= g = f + k < n, dy = -1, 0, 1 (outer), dx = -1, 0, 1 (inner) -- at the cell t = p + m_k + (dy, dx) of frame g
 * when t lies inside the grid (skipped, not clamped, otherwise; p + m_k itself may lie outside):
 *   w = exp(-(k^2 / (2 sigma_t^2) + (dy^2 + dx^2) / 2 + d2 / (2 sigma_r^2))),  d2 = |low[g][t] - low[f][p]|^2 (an integer),
 *   num = fma(w, z[g][t], num),  den = den + w,  out = num / den (the IEEE division).
 * The spatial term counts (dy, dx) only, not m_k: following the motion costs no weight.  The arithmetic and its order are those of
 * cgs_temporal_smooth, so all-zero fields give its output bit for bit; den >= 1, 0 <= out <= 1, ones in give 1.0f out, and with `radius`
 * frames of halo a window gives the one-call result bit for bit, as there.  No read is out of range for any int8 content of the fields;
 * components beyond +-CGS_TEMPORAL_MAX_SEARCH are the caller's error and merely move the taps further.  Compensated: translation by whole
 * cells, up to S cells a frame, one vector per 8 x 8 block.  Not compensated: motion inside a block, sub-cell motion, occlusion (no
 * forward / backward consistency check) -- there the range term is what is left.  Block 8 and S <= 4 are judgements, not tuned results.
 * As cgs_temporal_smooth: z, low, out not NULL, n >= 1, 0 <= f0 < f1 <= n, radius >= 1, sigma_r > 0 and finite, z / out 4-byte aligned,
 * and fwd, bwd not NULL when n > 1, else CGS_ERR_BADARG (nothing is launched); then radius <= CGS_TEMPORAL_MAX_RADIUS, else
 * CGS_ERR_UNSUPPORTED.                                                                                                                    */
enum { CGS_TEMPORAL_BLOCK = 8, CGS_TEMPORAL_MAX_SEARCH = 4 };
int cgs_temporal_flow(const uint8_t* low, int32_t n, int32_t search, int8_t* fwd, int8_t* bwd, cgs_stream_t stream);
int cgs_temporal_smooth_mc(const float* z, const uint8_t* low, const int8_t* fwd, const int8_t* bwd, int32_t n, int32_t f0, int32_t f1,
                           int32_t radius, float sigma_r, float* out, cgs_stream_t stream);

/* ---- GrabCut-style mask refinement by an exact min cut (csrc/graph_cut.hip) --------------------------------------------------------------
 * cgs_graph_cut: for each of n frames of h x w cells (1 <= h, w <= CGS_CUT_MAX_SIDE), frames uint8 [n][h][w][3] (RGB), z fp32 [n][h][w],
 * the labelling of a binary graph cut that is seeded by the mask and uses colour models of the frame's own foreground and background.
 * Everything is an integer or an fp32 compare; costs are in S = 16 units per nat and come from three int32 tables the caller builds in
 * float64: wa, wd [CGS_CUT_TABLE] and l [CGS_CUT_LOG_TABLE] (below).  This comment is the rule.
 *   1. seed    the seed label of a cell is z > thresh (CGS_OBJ_F32_GT) or z >= thresh (CGS_OBJ_F32_GE), compared in fp32, a NaN is off.
 *              A cell is hard background where z < lo or z is a NaN, hard foreground where z > hi, and unknown otherwise.
 *              lo <= thresh <= hi, so a hard cell agrees with its seed label.  The first labelling is the seed labelling.
 *   2. n-links connectivity 4: the pairs of horizontal and vertical neighbours (axial); 8: also the two diagonals.  d2 of a pair is the
 *              squared distance of its two RGB triples (an integer), P the number of unordered pairs of the frame, and
 *              m = max(1, sum(d2) / P) in integer division (m = 1 when P = 0); idx = min(CGS_CUT_TABLE - 1, 64 d2 / m), again an integer
 *              division.  The capacity of the pair, in both directions, is wa[idx] when it is axial and wd[idx] when it is diagonal.
 *              wa[i] = rint(S lambda exp(-i / 128)), wd[i] = rint(S lambda exp(-i / 128) / sqrt(2)), lambda a whole number 0..100:
 *              GrabCut's beta = 1 / (2 <d2>) in integers.
 *   3. models  histograms, not mixtures: b = `bins` (4 or 8) bins a channel, B = b^3, bin = (R >> s) b^2 + (G >> s) b + (B >> s) with
 *              s = 8 - log2 b.  H1 / H0 count the cells the current labelling has on / off (hard cells included), N1 / N0 are their
 *              sizes.  N1 = 0 or N0 = 0: the labelling stays, status gains CGS_CUT_EMPTY and the frame is finished.  Else an unknown
 *              cell has cost_fg = l[N1 + B] - l[H1[bin] + 1] and cost_bg = l[N0 + B] - l[H0[bin] + 1], l[k] = rint(S ln k) for
 *              k = 1 .. 4096 + 512 (l[0] is not read), and the t-links source -> cell = cost_bg, cell -> sink = cost_fg.  A hard
 *              foreground cell has source -> cell = BIG, cell -> sink = 0, a hard background cell the mirror; BIG = 8 wa[0] + 1 is more
 *              than a cell's n-links together, and 4096 BIG < 2^31.
 *   4. cut     the new labelling is on exactly in the cells that cannot reach the sink in the residual graph of a maximum flow: the
 *              largest source side of a minimum cut, which is unique and depends neither on the algorithm nor on any order.  `energy`
 *              is the value of that flow in the whole graph (the part min(source -> cell, cell -> sink) that passes straight through
 *              a cell included).
 *   5. iterate steps 3 and 4 up to `iters` times (1..CGS_CUT_MAX_ITERS).  A cut that returns the labelling it started from ends the
 *              iteration; status gains CGS_CUT_EARLY when fewer than `iters` cuts had been run by then.
 *   6. out     uint8 [n][h][w], 1 = on.  stats int32 [n][CGS_CUT_FIELDS]: status bits, cuts completed, the most rounds a cut of the
 *              frame took (below), energy of the last completed cut (0: none), cells on in the seed labelling, cells on in out, unknown
 *              cells, cells of out that differ from the seed labelling.
 * How it is computed (no part of the rule but for `rounds`): one workgroup per frame, the whole graph in LDS; push-relabel with the
 * source folded into an initial excess, in rounds.  A round is an exact backward breadth-first search from the sink over residual arcs (at
 * most h w steps); the cut is finished when no cell with excess has a finite distance -- the label is then "distance infinite" -- else
 * a constant number of sweeps follows, each a push phase and a relabel phase with a barrier between them.  The rounds of a cut are the
 * searches it ran, at least 1.  A cut that is not finished by its max_rounds-th search leaves the labelling it started from, sets
 * CGS_CUT_NOT_CONVERGED, counts max_rounds as its rounds and ends the frame: every loop is bounded, whatever the input.
 * frames, z, wa, wd, l, out, stats not NULL, z / wa / wd / l / stats 4-byte aligned, n >= 1, src_kind CGS_OBJ_F32_GT or CGS_OBJ_F32_GE,
 * lo <= thresh <= hi (none a NaN), connectivity 4 or 8, bins 4 or 8, 1 <= iters <= CGS_CUT_MAX_ITERS, 1 <= max_rounds <= CGS_CUT_MAX_ROUNDS,
 * else CGS_ERR_BADARG (nothing is launched); then 1 <= h, w <= CGS_CUT_MAX_SIDE, else CGS_ERR_UNSUPPORTED.  Tables other than the rule's
 * (wa[0] above 1600, which would not fit the 16-bit residuals) are the caller's error; no read or write is out of range for any content.
 * cgs_graph_cut_sweeps is the same with the number of sweeps a round (16, 32 or 64, else CGS_ERR_UNSUPPORTED) chosen by the caller: the
 * result is the rule's at every value but for `rounds`; tools/time_graph_cut.py times the three.  cgs_graph_cut runs CGS_CUT_SWEEPS.   */
enum { CGS_CUT_MAX_SIDE = 64, CGS_CUT_FIELDS = 8, CGS_CUT_TABLE = 1024, CGS_CUT_LOG_TABLE = 4096 + 512 + 1, CGS_CUT_MAX_ITERS = 8 };
enum { CGS_CUT_SCALE = 16, CGS_CUT_MAX_LAMBDA = 100, CGS_CUT_SWEEPS = 16, CGS_CUT_MAX_ROUNDS = 1 << 16 };
enum { CGS_CUT_EMPTY = 1, CGS_CUT_EARLY = 2, CGS_CUT_NOT_CONVERGED = 4 };
int cgs_graph_cut(const uint8_t* frames, const float* z, int32_t src_kind, float thresh, float lo, float hi, int32_t n, int32_t h, int32_t w,
                  int32_t connectivity, int32_t bins, int32_t iters, int32_t max_rounds, const int32_t* wa, const int32_t* wd,
                  const int32_t* l, uint8_t* out, int32_t* stats, cgs_stream_t stream);
int cgs_graph_cut_sweeps(const uint8_t* frames, const float* z, int32_t src_kind, float thresh, float lo, float hi, int32_t n, int32_t h,
                         int32_t w, int32_t connectivity, int32_t bins, int32_t iters, int32_t max_rounds, int32_t sweeps, const int32_t* wa,
                         const int32_t* wd, const int32_t* l, uint8_t* out, int32_t* stats, cgs_stream_t stream);

const char* cgs_build_arch(void);
int cgs_abi_version(void);

/* ---- optional BatchNorm2d (+ ReLU / LeakyReLU) epilogue (csrc/bn.hip) ------------------------------------------------------------------
 * SURVEY section 8 row f4 ("an optional BN epilogue") / the north_star's BN wording.  The reference has NO BatchNorm: this op is on
 * no parity path and nothing of the reference pins it (tests: torch.nn.BatchNorm2d + autograd in float64).  NHWC fp32 x / y / dy / dx
 * [pixels][c], c a multiple of 4, <= 64; act: CGS_ACT_NONE / RELU / LRELU.  train != 0: batch statistics (biased variance for the normalisation,
 * unbiased into running_var, momentum as torch); train == 0: running statistics.  stats [c][4] = mean, 1/sqrt(var+eps), scale, shift.
 * ws: (3 cgs_bn_rows(pixels, c) + 2) * c floats.  Statistics are per GPU under data parallelism (no collective).                          */
int cgs_bn_rows(int64_t pixels, int32_t c);
int cgs_bn_act_fwd(int64_t pixels, int32_t c, const float* x, const float* gamma, const float* beta, float eps, int32_t act, float slope,
                   int32_t train, float* y, float* stats, float* ws, float* running_mean, float* running_var, float momentum,
                   cgs_stream_t stream);
int cgs_bn_act_bwd(int64_t pixels, int32_t c, const float* x, const float* y, const float* dy, const float* stats, int32_t act, float slope,
                   int32_t train, float* dx, float* dgamma, float* dbeta, float* ws, cgs_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* CGS_HIP_H */
