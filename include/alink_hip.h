/*
 * alink_hip.h — C-ABI of libalink_hip.so, the MI355X (gfx950) implementation of A-LINK's
 * face-recognition hot path.
 *
 * The reference (iamgroot42/A-LINK) has NO native boundary: its hot path is Python duck typing on
 * top of MXNet / Keras.  Every entry point below therefore cites the reference *call site* it
 * replaces (paths relative to the reference checkout).  A maintainer binds these with ctypes (see
 * INTEGRATION.md); this repo's own host side (a-link_amd/_abi.py) does exactly that.
 *
 * Conventions
 *   - every function returns 0 on success or a negative ALINK_E* code; nothing throws across the ABI;
 *     alink_last_error() returns a thread-local human-readable message for the last failure.
 *   - all `dev_*` pointers are device (HBM) pointers owned by the caller (PyTorch-ROCm in this repo);
 *     `stream` is a hipStream_t passed as void* (NULL = default stream).  No entry point allocates,
 *     frees or synchronises inside the launch path (graph-capture safe), except *_create / *_finalize
 *     / *_destroy / *_profile which are documented as synchronous.
 *   - handles are opaque, one per (process, GPU); a handle is not thread-safe (the reference is
 *     single-threaded: code/ALINK_arc.py:22-25).
 *   - pixels are what the reference feeds its models: float32, RGB, 0..255
 *     (code/readDFW.py:82,124); 512-d embeddings and all head tensors are float32.
 */
#ifndef ALINK_HIP_H
#define ALINK_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALINK_OK          0
#define ALINK_EINVAL     -1   /* bad argument / shape the kernels do not support            */
#define ALINK_ENOMEM     -2   /* hipMalloc failed or caller workspace too small              */
#define ALINK_EHIP       -3   /* a HIP runtime call failed (message has hipGetErrorString)   */
#define ALINK_ESTATE     -4   /* call order violated (e.g. embed before finalize)            */
#define ALINK_ENOTFOUND  -5   /* unknown tensor name                                         */

/* activation / weight storage type of the backbone GEMMs (accumulation is always f32) */
#define ALINK_DT_BF16 0
#define ALINK_DT_F16  1
#define ALINK_DT_F32  2   /* pair head: alink_head_set_compute_dtype; IR backbone: the float32 precision mode */
#define ALINK_DT_F16X2 3  /* IR backbone only: split precision — every activation and folded weight is an f16 PAIR   */
                          /* hi + lo (22 significant bits, power-of-two scales per tensor), three products hi*hi,     */
                          /* hi*lo, lo*hi on the f16 matrix cores into f32 accumulators: the accuracy of the float32  */
                          /* mode (selection sets identical to the f32 arithmetic) at ~1/3 of the bf16 rate.          */
                          /* Needs alink_backbone_calibrate before the first alink_embed; embed / profile / the small-    */
                          /* batch latency mode, no gradient pass.                                                    */

/* input pixel layouts accepted by alink_embed */
#define ALINK_LAYOUT_NHWC_F32 0   /* what siamese.ArcFace.process receives (code/siamese.py:232-234) */
#define ALINK_LAYOUT_NCHW_F32 1   /* what FaceModel.get_feature receives  (code/face_model.py:83-88)  */
#define ALINK_LAYOUT_NHWC_U8  2   /* extension: raw 8-bit pixels, 4x less input traffic              */

const char* alink_last_error(void);
/* Prepares `device` (function attributes, hardware-contract probe); idempotent; the caller's current device
 * is left unchanged.  DEVICE RULE for the whole library: a handle lives on the device that was current
 * when it was created (one process per GPU: torch.cuda.set_device(LOCAL_RANK) first); every entry point
 * makes its handle's device current for the duration of the call and restores the caller's; entry points
 * without a handle run on the device that owns the buffers they are given.  `stream` arguments must be
 * streams of that same device. */
int  alink_init(int device);
int  alink_version(void);

/* ------------------------------------------------------------------------------------------------
 * Backbone: insightface LResNet-E-IR ("ArcFace") feature extractor.
 * Replaces face_model.get_model (code/face_model.py:28-41: mx.model.load_checkpoint + bind) and
 * FaceModel.get_feature (code/face_model.py:86-93: forward + sklearn normalize).
 * ---------------------------------------------------------------------------------------------- */
typedef struct alink_backbone alink_backbone_t;

typedef struct {
    int units[4];      /* residual units per stage: r100 = {3,13,30,3}, r50 = {3,4,14,3}   */
    int widths[5];     /* {64,64,128,256,512}: stem width then one per stage (multiples of 64) */
    int height, width; /* input size; "112,112" in code/siamese.py:222                       */
    int emb;           /* embedding size (512), multiple of 64                               */
    int dtype;         /* ALINK_DT_BF16 | ALINK_DT_F16 | ALINK_DT_F32 (the reference's own precision:  */
                       /* exact-f32 MFMA GEMMs, ~1/12 of the bf16 rate; embed only, no profile / gradient) */
    float bn_eps;      /* 2e-5 in the insightface symbol                                     */
} alink_ir_cfg;

alink_backbone_t* alink_backbone_create(const alink_ir_cfg* cfg);
void alink_backbone_destroy(alink_backbone_t* bb);

/* Hand over one raw checkpoint tensor (host float32, MXNet layout and MXNet names:
 * conv (O,I,kh,kw); FC (O, C*H*W); BN gamma/beta/moving_mean/moving_var; PReLU gamma).
 * This is the per-tensor body of arg_params/aux_params in code/face_model.py:34,40. */
int alink_backbone_load(alink_backbone_t* bb, const char* name, const float* host, size_t count);
/* number of tensors the configured network expects, and the i-th expected name / element count */
int alink_backbone_num_tensors(const alink_backbone_t* bb);
int alink_backbone_tensor_info(const alink_backbone_t* bb, int i, const char** name, size_t* count);
/* fold BN into weights/biases, convert, upload.  Synchronous; allocates device memory. */
int alink_backbone_finalize(alink_backbone_t* bb);

/* Optional: split one alink_embed call into up to `n` (1..8, default 1 = off) independent image
 * shards of >= 64 images on internal streams (ordered after / before `stream` with events).  Results
 * do not depend on n.  Callers that embed many batches get more from issuing whole 256-image calls
 * round-robin on their own streams (what a-link_amd/backbone.py does): the calls are independent. */
int alink_backbone_set_streams(alink_backbone_t* bb, int n);

size_t alink_backbone_workspace_bytes(const alink_backbone_t* bb, int n_images);

/* N images -> N L2-normalised embeddings (code/face_model.py:86-93, batched).
 * dev_in: pixels in `layout`; dev_out: N x emb float32. */
int alink_embed(alink_backbone_t* bb, const void* dev_in, int layout, int n_images,
                float* dev_out, void* dev_workspace, size_t workspace_bytes, void* stream);

/* Per-launch timing of one alink_embed with HIP events on `stream` (synchronous; for bench.py's
 * roofline).  Every kernel is launched 4 times back to back between its events and the mean is
 * reported, so the events' own cost is not booked as kernel time.  ms[i]/flops[i]/kind[i] describe launch i; kind: 0 stem, 1 implicit-GEMM conv,
 * 2 FC split-K GEMM, 3 FC finish.  *n_launches in: capacity, out: count.  Convolutions keep one entry per layer of the chain:
 * where one launch computes two layers (a fused stage-1 unit, unit_c64.hip) each gets its own FLOPs and half of the launch's time. */
int alink_embed_profile(alink_backbone_t* bb, const void* dev_in, int layout, int n_images,
                        float* dev_out, void* dev_workspace, size_t workspace_bytes, void* stream,
                        float* ms, double* flops, int* kind, int* n_launches);

/* EXTENSION (not in the reference, which has only a black-box pixel attack: code/attack.py; named by
 * BASELINE.json's north_star and SURVEY.md §8f N1): d(loss)/d(pixels) through the frozen backbone for
 * FGSM / PGD.  alink_backbone_enable_grad (before finalize) also builds the transposed, flipped
 * folded weights (doubles weight memory) and refuses checkpoints with negative PReLU slopes.
 * alink_embed_cached = alink_embed that keeps what the backward pass needs in the (larger) workspace;
 * alink_embed_input_grad then maps dev_demb = d(loss)/d(embedding) (n x emb, w.r.t. the L2-normalised
 * output dev_emb of that forward) to dev_dpix = d(loss)/d(pixel) (n images, float32, NHWC or NCHW). */
int alink_backbone_enable_grad(alink_backbone_t* bb);

/* Latency mode for batches of <= 32 images (FaceModel.get_feature is a batch-1 call: code/face_model.py:86-93).
 * A 3x3 layer at batch 1 has a handful of workgroups that each walk all of K; with the switch on such layers
 * are split over K into f32 partial slabs added in a fixed order (IR-ResNet-100: batch 1 2.3 -> 1.6 ms, batch 16
 * 2.4 -> 2.2 ms).  Default OFF: a split sum rounds differently from the fused one, so an image's
 * embedding would no longer be bit-identical whatever batch it arrives in.  Changes the workspace size:
 * query alink_backbone_workspace_bytes after setting it. */
int alink_backbone_set_small_batch_split(alink_backbone_t* bb, int on);

/* ALINK_DT_F16X2 (split precision) only.  The mode stores every activation as an f16 pair scaled by a power of two
 * per tensor, chosen so that the largest value a tensor takes on the calibration images lands in [1024, 2048) —
 * 32x below the f16 overflow threshold, the lo halves of values down to 2^-13 of it normal f16.  A power-of-two scale is
 * exact for every value whose lo half stays normal; far smaller values (lo subnormal) round differently under another
 * scale, so two calibrations move an embedding by ~2e-7 — far below the mode's own error (2e-6), not zero: embeddings are
 * bit-reproducible for FIXED scales (alink_backbone_get_scales / set_scales carry them between processes, ranks and
 * checkpoints).  The calibration images only have to be "like" later inputs within that 32x.  Synchronous; runs the n_images (<= what the workspace was sized for) through
 * the network layer by layer.  merge != 0 keeps every exponent at or below its current value (re-calibration after
 * alink_backbone_range_flag reported a batch that left the range).  Must run once before the first alink_embed. */
int alink_backbone_calibrate(alink_backbone_t* bb, const void* dev_in, int layout, int n_images,
                             void* dev_workspace, size_t workspace_bytes, int merge, void* stream);
/* 16-bit storage modes (BF16 cannot, F16 and F16X2 can leave their range): 1 if, since the last reset, any embedding
 * written by alink_embed was non-finite.  The word lives in pinned host memory the last kernel of a forward writes;
 * the caller must have synchronised the streams it embedded on.  reset != 0 clears it. */
int alink_backbone_range_flag(alink_backbone_t* bb, int reset);
/* the device this handle lives on (the one current at alink_backbone_create: the device rule at the top of this header); -1 for NULL */
int alink_backbone_device(const alink_backbone_t* bb);
/* The calibration state of the split-precision mode, portable: one scale exponent per tensor (the stem's output, then every
 * convolution launch's output, in launch order; stored value = true value x 2^e).  An embedding is bit-reproducible for
 * FIXED scales only (a different scale moves the lo halves of values far below the tensor's maximum through different
 * f16 roundings: drift ~2e-7, far below the mode's own error, but not zero) — so a checkpoint saved for later
 * (reference code/siamese.py:114-125 is the save / load contract of the models) and the ranks of a one-process-per-GPU
 * job, whose top-k merge assumes replicated arithmetic, must SHARE them: get them on the rank / in the process that
 * calibrated, set them everywhere else.  num_scales is 0 for any other dtype.  set_scales marks the handle calibrated. */
/* Split precision only.  n = 3 (default): every multiplication as X_hi W_hi + X_hi W_lo + X_lo W_hi — the exact mode.
 * n = 1: X_hi W_hi alone — the SCREENING form on the same handle (same folded weights, same calibrated scales, same
 * workspace): one matrix-core product per multiplication like the plain f16 mode, but with nothing to overflow (the scales)
 * and the residual stream still carried and added as hi + lo, so only the rounding of each convolution's operands to 11 bits
 * remains.  For screen-then-settle selection (a-link_amd/settle.py): screen with n = 1, settle with n = 3.  Takes effect
 * for launches enqueued after the call.  Calibration always runs with n = 3. */
int alink_backbone_set_products(alink_backbone_t* bb, int n);
int alink_backbone_num_scales(const alink_backbone_t* bb);
int alink_backbone_get_scales(const alink_backbone_t* bb, int* exponents, int n);
int alink_backbone_set_scales(alink_backbone_t* bb, const int* exponents, int n);
size_t alink_backbone_grad_workspace_bytes(const alink_backbone_t* bb, int n_images);
int alink_embed_cached(alink_backbone_t* bb, const void* dev_in, int layout, int n_images, float* dev_out,
                       void* dev_workspace, size_t workspace_bytes, void* stream);
int alink_embed_input_grad(alink_backbone_t* bb, const float* dev_demb, const float* dev_emb, int layout,
                           int n_images, float* dev_dpix, void* dev_workspace, size_t workspace_bytes,
                           void* stream);

/* Diagnostic / unit-test entry: one fused NHWC convolution launch of the implicit-GEMM kernel
 *   out = [prelu_alpha]( conv(in, w) + bias[class] ) [+ resid]
 * dev_w is (Cout, ksz, ksz, Cin) in `dtype` in NATURAL cout order (the call permutes a private
 * copy — synchronous, test use only); dev_bias is (ncls, Cout) f32 with ncls = 9 if border_cls.
 * `fine`: where the linear-tile kernel applies (3x3 stride 1 on 7/14/28-wide maps), 1 / 0 force its
 * 64- / 128-channel workgroup form, < 0 chooses by grid size exactly as alink_embed does. */
int alink_conv_nhwc(int dtype, const void* dev_in, const void* dev_w, const float* dev_bias,
                    const float* dev_alpha, const void* dev_resid, void* dev_out,
                    int N, int H, int W, int Cin, int Cout, int ksz, int stride, int pad,
                    int border_cls, int fine, void* stream);

/* Split-precision twin (ALINK_DT_F16X2 kernels): every tensor float32 in its natural layout on the device — dev_w
 * (Cout, ksz, ksz, Cin), dev_resid / dev_out (M, Cout) — converted to and from f16 pairs on the host (synchronous,
 * test use only); e_*: the power-of-two scale exponents the stored tensors carry (stored = true x 2^e). */
int alink_conv_nhwc_x2(const float* dev_in, const float* dev_w, const float* dev_bias, const float* dev_alpha,
                       const float* dev_resid, float* dev_out, int N, int H, int W, int Cin, int Cout, int ksz,
                       int stride, int pad, int border_cls, int fine, int e_in, int e_w, int e_out, int e_res,
                       void* stream);

/* Diagnostic / unit-test entries that reach every launch form and report what ran.  alink_conv_nhwc_ex is alink_conv_nhwc plus:
 *   route        0 = the kernel direct_variant chooses (the 16-bit forward), 1 = direct_variant_tiles (backward passes, ResNet-50, VGG16)
 *   dev_dact     (M, Cout) in `dtype`, or NULL: backward epilogue, out = (conv + bias) * (dact > 0 ? 1 : alpha[c]); needs dev_alpha
 *   post_relu    ReLU after the residual add (keeps a NaN)
 *   dev_in2, dev_w2, Cin2, in2_compact: a fused 1x1 projection shortcut, out += conv1x1(in2, w2) sampled at (oy * stride, ox * stride);
 *                dev_in2 (N, H, W, Cin2), or (N, Ho, Wo, Cin2) if in2_compact; dev_w2 (Cout, Cin2) in natural order
 *   splitk       > 1: the K walk cut into that many f32 slabs (allocated by the call) and summed by the split-finish kernel
 *   kernel_out   the ConvKernel value chosen (csrc/conv_kernel.h), form_out: 0 = that kernel itself, 1 = conv3x3_lat_kernel,
 *                2 = conv_gemm_lat_kernel; either may be NULL; both are -1 when the call fails before choosing
 * A combination the chosen kernel has no form of (the rolling-row kernels with dact / post_relu / splitk, a shortcut on a tile
 * kernel, split precision with dact ...) returns an error code with alink_last_error set and launches nothing. */
int alink_conv_nhwc_ex(int dtype, const void* dev_in, const void* dev_w, const float* dev_bias,
                       const float* dev_alpha, const void* dev_resid, void* dev_out,
                       int N, int H, int W, int Cin, int Cout, int ksz, int stride, int pad,
                       int border_cls, int fine, int route, const void* dev_dact, int post_relu,
                       const void* dev_in2, const void* dev_w2, int Cin2, int in2_compact, int splitk,
                       int* kernel_out, int* form_out, void* stream);

/* alink_conv_nhwc_x2 plus nprod (3, or 1: the one-product screening form), splitk, post_relu and the two reports. */
int alink_conv_nhwc_x2_ex(const float* dev_in, const float* dev_w, const float* dev_bias, const float* dev_alpha,
                          const float* dev_resid, float* dev_out, int N, int H, int W, int Cin, int Cout, int ksz,
                          int stride, int pad, int border_cls, int fine, int e_in, int e_w, int e_out, int e_res,
                          int nprod, int splitk, int post_relu, int* kernel_out, int* form_out, void* stream);

/* alink_gemm32_ex: ONE launch of the exact-f32 GEMM (csrc/sgemm.hip: SmallRes, the float32 backbone mode, the margin loss) with
 * every caller-settable field of its launch descriptor in the caller's hands, and a report of what ran.  C[M][N] = A[M][K] . B[K][N],
 * all operands float32 on the device; the fields are those of alink::GemmP (csrc/sgemm.h), which documents them:
 *   amode  0 = A row-major [M][lda], 1 = A given as [K][lda] (columns = m), 2 = im2col gather of an NHWC tensor (m = (n, oy, ox),
 *          k = (ky, kx, ci)), 3 = its transpose with the reduction over pixels and one extra row of ones (M = 9 Ci + 1)
 *   bmode  0 = B row-major [K][ldb], 1 = B given as [N][ldb], 2 = 3x3 weights (ky, kx, ci, co) flipped and transposed (input gradient)
 *   max_split  >= 1: the split along K is planned as production plans it (gemm32_plan_split with this limit; d->splitk and
 *              d->kper are ignored); 0: the caller's d->splitk / d->kper are used as they stand — the fixed plans of
 *              alink_smallres_score_pairs and of the float32 backbone's FC
 *   dev_workspace, workspace_floats: the split's partial slabs, splitk x M x ldc floats; may be NULL / 0 for an unsplit launch
 *   report     NULL, or int[5] = { tile columns (32: the 128 x 32 tile, 64: the 64 x 64 tile), stage depth (16 | 64),
 *              loaders (1: 16-byte, 0: 4-byte), splitk, kper } as the launcher itself decides them; all -1 when the call is refused
 * A request the launcher rejects (a split with ldc != N or without workspace, bmode 2 with Ci % 4 != 0 or amode != 2, a mode pair
 * without a kernel, kper no multiple of 16, force_bk other than 0 / 16 / 64) or a workspace that is too small returns an error
 * code with alink_last_error set and launches nothing.  Synchronous (test use only). */
enum { ALINK_GEMM_A_ROW = 0, ALINK_GEMM_A_COL = 1, ALINK_GEMM_A_CONV = 2, ALINK_GEMM_A_CONVT = 3 };
enum { ALINK_GEMM_B_ROW = 0, ALINK_GEMM_B_COLT = 1, ALINK_GEMM_B_FLIP = 2 };
typedef struct alink_gemm32_desc {
    const float* A;
    const float* B;
    float* C;
    const float* A2;
    int a_split;
    int M, N, K, lda, ldb, ldc;
    int amode, bmode;
    int H, W, Ci, Ho, Wo, pad, prescale, ks, cstride;
    float pre_sub, pre_mul;
    const float* bias;
    const float* act;
    const float* alpha;
    const float* resid;
    int relu, accumulate;
    int splitk, kper;
    int force_bk;
} alink_gemm32_desc;
int alink_gemm32_ex(const alink_gemm32_desc* d, int max_split, float* dev_workspace, size_t workspace_floats, int* report,
                    void* stream);

/* ------------------------------------------------------------------------------------------------
 * VGGFace2 ResNet-50 feature extractor: siamese.RESNET50 (code/siamese.py:203-216) =
 * keras_vggface VGGFace(model='resnet50', include_top=False) cut at 'avg_pool', flattened (2048-d),
 * fed through utils.preprocess_input(version=2).  Tensors are handed over with Keras names and
 * layouts: "<layer>/kernel" (kh, kw, in, out), "<layer>/bn/{gamma,beta,moving_mean,moving_variance}",
 * layers conv1/7x7_s2 and conv{2..5}_{u}_{1x1_reduce,3x3,1x1_increase,1x1_proj}.
 * alink_resnet50_embed: dev_in (n, H, W, 3) float32; preprocessed = 0: raw RGB 0..255 pixels (the
 * BGR flip and mean subtraction of preprocess_input happen in the stem kernel's loader);
 * preprocessed = 1: the caller already applied RESNET50.preprocess.  dev_out (n, 2048) float32.
 * ---------------------------------------------------------------------------------------------- */
typedef struct alink_resnet50 alink_resnet50_t;
alink_resnet50_t* alink_resnet50_create(int height, int width, int dtype, float bn_eps);
void alink_resnet50_destroy(alink_resnet50_t* r);
int alink_resnet50_num_tensors(const alink_resnet50_t* r);
int alink_resnet50_tensor_info(const alink_resnet50_t* r, int i, const char** name, size_t* count);
int alink_resnet50_load(alink_resnet50_t* r, const char* name, const float* host, size_t count);
int alink_resnet50_finalize(alink_resnet50_t* r);
size_t alink_resnet50_workspace_bytes(const alink_resnet50_t* r, int n_images);
int alink_resnet50_embed(alink_resnet50_t* r, const float* dev_in, int n_images, int preprocessed,
                         float* dev_out, void* dev_workspace, size_t workspace_bytes, void* stream);
/* dtype = ALINK_DT_F16X2 (split precision: features to float32 accuracy, so that selection through the drivers that use
 * this feature model — code/ALINK.py:67, code/ALINK_MTP.py:84, code/existing_al.py:58 — follows the reference's float32
 * arithmetic): as for the IR backbone, alink_resnet50_calibrate once before the first embed (and again with merge != 0 if
 * alink_resnet50_range_flag reports a batch that left the range: a non-finite feature was written since the last reset). */
int alink_resnet50_calibrate(alink_resnet50_t* r, const float* dev_in, int n_images, int preprocessed,
                             void* dev_workspace, size_t workspace_bytes, int merge, void* stream);
int alink_resnet50_range_flag(alink_resnet50_t* r, int reset);
/* the portable calibration state, as for the IR backbone (one exponent per op of the chain, in op order) */
int alink_resnet50_num_scales(const alink_resnet50_t* r);
int alink_resnet50_get_scales(const alink_resnet50_t* r, int* exponents, int n);
int alink_resnet50_set_scales(alink_resnet50_t* r, const int* exponents, int n);
/* EXTENSION, as alink_backbone_enable_grad and its three companions above: d(loss)/d(pixels) through the frozen network for
 * FGSM / PGD, 16-bit modes only (ALINK_DT_F16X2: ALINK_ESTATE).  alink_resnet50_enable_grad (before finalize) also builds the
 * transposed, flipped folded weights (doubles weight memory).  alink_resnet50_embed_cached = alink_resnet50_embed, bit for
 * bit, that keeps every activation the backward pass needs in the (larger) workspace: about 9.1 M 16-bit elements per
 * 224 x 224 image.  alink_resnet50_input_grad then maps dev_dfeat = d(loss)/d(feature) (n x 2048 float32) of that forward to
 * dev_dpix = d(loss)/d(pixel) (n x H x W x 3 float32, in the channel order of the forward's input: with preprocessed = 0 the
 * gradient with respect to the raw RGB pixels).  Same n, preprocessed and workspace as the cached forward; the gradient
 * tensors are scaled by a power of two per call (max|dev_dfeat|), so small gradients do not underflow in ALINK_DT_F16. */
int alink_resnet50_enable_grad(alink_resnet50_t* r);
size_t alink_resnet50_grad_workspace_bytes(const alink_resnet50_t* r, int n_images);
int alink_resnet50_embed_cached(alink_resnet50_t* r, const float* dev_in, int n_images, int preprocessed, float* dev_out,
                                void* dev_workspace, size_t workspace_bytes, void* stream);
int alink_resnet50_input_grad(alink_resnet50_t* r, const float* dev_dfeat, int n_images, int preprocessed, float* dev_dpix,
                              void* dev_workspace, size_t workspace_bytes, void* stream);
/* alink_resnet50_input_grad with HIP events around its stages (synchronous): ms[0] gradient scale + average pool, ms[1 .. 16] the
 * bottleneck units from conv5_3 down to conv2_1, ms[17] max-pool, ms[18] stem.  *n_stages in: capacity, out: count. */
int alink_resnet50_input_grad_profile(alink_resnet50_t* r, const float* dev_dfeat, int n_images, int preprocessed,
                                      float* dev_dpix, void* dev_workspace, size_t workspace_bytes, void* stream, float* ms,
                                      int* n_stages);
/* per-op HIP-event timing of one forward (synchronous): ms[i] / flops[i] for op i, name via op_name */
int alink_resnet50_profile(alink_resnet50_t* r, const float* dev_in, int n_images, float* dev_out,
                           void* dev_workspace, size_t workspace_bytes, void* stream, float* ms,
                           double* flops, int* n_ops);
const char* alink_resnet50_op_name(const alink_resnet50_t* r, int i);

/* ------------------------------------------------------------------------------------------------
 * VGGFace VGG-16 feature extractor: siamese.FaceVGG16 (code/siamese.py:187-200) = keras_vggface
 * VGGFace(model='vgg16', include_top=False) cut at 'pool5', flattened ((H/32)(W/32)512 = 25088 at
 * 224 x 224), fed through utils.preprocess_input(version=1).  Tensors: "conv{b}_{l}/kernel"
 * (3, 3, in, out) and "conv{b}_{l}/bias".  dev_in (n, H, W, 3) float32, raw RGB (preprocessed = 0)
 * or already preprocessed (1); dev_out (n, feature_size) float32 in Keras' Flatten order (h, w, c).
 * ---------------------------------------------------------------------------------------------- */
typedef struct alink_vgg16 alink_vgg16_t;
alink_vgg16_t* alink_vgg16_create(int height, int width, int dtype);
void alink_vgg16_destroy(alink_vgg16_t* r);
int alink_vgg16_num_tensors(const alink_vgg16_t* r);
int alink_vgg16_tensor_info(const alink_vgg16_t* r, int i, const char** name, size_t* count);
int alink_vgg16_feature_size(const alink_vgg16_t* r);
int alink_vgg16_load(alink_vgg16_t* r, const char* name, const float* host, size_t count);
int alink_vgg16_finalize(alink_vgg16_t* r);
size_t alink_vgg16_workspace_bytes(const alink_vgg16_t* r, int n_images);
int alink_vgg16_embed(alink_vgg16_t* r, const float* dev_in, int n_images, int preprocessed,
                      float* dev_out, void* dev_workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Siamese pair head: |l - r| -> Dense(h1) ReLU -> Dense(h2) ReLU -> Dense(2) -> softmax.
 * Replaces SiameseNetwork.__init__/predict/finetune/customTrainModel's Keras calls
 * (code/siamese.py:19-35, 52-58, 81-112, 130-131) and committee.Bagging.predict
 * (code/committee.py:13-20).  All f32 (exact-f32 MFMA), Keras-2.1.2 semantics.
 * ---------------------------------------------------------------------------------------------- */
typedef struct alink_head alink_head_t;

alink_head_t* alink_head_create(int d_in, int h1, int h2, float lr, float rho, float eps);
/* out_dim = 2: Dense(2) + softmax (code/siamese.py:31-32); out_dim = 1: Dense(1, sigmoid), the pair
 * scorer of the baseline scripts (code/siamese3.py:25, used by code/existing_al.py) — probabilities,
 * labels and metrics are then (n, 1). */
alink_head_t* alink_head_create_ex(int d_in, int h1, int h2, int out_dim, float lr, float rho, float eps);
void alink_head_destroy(alink_head_t* h);
size_t alink_head_num_params(const alink_head_t* h);   /* W1,b1,W2,b2,W3,b3 flattened */
/* Parameters in Keras order and layout: kernel (in,out) row-major then bias, per layer. */
int alink_head_set_params(alink_head_t* h, const float* host_params, size_t count);
int alink_head_get_params(const alink_head_t* h, float* host_params, size_t count);
int alink_head_reset_optimizer(alink_head_t* h);
/* Compute type of the head's forward / backward GEMMs: ALINK_DT_F32 (default: exact-f32 MFMA, Keras' floatx) or
 * ALINK_DT_BF16 — BASELINE configs[4]'s "bf16 fine-tune", mixed precision: parameters, gradients and Adadelta state stay
 * f32 (get/set_params, params_dev, grads_dev unchanged: the all-reduce buffer is f32); the GEMM operands are bf16 —
 * a 2-byte copy of the weights (refreshed by the update kernels) and activations / activation gradients rounded to
 * bf16 where they are produced — with exact products accumulated in f32; biases are not quantised.  Applies to
 * predict (on the bf16 matrix cores for the 512 / 64 / 2 head: 3.6x the f32 pair-scoring rate), eval and the train step alike.  The reference trains in float32 (code/siamese.py:33-35). */
int alink_head_set_compute_dtype(alink_head_t* h, int dtype);
int alink_head_get_compute_dtype(const alink_head_t* h);
/* keras.callbacks.ReduceLROnPlateau hook (code/siamese.py:54): change Adadelta's lr */
int alink_head_set_lr(alink_head_t* h, float lr);
float alink_head_get_lr(const alink_head_t* h);
/* device pointers of the flat parameter / gradient buffers (for RCCL all-reduce / broadcast by the caller).
 * The forward keeps packed copies of W1 / W2: call alink_head_params_dev again AFTER writing through the
 * pointer (each call marks those copies stale).  The gradient buffer is num_params floats followed by 4
 * spare floats: a data-parallel caller points dev_metrics of alink_head_train_step at them so that ONE
 * all-reduce carries the gradients and {loss, accuracy}. */
float* alink_head_params_dev(alink_head_t* h);
float* alink_head_grads_dev(alink_head_t* h);

/* probs[p] = softmax(head(|L[li[p]] - R[ri[p]]|)) for p < P.  li/ri may be NULL (= identity):
 * that is SiameseNetwork.predict([L,R]) (code/siamese.py:130-131); with index lists the pairs are
 * gathered from embedding matrices instead of being materialised (utilities/generateMatrixDFW.py:25-36). */
int alink_head_forward(alink_head_t* h, const float* dev_L, const float* dev_R,
                       const int32_t* dev_li, const int32_t* dev_ri, int64_t P,
                       float* dev_probs, void* stream);
/* Bagging.predict: mean over n_heads members of alink_head_forward (code/committee.py:13-20). */
int alink_committee_forward(alink_head_t* const* heads, int n_heads, const float* dev_L,
                            const float* dev_R, const int32_t* dev_li, const int32_t* dev_ri,
                            int64_t P, float* dev_probs, void* dev_scratch, void* stream);

/* The same mean when every member scores the pairs on ITS OWN feature matrices (a committee whose members
 * have different feature extractors: BASELINE configs[2], three backbones): dev_L[m] / dev_R[m] are member m's
 * embedding matrices, the index lists are shared. */
int alink_committee_forward_multi(alink_head_t* const* heads, int n_heads, const float* const* dev_L,
                                  const float* const* dev_R, const int32_t* dev_li, const int32_t* dev_ri,
                                  int64_t P, float* dev_probs, void* stream);

/* The N x N verification score matrix of utilities/generateMatrixDFW.py:25-36:
 *   scores[r][j] = mean_m softmax(head_m(|E[row0 + r] - E[j]|))[col],  r < nrows, j < n
 * (the reference keeps out[0], i.e. col = 0, of one model: n_heads = 1).  Pairs are enumerated by the
 * kernel; nothing is materialised.  dev_scores is nrows x n float32. */
int alink_pair_scores_matrix(alink_head_t* const* heads, int n_heads, const float* dev_emb, int n,
                             int row0, int nrows, int col, float* dev_scores, void* stream);

/* The RECTANGULAR score matrix of two feature matrices through one head — what the identification loop of
 * code/ALINK_MTP.py:279-288 computes one predict() per probe (every probe against every gallery face):
 *   scores[i][j] = softmax(head(|L[i] - R[j]|)),  i < nL, j < nR
 * col = -1: both columns, dev_scores is (nL, nR, od); col = 0 .. od - 1: that column alone, dev_scores is (nL, nR).
 * Pairs are enumerated by the kernel (alink_head_forward's own, row-wise: element [i][j] has the bits
 * alink_head_forward gives the materialised pair), nothing is materialised; nL == 0 or nR == 0 writes nothing.
 * LIMIT: nL * nR * od <= ALINK_HEAD_RECT_MAX_SCORES, else ALINK_EINVAL — the kernel's pair and output indices are
 * 64-bit, but the launch is one workgroup of 256 threads per 32 pairs and a launch holds fewer than 2^32 threads in a
 * grid dimension (2^29 - 32 pairs); 2^28 scores (1 GiB of float32) stays clear of that for every od.  Walk a larger
 * matrix in blocks of rows. */
#define ALINK_HEAD_RECT_MAX_SCORES (1ll << 28)
int alink_head_forward_rect(alink_head_t* h, const float* dev_L, int nL, const float* dev_R, int nR, int col,
                            float* dev_scores, void* stream);

/* One Keras train_on_batch: forward, binary_crossentropy (clip 1e-7, mean over the 2 outputs,
 * sample-weighted mean over the batch), backward, [grads left in alink_head_grads_dev],
 * then Adadelta.  dev_y is (n,2) one-hot, dev_sw (n) sample weights or NULL.
 * dev_metrics receives {loss, binary_accuracy}.  `apply` = 0 computes gradients only (the caller
 * all-reduces them, then calls alink_head_apply_update) — the data-parallel fine-tune step. */
int alink_head_train_step(alink_head_t* h, const float* dev_L, const float* dev_R,
                          const float* dev_y, const float* dev_sw, int n, float grad_scale,
                          int apply, float* dev_metrics, void* stream);
int alink_head_apply_update(alink_head_t* h, void* stream);
/* The same and, in the same launch, the same Adadelta rule (the head's lr, rho, eps) on a second parameter block of n2
 * floats: the tower of an end-to-end model (SmallRes' step ends with one update launch instead of two). */
int alink_head_apply_update_with(alink_head_t* h, float* dev_params2, const float* dev_grads2, float* dev_acc2,
                                 float* dev_dacc2, size_t n2, void* stream);
/* Optional: on a non-default stream, capture the train step into a hipGraph per distinct (operand
 * pointers, n, grad_scale, apply, lr) and replay it.  Default OFF: measured 67.8 us vs 66.2 us of plain
 * launches — the chain is bound by dependency latency between its kernels, not by launch cost. */
int alink_head_set_graph(alink_head_t* h, int on);
/* Gradient of the last alink_head_train_step's loss w.r.t. its inputs (for end-to-end models such as
 * SmallRes, code/siamese.py:158-168): dL, dR are (n, d_in) f32. */
int alink_head_input_grads(alink_head_t* h, const float* dev_L, const float* dev_R, int n,
                           float* dev_dL, float* dev_dR, void* stream);
/* The same for inputs that are the outputs of a ReLU (SmallRes' Dense(2048, relu), code/siamese.py:156):
 * gradients w.r.t. that layer's pre-activations, i.e. the above times (input > 0), in the same launch. */
int alink_head_input_grads_relu(alink_head_t* h, const float* dev_L, const float* dev_R, int n,
                                float* dev_dL, float* dev_dR, void* stream);
/* alink_head_train_step(apply = 0) and alink_head_input_grads (relu_inputs: ..._relu) as ONE call: what an end-to-end
 * model's step needs from its head (SmallRes.trainModel, code/siamese.py:158-180).  For SmallRes' own head shape
 * (128 / 32 / 2 outputs on a multiple of 256 features, at most 32 pairs, float32) the pair is three launches instead
 * of seven; other shapes run the two calls above.  Gradients are left in alink_head_grads_dev, the parameters
 * untouched (alink_head_apply_update applies them).  dev_colsum (optional, d_in floats): the column sums of the
 * 2n x d_in matrix [dL ; dR], rows ascending — the bias gradient of the layer that produced the inputs. */
int alink_head_train_step_input_grads(alink_head_t* h, const float* dev_L, const float* dev_R, const float* dev_y,
                                      const float* dev_sw, int n, float grad_scale, int relu_inputs,
                                      float* dev_dL, float* dev_dR, float* dev_colsum, float* dev_metrics,
                                      void* stream);
/* Keras test_on_batch: {loss, binary_accuracy} without touching parameters. */
int alink_head_eval(alink_head_t* h, const float* dev_L, const float* dev_R, const float* dev_y,
                    int n, float* dev_metrics, void* stream);
/* The inner loop of SiameseNetwork.customTrainModel (code/siamese.py:91-110) for `steps` consecutive steps, enqueued by ONE
 * call: per step train_on_batch on the rows that were not held out, then test_on_batch on the held-out ones — the batches
 * given as ROW INDICES into a device-resident feature table (dev_table, rows of d_in floats: left row li[r] against right row
 * ri[r]), so that no feature crosses the host boundary during an epoch (the reference stacks 2 x n x d_in floats per step).
 * host_desc: 4 int64 per step {offset into dev_idx, offset into dev_vals, n, n_held}; at dev_idx + offset: li[n] then ri[n]
 * (int32), the n_held held-out rows FIRST; at dev_vals + offset: y[n][out_dim] in the same row order, then (with_weights)
 * sample_weight[n - n_held] of the trained rows.  dev_metrics: 4 floats per step {train loss, train accuracy, held-out loss,
 * held-out accuracy}; the last two untouched when n_held = 0.  The same kernels, on the same rows in the same order, as
 * alink_head_train_step + alink_head_eval called once per step on gathered rows (bit-identical parameters and metrics). */
int alink_head_custom_train_steps(alink_head_t* h, const float* dev_table, const int32_t* dev_idx, const float* dev_vals,
                                  const int64_t* host_desc, int steps, int with_weights, float* dev_metrics, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SmallRes: the end-to-end-trained low-resolution siamese CNN (code/siamese.py:134-184):
 *   tower  conv3x3(3->32,same) relu, conv3x3(32->32,valid) relu, maxpool2, dropout.25,
 *          conv3x3(32->64,same) relu, conv3x3(64->64,valid) relu, maxpool2, dropout.25, flatten,
 *          dense(feat) relu        (shared by both inputs)
 *   head   |l-r| -> dense128 relu -> dense32 relu -> dense2 -> softmax, BCE + Adadelta
 * f32 throughout.  Pixels are (n, H, W, 3) f32; `prescale` applies SmallRes.preprocess
 * ((x-128)/128, code/siamese.py:179-181) in the first kernel.
 * Parameters in Keras order: conv kernels (3,3,in,out) + bias x4, dense (in,out) + bias, then the head.
 * ---------------------------------------------------------------------------------------------- */
typedef struct alink_smallres alink_smallres_t;
alink_smallres_t* alink_smallres_create(int img_h, int img_w, int feat, float lr, float rho, float eps);
void alink_smallres_destroy(alink_smallres_t* m);
size_t alink_smallres_num_params(const alink_smallres_t* m);
int alink_smallres_set_params(alink_smallres_t* m, const float* host, size_t count);
int alink_smallres_get_params(const alink_smallres_t* m, float* host, size_t count);
int alink_smallres_set_lr(alink_smallres_t* m, float lr);
float* alink_smallres_grads_dev(alink_smallres_t* m);      /* flat tower+head gradients (all-reduce), followed by 4 spare floats:
                                                            * a data-parallel caller points dev_metrics at them (as for alink_head_grads_dev) */
/* predict: probs (n,2).  n <= 256 per call. */
int alink_smallres_forward(alink_smallres_t* m, const float* dev_L, const float* dev_R, int n, int prescale,
                           float* dev_probs, void* stream);
/* EXTENSION (the few-pixel search against the pixel student): the same outputs for ANY n >= 0, chunked inside the call by 256,
 * asynchronous on `stream`, under a FIXED PLAN: every GEMM of the tower runs with the split count and the stage depth the planner
 * picks for that layer at a full chunk of 512 images (tile shape 128 x 32 for layers of <= 32 outputs, else 64 x 64) — functions
 * of the layer alone — and the head's forward is one row-wise kernel.  CONTRACT: row i of dev_probs has the same bits for every
 * n, every chunk boundary and every position in the call.  (alink_smallres_forward plans by the batch it is given: its bits can
 * differ from these in the last place.)  Parameters, optimizer state and gradient buffers are untouched; the handle's
 * activation buffers are overwritten. */
int alink_smallres_score_pairs(alink_smallres_t* m, const float* dev_L, const float* dev_R, int n, int prescale,
                               float* dev_probs, void* stream);
/* EXTENSION (gallery identification: code/ALINK_MTP.py:281-284 re-embeds the probe and the whole gallery for every probe).
 * The shared tower alone, one image at a time instead of one pair at a time:
 *   dev_feat[i] = relu(Dense(flatten(tower(dev_images[i]))))          (n, feat) float32, the inputs of the pair head
 * for ANY n >= 0, chunked inside the call by 512 images, asynchronous on `stream`, under the FIXED PLAN of
 * alink_smallres_score_pairs.  CONTRACT: a face has the same bits alone, in any batch, in any chunk and at any position, and
 * the bits it has inside alink_smallres_score_pairs — so alink_smallres_score_features on these rows equals
 * alink_smallres_score_pairs on the pixel pairs bit for bit.  Parameters, optimizer state and gradient buffers are untouched; the
 * handle's activation buffers are overwritten. */
int alink_smallres_features(alink_smallres_t* m, const float* dev_images, int n, int prescale, float* dev_feat, void* stream);
/* EXTENSION: alink_head_forward_rect through the model's OWN pair head (code/ALINK_MTP.py:284's predict on features computed
 * once): scores[i][j] = softmax(head(|L[i] - R[j]|)) of two feature matrices (nL, feat) and (nR, feat); col, the shape of
 * dev_scores and the size limit as there. */
int alink_smallres_score_features(alink_smallres_t* m, const float* dev_L, int nL, const float* dev_R, int nR, int col,
                                  float* dev_scores, void* stream);
/* one Keras train_on_batch (apply != 0) or gradients only.  dev_masks: the two dropout keep-masks for
 * the 2n tower passes, u8, laid out [2n*P1*P1*32] then [2n*P2*P2*64] (1 = keep), or NULL = no dropout.
 * dev_metrics: {loss, binary_accuracy}. */
int alink_smallres_train_step(alink_smallres_t* m, const float* dev_L, const float* dev_R, const float* dev_y,
                              const float* dev_sw, int n, int prescale, const uint8_t* dev_masks,
                              float grad_scale, int apply, float* dev_metrics, void* stream);
/* The same with the step's Dropout keep-masks drawn BY the step: dev_masks (2n (a + b) bytes, a and b from
 * alink_smallres_mask_sizes) is first filled with alink_keep_masks(dev_masks, 2n (a + b), 0.75, mask_seed) — by
 * extra workgroups of the step's first launch instead of a launch of its own — then read as above. */
int alink_smallres_train_step_drawn(alink_smallres_t* m, const float* dev_L, const float* dev_R, const float* dev_y,
                                    const float* dev_sw, int n, int prescale, uint8_t* dev_masks, uint64_t mask_seed,
                                    float grad_scale, int apply, float* dev_metrics, void* stream);
/* Keras train_on_batch (code/siamese.py:172-184 hands NumPy arrays) as ONE synchronous call on HOST operands: host_L / host_R
 * (n, H, W, 3) f32, host_y (n, 2), host_sw (n) or NULL.  The operands go through pinned staging owned by the handle (one
 * upload), the step draws its Dropout masks from mask_seed (dropout = 0: no Dropout), applies its update, the stream is
 * synchronised and {loss, accuracy} are returned in host_metrics[2]. */
int alink_smallres_train_on_batch_host(alink_smallres_t* m, const float* host_L, const float* host_R, const float* host_y,
                                       const float* host_sw, int n, int prescale, int dropout, uint64_t mask_seed,
                                       float* host_metrics, void* stream);
/* Optional (SmallResNet turns it on): on a non-default stream, the whole train step — ~40 short launches on two streams — is
 * captured per distinct (operand pointers, n, flags, lr) the second time it is seen and replayed from then on.  The caller keeps its
 * operands at stable addresses (staging buffers) for that to hit.  Same kernels, same order: the same results. */
int alink_smallres_set_graph(alink_smallres_t* m, int on);
int alink_smallres_apply_update(alink_smallres_t* m, void* stream);
int alink_smallres_eval(alink_smallres_t* m, const float* dev_L, const float* dev_R, const float* dev_y, int n,
                        int prescale, float* dev_metrics, void* stream);
/* EXTENSION (the FGSM / PGD noise of the Multi-PIE driver, which perturbs the pixels SmallRes reads): the gradient of the
 * inference loss (no Dropout) with respect to the pixels of both sides, dev_dL / dev_dR (n, H, W, 3) f32; with `prescale` it is
 * the gradient with respect to the raw 0..255 pixels (the first layer's factor 1/128 included).  dev_y (n, 2), dev_sw (n) or
 * NULL, n <= 256; grad_scale as in alink_smallres_train_step (<= 0: the Keras batch mean 1 / count(sw != 0); > 0 replaces
 * that factor — 1 gives every pair the gradient of its own loss).  dev_probs (optional): the (n, 2) outputs of the same forward.
 * CONTRACT: parameters and Adadelta state are untouched; the handle's activation and activation-gradient buffers and the
 * head's gradient buffer (alink_head_grads_dev) ARE overwritten — so never call it between a gradients-only step
 * (alink_smallres_train_step with apply = 0) and its alink_smallres_apply_update; and it is as thread-unsafe as every other
 * call on the handle.  No weight gradient is computed, nothing runs on the handle's side stream. */
int alink_smallres_input_grad(alink_smallres_t* m, const float* dev_L, const float* dev_R, const float* dev_y,
                              const float* dev_sw, int n, int prescale, float grad_scale, float* dev_dL, float* dev_dR,
                              float* dev_probs, void* stream);
/* sizes of the two dropout masks per tower image (elements): P1*P1*32 and P2*P2*64 */
int alink_smallres_mask_sizes(const alink_smallres_t* m, int* per_image_1, int* per_image_2);

/* ------------------------------------------------------------------------------------------------
 * Pool scoring helpers (HBM-bound): uncertainty measures (code/uncertainty.py:15-60) and top-k
 * (modAL multi_argmax as used at code/uncertainty.py:155,183,213; disparity top-k at
 * code/ALINK_arc.py:181).
 * ---------------------------------------------------------------------------------------------- */
#define ALINK_SCORE_UNCERTAINTY 0   /* 1 - max_c p                                  */
#define ALINK_SCORE_MARGIN      1   /* p_(1) - p_(2)                                */
#define ALINK_SCORE_ENTROPY     2   /* -sum p ln p (p renormalised)                 */
#define ALINK_SCORE_DISPARITY   3   /* -|a[:,col] - b[:,col]| (needs dev_b)         */
int alink_score(int kind, const float* dev_probs, const float* dev_b, int col, int64_t P, int C,
                float* dev_scores, void* stream);
/* Query-by-committee disagreement (modAL.disagreement, which the reference imports at code/learners.py:12 and names as
 * Committee's query strategies at code/learners.py:245,287) of n_members committee members over P pairs.
 * dev_member_probs: HOST array of n_members DEVICE pointers, member m's (P, C) float32 class probabilities (as
 * alink_committee_forward_multi takes its matrices).  Every output may be NULL; all requested outputs come from ONE pass
 * (one launch; the maximum-KL term reads each member's row a second time once the members' sum is complete).  Over pair
 * i, member m, class c, with M = n_members:
 *   votes[i][m]          = the first c that maximises p_m[i][c] (np.argmax); `>` comparisons, a NaN never wins.
 *   consensus[i][c]      = ((p_0 + p_1) + ... + p_{M-1}) / (float)M, in member order with one IEEE division: bit-equal to
 *                          what alink_committee_forward / _multi write for the same members.
 *   consensus_entropy[i] = -sum_c q ln q over the renormalised consensus, q > 0 terms only: bit-equal to
 *                          alink_score(ALINK_SCORE_ENTROPY) of the consensus.
 *   max_disagreement[i]  = max_m sum_c ph ln(ph M / s_c): ph = member m's row renormalised (ph > 0 terms only), s_c the
 *                          members' SUM, so the ratio is at most M (1 + rounding) and finite even where the divided mean
 *                          of denormal probabilities underflows to 0 (scipy.stats.entropy(pk, qk) per member, then the
 *                          maximum; the consensus is taken as it is: rows are probabilities, summing to 1 within rounding).
 *   vote_entropy[i]      = -sum_c (n_c / M) ln(n_c / M) over the vote counts n_c, computed as sum over v = 1 .. M ascending of
 *                          k_v t_v (k_v = classes holding v votes, t_v = -(v / M) logf(v / M)): a function of the MULTISET of
 *                          counts, so equal disagreement is an exact tie and alink_topk's lower-index rule decides it.
 * 1 <= n_members <= 64, 2 <= C <= 32 (else ALINK_EINVAL); P == 0 writes nothing; any P runs (the kernel strides). */
#define ALINK_DISAGREE_MAX_MEMBERS 64
#define ALINK_DISAGREE_MAX_CLASSES 32
int alink_committee_disagreement(const float* const* dev_member_probs, int n_members, int64_t P, int C,
                                 float* dev_vote_entropy,      /* (P)                                     */
                                 float* dev_consensus_entropy, /* (P)                                     */
                                 float* dev_max_disagreement,  /* (P)                                     */
                                 float* dev_consensus,         /* (P, C)                                  */
                                 int32_t* dev_votes,           /* (P, n_members): argmax class per member */
                                 void* stream);
/* indices of the k smallest (largest=0) or largest scores, ties broken by lower index, returned
 * sorted by (score, index).  dev_scratch >= alink_topk_scratch_bytes(P, k). */
size_t alink_topk_scratch_bytes(int64_t P, int k);
int alink_topk(const float* dev_scores, int64_t P, int k, int largest, int32_t* dev_idx,
               float* dev_vals, void* dev_scratch, void* stream);
/* Ranked batch-mode query selection (modAL.batch: Cardoso et al. 2017), the greedy rule that keeps a batch from filling with
 * near-duplicates: EXTENSION, no reference driver calls it.  N pool rows x_n of D floats, M labelled rows z_m (dev_labeled,
 * (M, D), always materialised), a utility u_n per pool row (larger = more informative), a batch of k (clipped to N).
 *   d2_n    = min over the labelled rows and the picks so far of |x_n - .|^2        (squared Euclidean distance)
 *   for pick t = 0 .. k - 1:
 *     alpha_t = (N - t) / (N + M)          |unlabelled| / (|unlabelled| + |labelled|), picks counting as labelled: the
 *                                          float32 of the float64 quotient; a caller's alpha in [0, 1] replaces it
 *     score_n = alpha_t (1 - 1 / (1 + sqrt(d2_n))) + (1 - alpha_t) u_n              for every row not yet picked
 *     pick_t  = argmax_n score_n, ties to the lower index;  d2_n = min(d2_n, |x_n - x_pick|^2)
 * dev_idx[t] = pick_t in order, dev_scores[t] = the score it had when picked.  `>` comparisons: a NaN score never wins, and
 * once nothing but NaN scores is left the remaining picks are -1.
 * Two row forms: dev_li == NULL: dev_x is the (N, D) row table (dev_r, dev_ri unused); otherwise row n is
 * |dev_x[dev_li[n]] - dev_r[dev_ri[n]]| formed on the fly from a left and a right feature table of D columns (the index form
 * of alink_head_forward; what the pair scorer sees, code/siamese.py:27-35) — the N x D rows are never materialised, and the
 * indices are NOT range-checked.
 * Arithmetic is pinned: float32; the D squared differences are summed by fused multiply-add in one fixed order that depends
 * on D alone (element e to lane (e / 4) % 64, ascending per lane, then an xor butterfly over the 64 lanes), the same in
 * both row forms, so both give the same bits; sqrt and the division are correctly rounded; the score is
 * fl(fl(alpha fl(1 - s)) + fl(fl(1 - alpha) u)) with s = fl(1 / fl(1 + fl(sqrt(d2)))), no product contracted into the sum.
 * The call enqueues 1 + k + 1 launches on `stream` and returns: no host synchronisation, nothing read back.
 * Limits (ALINK_EINVAL beyond): 1 <= N < 2^31, 1 <= D <= 8192 (the picked row is held in LDS), M >= 1 (the cold start — the
 * row nearest to all others — is alink_information_density's central row, made the one labelled row of this call by
 * batch.ranked_batch_cold_device: a-link_amd/batch.py), k >= 1, alpha <= 1 (alpha < 0: the schedule).
 * dev_scratch >= alink_ranked_batch_scratch_bytes(N, k), 256-byte aligned. */
size_t alink_ranked_batch_scratch_bytes(int64_t N, int k);
int alink_ranked_batch(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D,
                       const float* dev_labeled, int64_t M, const float* dev_utility, int k, float alpha, int32_t* dev_idx,
                       float* dev_scores, void* dev_scratch, void* stream);
/* Information density (modAL.density: Settles & Craven 2008) and the cold start of the ranked batch (modAL.batch's
 * select_cold_start_instance), Euclidean metric: EXTENSION, no reference driver calls it.  N pool rows x_n of D floats against
 * R reference rows z_j: dev_ref, a materialised (R, D) table, or — dev_ref == NULL, R == N — the pool itself; self-pairs
 * count, as in modAL (d = 0, s = 1).
 *   d_nj = sqrt(|x_n - z_j|^2),  s_nj = 1 / (1 + d_nj)
 *   dev_density[n]       = (sum_j s_nj) / R                 modAL's information_density when the pool is its own reference
 *   dev_mean_distance[n] = (sum_j d_nj) / R
 *   dev_central[0]       = argmin_n sum_j d_nj              the cold start's row; `<` comparisons, ties to the lower index, a
 *                                                           NaN sum never wins, -1 when nothing but NaN sums is left
 * Any of the three outputs may be NULL, not all.  The pool has the two row forms of alink_ranked_batch (dev_li == NULL: dev_x is
 * the (N, D) row table; otherwise row n is |dev_x[dev_li[n]] - dev_r[dev_ri[n]]|, formed on the fly, never materialised, the
 * indices NOT range-checked).
 * Arithmetic is pinned: |x_n - z_j|^2 is alink_ranked_batch's — float32, direct differences, one fused multiply-add per element
 * in the one order that depends on D alone (element e to lane (e / 4) % 64, ascending per lane, then an xor butterfly over the
 * 64 lanes; rows zero-padded), never |a|^2 + |b|^2 - 2ab — the same bits in both row forms; d = fl(sqrt(d2)) and
 * s = fl(1 / fl(1 + d)) in float32, both correctly rounded; a row's two sums are FLOAT64, sum_j (double)s and sum_j (double)d:
 * distances concentrate in high dimension, rows' densities then differ in their low digits, and a float32 sum of 200,000 terms
 * would throw those away.  The outputs are the float32 of the float64 quotient by (double)R; the argmin compares the float64 sums.
 * Summation order, a function of (R, D) alone — no atomics, so results are bit-reproducible from run to run: the reference rows
 * pass in tiles of T = 8192 / Dp rows in ascending order (Dp = D rounded up to a multiple of 4; T rounded down to a multiple
 * of 16 when above 16); a pool row has 16 partial sums, and the reference row at position p of its tile goes to partial c with
 * 4 (c & 3) + (c >> 2) == p % 16; a partial adds its terms in ascending reference order; after the last tile the 16 partials
 * meet in an xor butterfly (8, 4, 2, 1).
 * The call enqueues one launch, two when dev_central is given, on `stream` and returns: no host synchronisation, nothing read
 * back.  Limits (ALINK_EINVAL beyond, nothing launched): 1 <= N < 2^31, 1 <= R < 2^31 (R == N without dev_ref), 1 <= D <= 8192
 * (a reference row is held in LDS), at least one output.  dev_scratch is needed for dev_central only:
 * >= alink_information_density_scratch_bytes(N), 256-byte aligned.  Not here: other metrics (a-link_amd/density.py has them on
 * the host), several ranks' pools in one call. */
size_t alink_information_density_scratch_bytes(int64_t N);
int alink_information_density(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D,
                              const float* dev_ref, int64_t R,  /* NULL: the pool is its own reference, R == N */
                              float* dev_density,               /* (N) or NULL */
                              float* dev_mean_distance,         /* (N) or NULL */
                              int32_t* dev_central,             /* (1) or NULL */
                              void* dev_scratch, void* stream);
/* Expected gradient length (Settles, Craven & Ray 2008) and the last layer's gradient embedding (BADGE: Ash et al. 2020) of P
 * pairs through one head: EXTENSION, no reference driver calls it.  The pairs are alink_head_forward's (dev_li / dev_ri index
 * the two feature tables, NULL = identity; the indices are NOT range-checked).  For pair x let l_c(x) be the loss
 * alink_head_train_step computes on the batch {x} with target class c and sample weight 1, g_c(x) its gradient over all six
 * parameter tensors:
 *   dev_egl[p]   = sum over c in {0, 1} of P(c | x) |g_c(x)|_2      P(c | x) = the head's probability (out_dim 1: p and 1 - p)
 *   dev_probs[p] = alink_head_forward's probabilities, bit for bit
 *   dev_emb[p][c * h2 + j] = (p_c - [c == yhat]) a2[j]               yhat = argmax p, ties to class 0 (out_dim 1: p > 0.5);
 *                                                                    the last layer's weight gradient for the label yhat
 * No per-sample weight gradient is formed: with d = |l - r|, a1 = relu(z1), a2 = relu(z2),
 *   u = (W3[:,0] - W3[:,1]) . [z2 > 0], n3 = 2   (out_dim 1: u = W3[:,0] . [z2 > 0], n3 = 1),   v = (u W2^T) . [z1 > 0],
 *   G^2 = n3 (|a2|^2 + 1) + |u|^2 (|a1|^2 + 1) + |v|^2 (|d|^2 + 1),    egl = 2 p0 p1 sqrt(G^2)   (out_dim 1: 2 p (1 - p) sqrt(G^2)).
 * A row with an output outside [1e-7, 1 - 1e-7] has egl exactly 0 and a zero embedding: the loss clips there and the train
 * step's gradient is zero.  float32 throughout, one launch, every sum in an order fixed by the head's shape (no atomics): a
 * pair's outputs do not depend on P or on where the pair stands.
 * accumulate / final_div act on dev_egl only, as the committee mean's do on probabilities: accumulate adds to the value already
 * there, final_div > 0 divides the sum by it (one call per member, the last with final_div = the number of members).
 * P == 0 writes nothing.  ALINK_EINVAL, nothing launched: a NULL head or table, all three outputs NULL, P < 0 or above
 * 2^29 - 32, accumulate without dev_egl, a head in the bf16 compute mode (this is the exact form). */
int alink_head_egl(alink_head_t* h, const float* dev_L, const float* dev_R, const int32_t* dev_li, const int32_t* dev_ri, int64_t P,
                   int accumulate, float final_div,       /* committee mean, on dev_egl */
                   float* dev_egl,                         /* [P]            or NULL */
                   float* dev_probs,                       /* [P][od]        or NULL */
                   float* dev_emb,                         /* [P][od*h2]     or NULL */
                   void* stream);
/* ALFA-Mix (Parvaneh et al. 2022, "Active learning by feature mixing") through one head: does the head's decision for a pair
 * flip when its feature is pulled a short way towards an anchor (the mean labelled row of a class)?  EXTENSION, no reference
 * driver calls it.  The pairs are alink_head_forward's (dev_li / dev_ri index the two feature tables, NULL = identity; the
 * indices are NOT range-checked).  For pair p, d = |L[li[p]] - R[ri[p]]| in float32; z1, a1, z2, a2, z3, probs are exactly
 * alink_head_forward's; yhat is alink_head_egl's: out_dim 2, p1 > p0 ? 1 : 0; out_dim 1, p > 0.5.
 * Gradient:
 *   w = W3[:,0] - W3[:,1]  (out_dim 1: W3[:,0]),   u = w . [z2 > 0],   v = (u W2^T) . [z1 > 0]      (alink_head_egl's u and v)
 *   q = v W1^T  (D values): the input gradient of z3_0 - z3_1 (out_dim 1: of z3)
 *   g = the direction that lowers the predicted class's margin — the train loss's input gradient for the label yhat up to a
 *       positive factor; no clip enters, so saturated rows have a direction too:
 *       out_dim 2: g = q if yhat = 1, else -q;    out_dim 1: g = -q if yhat = 1, else q;    G = |g|_2
 * Mix, for anchor a of A (1 .. 8; dev_anchors is an (A, D) float32 table):
 *   z = anchor_a - d,   Z = |z|_2,   s = eps Z / G,   t_e = s g_e
 *   delta_e = min(max(t_e, min(z_e, 0)), max(z_e, 0)):  a step of length eps |z| along g, kept per element between the row and
 *       the anchor — the paper's alpha = eps |z| g / |g| (/) z clamped to [0, 1] and applied as d + alpha (.) z, without the
 *       division;  G == 0, or G or Z not finite: delta = 0
 *   mixed_a = d + delta
 * Second forward: the forward's arithmetic on the row mixed_a in place of |l - r| — the same packed weights, k order, layer-2
 * split, sum order and softmax expression — gives dev_mixed_probs[p][a][:]; bit a of dev_flip[p] is set when the argmax of
 * dev_mixed_probs[p][a] (the same tie rule) differs from yhat.  dev_probs are alink_head_forward's bits; dev_mixed are the
 * mixed rows themselves (tests and diagnostics: P x A x D floats).
 * float32 throughout, one launch, no atomics; every sum runs in an order fixed by (D, h1, h2, A) alone, and a pair's outputs
 * do not depend on P or on where the pair stands:
 *   q_e      one matrix-core chain over k = 0 .. h1 - 1 ascending, two k per instruction (the k order of layers 1 and 2)
 *   G^2, Z^2 over the D elements: share j of 8 adds the 8-element blocks j, j + 8, ... in ascending order, a block in ascending
 *            e, one fused multiply-add per element; the eight shares meet in an xor butterfly (1, 2, 4).  z_e = fl(anchor_e -
 *            d_e) is rounded before it is squared and is the z_e of the clamp.
 *   G = fl(sqrt(G^2)), Z = fl(sqrt(Z^2)), s = fl(fl(eps Z) / G), t_e = fl(s g_e), mixed_e = fl(d_e + delta_e)
 * P == 0 writes nothing.  ALINK_EINVAL, nothing launched and no output touched: a NULL head, table or anchors, all four
 * outputs NULL, P < 0 or above 2^29 - 32, A outside 1 .. 8, eps not finite or < 0, D not a multiple of 8 or above 512 (the mix
 * holds a whole row in LDS), h1 not in {128, 256, 384, 512}, a head in the bf16 compute mode (this is the exact form). */
int alink_head_feature_mix(alink_head_t* h, const float* dev_L, const float* dev_R, const int32_t* dev_li, const int32_t* dev_ri,
                           int64_t P, const float* dev_anchors, int A, float eps,
                           float* dev_probs,        /* [P][od]        or NULL */
                           uint8_t* dev_flip,       /* [P]            or NULL */
                           float* dev_mixed_probs,  /* [P][A][od]     or NULL */
                           float* dev_mixed,        /* [P][A][D]      or NULL: tests and diagnostics */
                           void* stream);
/* k-means++ seeding (Arthur & Vassilvitskii 2007) over N pool rows of D floats: the batch rule of BADGE (Ash et al. 2020) when
 * the rows are alink_head_egl's gradient embeddings.  EXTENSION, no reference driver calls it.  The pool has the two row forms of
 * alink_ranked_batch (dev_li == NULL: dev_x is the (N, D) row table; otherwise row n is |dev_x[dev_li[n]] - dev_r[dev_ri[n]]|,
 * formed on the fly, never materialised, the indices NOT range-checked).  k picks (clipped to N); dev_uniform: k float64 values
 * in [0, 1), entry 0 never read (so the stream does not depend on `first`); first: a row index, or -1 for the row of largest
 * squared norm.  This is the library's only SAMPLING rule, so every step of the draw is pinned:
 *   pick 0      first, or with first = -1 the argmax_n of |x_n|^2 — float32, the squared distance to the zero row in the order
 *               below; `>` comparisons, ties to the lower index, a NaN never enters; dev_idx[0] = -1 when no row has a norm that
 *               is a number (every later pick is then -1 with potential 0).  dev_potential[0] = NaN.
 *   distances   after pick p: d2_n = min(d2_n, |x_n - x_p|^2) (after pick 0: assigned) — float32, alink_ranked_batch's
 *               arithmetic: direct differences, one fused multiply-add per element, element e to lane (e / 4) % 64, ascending per
 *               lane, then an xor butterfly over the 64 lanes (rows zero-padded); the same bits in both row forms.  A picked row
 *               and every exact duplicate of it has d2 = 0 exactly.
 *   weights     w_n = (double)d2_n if 0 < d2_n < inf, else 0 (a NaN row weighs nothing).
 *   sums        C_n = sum over m <= n of w_m, T = C_(N-1), float64;  target = uniform[t] * T, one float64 product.
 *   pick t      the smallest n with w_n > 0 and C_n > target; if there is none (the product rounded up to T) the last row with
 *               w > 0.  dev_potential[t] = T, the k-means potential before the pick.
 *   exhaustion  T == 0 (fewer distinct rows than picks): pick t and every later pick are -1, their potential 0.
 * Every comparison is of a cumulative sum against the target, never of a partial sum against target - prefix (that subtraction
 * rounds).  The order of the float64 sums is a function of N alone — no atomics, so results are bit-identical from run to run:
 * rows are cut into contiguous chunks of c = 8 ceil(N / 16384) rows; a chunk's sum adds, for each of 4 interleaved row-pair
 * streams (rows 8 i + 2 v, 8 i + 2 v + 1 of the chunk in stream v), its weights in ascending order, then ((s0 + s1) + s2) + s3;
 * the chunk sums are accumulated in ascending chunk order (blocks of 8 chunks: the blocks' totals meet in a Hillis-Steele scan
 * over 64 blocks and an ascending sum over the 4 groups of 64, then each block adds its chunks one after another from the sum
 * of everything below it); inside the chosen chunk C_n = (that chunk's base + the totals of the 64-row segments before n's, one
 * after another) + a Hillis-Steele scan inside n's segment.  Where every w is an integer and T < 2^53 no sum rounds, and the
 * picks are those of np.cumsum / np.searchsorted(side="right") (a-link_amd/badge.py: kmeans_pp).
 * The call enqueues (first == -1 ? 1 : 0) + (k - 1) + 1 launches on `stream` and returns: no host synchronisation, nothing read
 * back.  ALINK_EINVAL, nothing launched and no output touched: a NULL argument, a pair form without dev_r / dev_ri, N outside
 * 1 .. 2^31 - 1, D outside 1 .. 8192 (the picked row is held in LDS), k < 1, first outside -1 .. N - 1, dev_scratch not 256-byte
 * aligned.  dev_scratch >= alink_kmeanspp_scratch_bytes(N, k).  Not here: several ranks' pools in one call, labelled rows as
 * centres that exist before the first pick, fusing the embedding into the distance pass. */
size_t alink_kmeanspp_scratch_bytes(int64_t N, int k);
int alink_kmeanspp(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D,
                   const double* dev_uniform, int64_t first, int k,
                   int32_t* dev_idx,                       /* (k) picks in order, -1 = none */
                   double* dev_potential,                  /* (k) T before each pick; [0] = NaN */
                   void* dev_scratch, void* stream);
/* EXTENSION — BAIT (Ash, Goel, Krishnamurthy & Kakade 2021): a batch chosen by the Fisher information it adds.
 * Greedy forward selection of over x k rows, each the row that most reduces tr(M^-1 Phi), then a backward prune to k.  No
 * reference driver calls it.  For the pair head the last layer's per-label gradients are collinear (two outputs: grad l(x, 0) =
 * p1 s, grad l(x, 1) = -p0 s with s = [-a2 ; a2]), the per-sample Fisher is the rank-one p0 p1 s s^T, and BAIT over the 2 h2
 * dimensions with the paper's rank-two trace expression equals BAIT over F = h2 dimensions with ONE factor row per sample and
 * the same ridge (DESIGN.md §9 derives it).  The pinned rule:
 *   factor   f is (P, F = h2) from alink_head_egl's dev_probs and dev_emb; yhat is alink_head_egl's, c* the other class.
 *            Two outputs: f_nj = emb[n, c* h2 + j] * (float)sqrt(2 p_yhat / p_c*), the scale in float64 from the float32
 *            probabilities, rounded once (= sqrt(2 p0 p1) a2).  One output: f_nj = |emb[n, j]| * (float)(sqrt(p (1 - p)) /
 *            |p - [p > 0.5]|) (= sqrt(p (1 - p)) a2).  A row with an output outside [1e-7, 1 - 1e-7] (float32 comparisons,
 *            alink_head_egl's; its emb is zero already) has f = 0.  The bias column is not part of the Fisher.
 *   blocks   a row may carry m factors side by side, a table (N, m F): independent committee members give a block-diagonal
 *            Fisher, and the score is the sum of the members' scores, each against its own A, B.  m = 1 is plain BAIT.
 *            Limits: F a multiple of 8, 8 <= F <= 128, 1 <= m <= 8, m F <= 512.
 *   Gram     Phi_j = (1 / N_all) sum over pool + labelled of f_j f_j^T, M0_j = lambda I + sum over the labelled of f_j f_j^T and
 *            B0 = M0^-1 are the caller's (float64, host: a-link_amd/bait.py forms them from a read-back of the factor rows).
 *   score    alink_bait_scores: per block q_A = f^T A f, q_B = f^T B f against float32 images of A = B Phi B and B.  g = f A:
 *            float32, one fused multiply-add per k from 0, k ascending (an MFMA accumulator); q = sum over columns c of g_c f_c:
 *            lane (c % 32) adds its columns c, c + 32, ... by fused multiply-add from 0 in ascending order, the 32 lanes meet in
 *            an xor butterfly (16, 8, 4, 2, 1; F < 32: the missing lanes hold 0).  sign = +1: term = q_A / (1 + q_B); sign = -1:
 *            term = q_A / (q_B - 1), and a row with any q_B >= 1 is skipped (its score is NaN).  score = the blocks' terms added
 *            in ascending order, float32, correctly rounded division.  A row's score is a function of (A, B, f_n) alone: not of N,
 *            its tile, or its place in the tile.  dev_scores (N) or NULL.  dev_partial_best: ceil(N / ALINK_BAIT_TILE) pairs
 *            (float score, int32 index), per tile of ALINK_BAIT_TILE rows the free row (dev_free[n] != 0) of largest score, ties
 *            to the lower index, a NaN never wins; (-inf, 2^31 - 1) for a tile without one.  dev_AB: per block the image of A
 *            then the image of B, element (k, c) of a matrix at ((k / 8) F + c) 8 + (k % 2) 4 + (k % 8) / 2.  One launch.
 *   forward  alink_bait_select, t = 0 .. k_forward - 1: one score launch (sign +1), then one launch of one workgroup that
 *            takes the best of the partial maxima (-1 when there is none: nothing changes then), records it, clears its free
 *            byte and, per block in float64: w = B f (w_i = sum over k ascending of B[k][i] f_k, fused multiply-adds from 0:
 *            B is symmetric and row k stands for column k), c = 1 + f^T w, B[i][j] -= (w_i w_j) / c; then C = Phi B and
 *            A = B C, both as Z[i][j] = sum over k ascending of X[k][i] Y[k][j] by fused multiply-add from 0 (A is RECOMPUTED,
 *            a function of (B, Phi) alone), and the float32 images of A and B.  dev_Phi and dev_B must be symmetric.
 *   backward while more than k_keep picks are kept: the same two launches with sign -1 over a table of the picked rows: remove
 *            the kept row of largest score q_A / (q_B - 1) summed over blocks, ties to the earlier pick; B[i][j] -= (w_i w_j)
 *            / (f^T w - 1)  (= B + w w^T / (1 - f^T w)).  If every kept row is skipped nothing more is removed, and the first
 *            k_keep kept picks are returned.  Result: the kept picks in the order they were picked with their forward scores
 *            (-1 / NaN beyond them); dev_free is 0 exactly on the rows returned and the rows it was 0 on before.
 *   Deliberately not the authors' code: no nLabeled / (nLabeled + K) rescaling of M0; deterministic ties.
 * alink_bait_select enqueues 1 + 2 k_forward (+ 2 + 2 (k_forward - k_keep) when k_keep < k_forward) launches on `stream` and
 * returns: no host synchronisation, no data-dependent loop, no atomics, no workgroup waits on another.  With k_keep == k_forward
 * there is no prune and dev_B comes back: k1 + k2 forward picks equal two chained calls bit for bit.  Results are bit-identical
 * from run to run.  ALINK_EINVAL, nothing launched: a NULL argument (dev_scores may be NULL), N outside
 * 1 .. 2^31 - 1, F / m outside the limits, sign not +-1, od not 1 or 2, k_keep < 1 or k_forward < k_keep or k_forward > N, a row
 * table or dev_AB not 16-byte aligned, dev_scratch not 256-byte aligned.  Not built: the Gram matrices on the device; per-sample rank above one; an incrementally
 * updated score (q' = q - (f . w)^2 / c ...), which would make a row's float32 score depend on the pick history. */
#define ALINK_BAIT_TILE 128   /* rows per tile of alink_bait_scores' partial maxima */
int alink_fisher_factor(const float* dev_probs, const float* dev_emb, int64_t P, int od, int h2, float* dev_f /* (P, h2) */, void* stream);
int alink_bait_scores(const float* dev_f, int64_t N, int F, int m, const float* dev_AB, const uint8_t* dev_free, int sign,
                      float* dev_scores, void* dev_partial_best, void* stream);
size_t alink_bait_select_scratch_bytes(int64_t N, int F, int m, int k_forward);
int alink_bait_select(const float* dev_f, int64_t N, int F, int m, const double* dev_Phi /* (m, F, F) */,
                      double* dev_B /* (m, F, F) in / out */, uint8_t* dev_free /* (N) in / out */, int k_forward, int k_keep,
                      int32_t* dev_idx /* (k_keep) */, float* dev_score /* (k_keep) */, void* dev_scratch, void* stream);
/* EXTENSION — Lloyd's k-means of a pool on the device: T iterations from given centres, the engine of k-means
 * sampling and of the diverse mini-batch (a-link_amd/cluster.py).  The pool as alink_kmeanspp takes it: an (N, D) row table dev_x
 * (dev_li == NULL), or row n = |dev_x[dev_li[n]] - dev_r[dev_ri[n]]| formed on the fly.  dev_weight: (N) float32 or NULL (every
 * weight 1); a weight that is not finite and > 0 counts as 0.  dev_centres: (K, D) float32, in: C_0, out: C_T.  The rule:
 *   assignment  against centres C:  dot(n, j) = x_n . c_j — float32, ONE fused multiply-add per element from 0 in ascending
 *               element order e = 0 .. D - 1 (what one MFMA accumulator gives: the order is a function of D alone, not of N, K, the
 *               tile a row or centre falls in, 16-byte or 4-byte loads, or the row form);  cn_j = |c_j|^2 — float32, the squared
 *               distance of c_j to the zero row in alink_ranked_batch's order (element e to lane (e / 4) % 64, one fused
 *               multiply-add each, ascending per lane, an xor butterfly over the 64 lanes);  score(n, j) = fmaf(-2, dot(n, j), cn_j),
 *               one rounding.  a_n = the j of least score by `<` from +inf: ties go to the lower j; a score that is NaN or +inf never
 *               wins, so a centre with a non-finite element never takes a row and is left as it is, and a row no centre wins (a NaN
 *               row) has a_n = -1 and d2_n = NaN and is left out of every sum and count.
 *   distance    d2_n = |x_n - c_(a_n)|^2 for the assigned centre only — float32, direct differences in alink_ranked_batch's order
 *               above: never negative, and comparable with the other strategies' distances.
 *   update      c_j <- (float)(sum over a_n = j of w_n x_n / sum over a_n = j of w_n): both sums float64 (a product w_n x_n is exact
 *               in float64), one float64 division, one rounding.  Rows of weight 0 are left out; a cluster whose weight sum is 0
 *               keeps its centre.  Order: rows are cut into S slices of L = 256 ceil(ceil(N / S') / 256) rows, S' = 1 for
 *               K >= 2048, else min(64, ceil(4096 / K)), S = ceil(N / L); a slice adds its rows of cluster j in ascending row order,
 *               the slices' sums are added in ascending order from 0.
 *   schedule    for t = 0 .. iters - 1: assign against C_t, update to C_(t+1); then one last assignment against C_iters.
 * Outputs, any but dev_assign NULL: dev_assign (N) int32 and dev_d2 (N) float32 of the last assignment; dev_inertia (iters + 1)
 * float64, the sum of w_n d2_n over the rows with a_n >= 0 and w_n > 0 of each assignment (rows are cut into contiguous chunks of
 * c = 8 ceil(N / 16384); a chunk adds, for each of 4 interleaved row-pair streams, its terms in ascending order, then
 * ((s0 + s1) + s2) + s3; eight neighbouring chunks are added in ascending order from 0, then those totals in ascending order);
 * dev_changed (iters + 1) int32, the rows whose a_n differs from the pass before (before the first pass every row counts as -1):
 * a pass with changed = 0 is an exact fixed point, and every later pass repeats it; dev_counts (K) int32 rows and dev_wsum (K)
 * float64 weight (the update's order) of each cluster of the last assignment; dev_nearest (K) int32, the row of each final cluster
 * with the least d2, ties to the lower row, -1 for a cluster without rows.
 * Where rows, centres and weights are small integers nothing rounds, and everything equals a-link_amd/cluster.py: kmeans (host
 * float64) bit for bit.  Results are bit-identical from run to run: no floating-point atomics.  The call enqueues at most 6
 * launches per pass on `stream` and returns: no host synchronisation, nothing read back.  The (N x K) scores never exist in
 * memory.  ALINK_EINVAL, nothing launched and no output touched: dev_x, dev_centres, dev_assign or dev_scratch NULL, a pair form
 * without dev_r / dev_ri, N outside 1 .. 2^31 - 1, D outside 1 .. 8192, K outside 1 .. 8192, iters < 0, dev_scratch not 256-byte
 * aligned.  dev_scratch >= alink_kmeans_scratch_bytes(N, D, K) (0 for sizes the call refuses).  Not here: several ranks' pools in
 * one call, a cosine metric, relocating empty clusters, mini-batch k-means, an early return once changed = 0. */
size_t alink_kmeans_scratch_bytes(int64_t N, int D, int K);
int alink_kmeans(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D,
                 const float* dev_weight, float* dev_centres, int K, int iters,
                 int32_t* dev_assign, float* dev_d2, double* dev_inertia, int32_t* dev_changed,
                 int32_t* dev_counts, double* dev_wsum, int32_t* dev_nearest,
                 void* dev_scratch, void* stream);
/* EXTENSION — the K nearest neighbours of every pool row among the pool's other rows, their squared distances
 * and the typicality of TypiClust (Hacohen, Dekel & Weinshall 2022; a-link_amd/typiclust.py).  The pool as alink_kmeans takes it: an
 * (N, D) row table dev_x (dev_li == NULL), or row n = |dev_x[dev_li[n]] - dev_r[dev_ri[n]]| formed on the fly.  dev_group: (N) int32
 * or NULL (every row in group 0).  The rule:
 *   candidates  of row n: every j != n of the same group.  A row of group < 0 has no neighbours and is nobody's neighbour, and so
 *               has a row whose |x|^2 (below) is NaN or +inf.  Duplicate rows are neighbours at distance 0.  Passing alink_kmeans'
 *               dev_assign as dev_group makes "the neighbours inside a row's own cluster" one call.
 *   score       dot(n, j) = x_n . x_j — float32, ONE fused multiply-add per element from 0 in ascending element order e = 0 .. D - 1,
 *               the chain of alink_kmeans (what one MFMA accumulator gives: a function of D alone);  xn_j = |x_j|^2 — float32, the
 *               squared distance of x_j to the zero row in alink_ranked_batch's order (element e to lane (e / 4) % 64, one fused
 *               multiply-add each, ascending per lane, an xor butterfly over the 64 lanes);  score(n, j) = fmaf(-2, dot(n, j), xn_j),
 *               one rounding.  A score that is NaN or +inf never enters a list.
 *   list        row n's neighbours are the K candidates of least (score, index) in lexicographic order, written in that order: ties
 *               go to the lower index.  dev_found[n] = how many there are (<= K); unfilled slots hold index -1 and d2 = NaN.
 *   distance    d2(n, slot) = |x_n - x_j|^2 for the K winners only — float32, direct differences in alink_ranked_batch's order
 *               above: never negative, and the number the ranked batch, information density, k-means++ and k-means report.  The
 *               ORDER of a list is the score's, not d2's: score(n, j) + |x_n|^2 and d2 round differently, so two neighbours whose
 *               distances agree to the last bits may stand in d2's reverse order.
 *   typicality  m_n = (float64 sum over the found slots, in ascending slot order, of sqrt((double)d2)) / found;
 *               dev_typicality[n] = (float)(1 / (m_n + eps)); 0 for a row with found = 0.  With squared != 0 the term is
 *               (double)d2 itself: what the public TypiClust code computes, whose index returns squared distances.
 * Where the rows are small integers nothing rounds, and idx, d2 and found equal a-link_amd/typiclust.py: knn (host float64) bit
 * for bit.  Results are bit-identical from run to run.  dev_idx (N, K) int32 is required; dev_d2 (N, K) float32, dev_found (N) int32
 * and dev_typicality (N) float32 may each be NULL.  The call enqueues at most 3 launches on `stream` and returns: no host
 * synchronisation, no cooperative launch, no grid barrier, no atomics, nothing read back; the (N x N) scores never exist in memory.
 * ALINK_EINVAL, nothing launched and no output touched: dev_x, dev_idx or dev_scratch NULL, a pair form without dev_r / dev_ri,
 * N outside 1 .. 2^31 - 1, D outside 1 .. 8192, K outside 1 .. 32, dev_scratch not 256-byte aligned.  dev_scratch >=
 * alink_knn_scratch_bytes(N, D, K) (0 for sizes the call refuses).  Queries against a separate reference set: alink_knn_rect
 * below.  Not here: K > 32, a cosine metric, several ranks' pools in one call, skipping candidate tiles that hold no row of a
 * workgroup's groups (every workgroup walks the whole pool, with or without dev_group). */
size_t alink_knn_scratch_bytes(int64_t N, int D, int K);
int alink_knn(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D,
              const int32_t* dev_group, int K, int squared, double eps,
              int32_t* dev_idx,                            /* (N, K) */
              float* dev_d2,                               /* (N, K) or NULL */
              int32_t* dev_found,                          /* (N) or NULL */
              float* dev_typicality,                       /* (N) or NULL */
              void* dev_scratch, void* stream);
/* EXTENSION (X12) — per group, the row of the largest value: dev_best[g], g = 0 .. G - 1, = the row n with dev_group[n] == g whose
 * dev_value[n] is largest by `>` from -inf; ties go to the lower row; NaN and -inf never win; a group without a winner gets -1;
 * rows whose group is outside 0 .. G - 1 are ignored.  Rows are cut into S slices of L = 256 ceil(ceil(N / S') / 256) rows,
 * S' = 1 for G >= 2048, else min(64, ceil(4096 / G)), S = ceil(N / L); a wave scans one slice for one group in ascending row order,
 * the slices' winners are combined in ascending order: no atomics, bit-identical from run to run.  Two launches on `stream`, no
 * host synchronisation.  ALINK_EINVAL, nothing launched: a NULL argument, N outside 1 .. 2^31 - 1, G outside 1 .. 8192, dev_scratch
 * not 256-byte aligned.  dev_scratch >= alink_group_argmax_scratch_bytes(N, G) (0 for sizes the call refuses). */
size_t alink_group_argmax_scratch_bytes(int64_t N, int G);
int alink_group_argmax(const float* dev_value, const int32_t* dev_group, int64_t N, int G,
                       int32_t* dev_best,                  /* (G) */
                       void* dev_scratch, void* stream);
/* EXTENSION — the K nearest rows of a separate REFERENCE set for every QUERY row (the rectangular form of
 * alink_knn), and the score of Contrastive Active Learning over such lists (Margatina, Vernikos, Barrault & Aletras 2021;
 * a-link_amd/cal.py).  Queries (N rows) and references (M rows) are each given as alink_knn takes a pool: an (., D) row table
 * (the li pointer NULL), or row n = |x[li[n]] - r[ri[n]]| formed on the fly.  ONE form holds for both sides of a call — both
 * tables or both pair forms; in the pair form the two sides may share tables or bring their own.  A mixed call is refused: the
 * caller can materialise the smaller side.  16-byte loads are used only when D % 4 == 0 and every table pointer of both sides is
 * 16-byte aligned.  The rule:
 *   score       dot(n, j) = q_n . c_j — float32, ONE fused multiply-add per element from 0 in ascending element order
 *               e = 0 .. D - 1, the chain of alink_kmeans / alink_knn (what one MFMA accumulator gives: a function of D alone);
 *               cn_j = |c_j|^2 — float32, the squared distance of c_j to the zero row in alink_ranked_batch's order, exactly as
 *               alink_knn's xn_j;  score(n, j) = fmaf(-2, dot(n, j), cn_j), one rounding.
 *   candidates  of query n: every reference — there is no self-exclusion, the sets are different, and there are no groups.  A
 *               reference whose cn_j is NaN or +inf is nobody's neighbour; a query whose own |q_n|^2 (the same order) is NaN or
 *               +inf has no neighbours; a score that is NaN or +inf never enters a list.
 *   list        query n's neighbours are the K references of least (score, index) in lexicographic order, written in that order:
 *               ties go to the lower reference index.  dev_found[n] = how many there are (<= min(K, M)); unfilled slots hold
 *               index -1 and d2 = NaN.
 *   distance    d2(n, slot) = |q_n - c_j|^2 for the K winners only — float32, direct differences in alink_ranked_batch's order.
 *               The ORDER of a list is the score's, not d2's (see alink_knn).
 * Where the rows are small integers nothing rounds, and idx, d2 and found equal a-link_amd/cal.py: knn_rect (host float64) bit
 * for bit.  Results are bit-identical from run to run.  dev_idx (N, K) int32, indices into the references, is required; dev_d2
 * (N, K) float32 and dev_found (N) int32 may each be NULL.  The call enqueues at most 4 launches on `stream` (the two norm passes,
 * the list pass, the distance pass) and returns: no host synchronisation, no cooperative launch, no grid barrier, no atomics,
 * nothing read back; the (N x M) scores never exist in memory.  A workgroup owns 128 queries and walks all M references, so
 * ceil(N / 128) workgroups run.  ALINK_EINVAL, nothing launched and no output touched: dev_qx, dev_cx, dev_idx or dev_scratch
 * NULL, a pair form without its r / ri, mixed forms, N or M outside 1 .. 2^31 - 1, D outside 1 .. 8192, K outside 1 .. 32,
 * dev_scratch not 256-byte aligned.  dev_scratch >= alink_knn_rect_scratch_bytes(N, M, D, K) (0 for sizes the call refuses).
 * Not here: splitting the references over workgroups (a handful of queries against a huge gallery), K > 32, groups, a cosine
 * metric, several ranks' pools in one call.
 * alink_cal_score — dev_score[n] = the mean over query n's found neighbours of KL(neighbour || query), the direction of the
 * authors' code.  dev_p (N, C) float32, the queries' probabilities; dev_q (M, C) float32, the references'; dev_idx (N, K) as
 * alink_knn_rect writes it.  All arithmetic is float64 from the float32 inputs, every product and sum rounded once:
 *   p'_c  = p[n, c] if p[n, c] > 2^-126, else 2^-126
 *   kl(j) = sum over c ascending, from 0, of q[j, c] * (log(q[j, c]) - log(p'_c)) — over the c with q[j, c] > 0 only
 *   score = (sum over the slots ascending, from 0, of kl(idx[n, slot]) — over the slots with 0 <= idx < M only) / found,
 * found = the number of those slots; dev_score[n] = (float)score, 0 for a query with found = 0.  The floor on p' keeps the score
 * finite where a float32 softmax has saturated to exactly 0 (the public code works on log-softmax outputs and cannot meet one).
 * An index >= M in dev_idx is the caller's error: such a slot is skipped like an unfilled one, the references are never read
 * through it.  One launch, one thread per query, no atomics, nothing read back.  ALINK_EINVAL, nothing launched: a NULL pointer,
 * N or M outside 1 .. 2^31 - 1, K outside 1 .. 32, C outside 1 .. 32. */
size_t alink_knn_rect_scratch_bytes(int64_t N, int64_t M, int D, int K);
int alink_knn_rect(const float* dev_qx, const float* dev_qr, const int32_t* dev_qli, const int32_t* dev_qri, int64_t N,
                   const float* dev_cx, const float* dev_cr, const int32_t* dev_cli, const int32_t* dev_cri, int64_t M,
                   int D, int K,
                   int32_t* dev_idx,                       /* (N, K) indices into the references, required */
                   float* dev_d2,                          /* (N, K) or NULL */
                   int32_t* dev_found,                     /* (N) or NULL */
                   void* dev_scratch, void* stream);
int alink_cal_score(const float* dev_p,                    /* (N, C) the queries' probabilities */
                    const float* dev_q,                    /* (M, C) the references' probabilities */
                    int C, const int32_t* dev_idx, int64_t N, int64_t M, int K,
                    float* dev_score,                      /* (N) */
                    void* stream);
/* EXTENSION — the fixed-radius neighbour graph of a pool and the greedy maximum coverage over it: ProbCover
 * (Yehuda, Dekel, Hacohen & Weinshall 2022, "Active Learning Through a Covering Lens"; a-link_amd/probcover.py).  The pool as
 * alink_knn takes it: an (N, D) row table dev_x (dev_li == NULL), or row n = |dev_x[dev_li[n]] - dev_r[dev_ri[n]]| formed on the
 * fly.  dev_group: (N) int32 or NULL (every row in group 0).  The rule:
 *   eligible    a row whose group is >= 0 and whose |x|^2 (below) is finite.  A row that is not eligible has no ball, lies in
 *               nobody's ball, is never covered and is never picked.
 *   score       dot(n, j) = x_n . x_j — float32, ONE fused multiply-add per element from 0 in ascending element order
 *               e = 0 .. D - 1, the chain of alink_kmeans / alink_knn (what one MFMA accumulator gives: a function of D alone, and
 *               symmetric in (n, j) because each product is);  xn_j = |x_j|^2 — float32, the squared distance of x_j to the zero
 *               row in alink_ranked_batch's order (alink_knn's value);  t(n, j) = fmaf(-2, dot(n, j), xn_n + xn_j): one float32
 *               addition, which commutes, then one fused rounding — t(n, j) and t(j, n) are the same bits.
 *   edge        j is in ball(n) when both rows are eligible and t(n, j) < radius2 — strict, as in the paper's code — or j == n: an
 *               eligible row is always in its own ball.  The decision is symmetric: n covers j exactly when j covers n.  Groups
 *               do not limit a ball: it holds rows of every group.  radius2 = delta^2 is a float32 the caller passes.
 *   purity      t_other(n) = the least t(n, j) over eligible j of a DIFFERENT group than n's, by `<` from +inf: ties go to the
 *               lower j; j_other(n) = that j, -1 (and t_other = +inf) where there is none or n is not eligible.  A ball of
 *               radius^2 r2 round n is impure exactly when t_other(n) < r2, so ONE pass gives the whole purity curve; it does not
 *               depend on the radius2 of the call.
 *   graph       CSR: offsets int64 (N + 1), the exclusive prefix sum of the degrees (the caller forms it); nbr int32 (E), each
 *               row's neighbours in ascending index order.
 * alink_ball_count writes dev_deg (N) int32, the size of every ball (0 for a row that is not eligible), dev_t_other (N) float32 and
 * dev_j_other (N) int32.  Each may be NULL, not all three; dev_t_other / dev_j_other need dev_group.  Two launches.
 * alink_ball_fill makes the same pass and the same decisions bit for bit (one device function forms the score and decides the
 * edge in both) and writes dev_nbr (E) int32: row n's neighbours at dev_offsets[n] .. dev_offsets[n + 1] - 1, ascending, every slot
 * once, without atomics (per 32 candidates the two lanes of a row OR their decision masks; a lane writes candidate c at
 * offsets[n] + base + popc(mask below c)).  A row never writes at or past dev_offsets[n + 1] nor outside [0, E): such a write is
 * dropped.  dev_mismatch (1) int32 = the number of rows whose ball did not exactly fill their span — 0 whenever the offsets are
 * the prefix sum of alink_ball_count's degrees for the same arguments; written by plain stores from a final one-workgroup launch.
 * Three launches.  Both: dev_scratch >= alink_ball_scratch_bytes(N, D) (0 for sizes the calls refuse); where the rows are small
 * integers nothing rounds, and everything equals a-link_amd/probcover.py: ball_graph / nearest_other (host float64) bit for bit.
 * alink_max_coverage — greedy maximum coverage over such a graph.  dev_covered (N) uint8, in: rows covered already (nonzero),
 * out: after the last pick.  First every row of ball(s) of every seed s in dev_seed (S, int32; NULL with S = 0; a seed outside
 * 0 .. N - 1 is ignored) is covered — the labelled rows.  Then for t = 0 .. k - 1: degree_t(u) = the number of v in ball(u) not
 * covered; the pick is the u of largest degree by `>` from 0, ties to the lower u; dev_picks[t] = u, dev_gain[t] = its degree;
 * every row of ball(u) is covered.  If the largest degree is 0 the pick is -1 with gain 0, and so is every later one: an
 * uncovered eligible row counts itself, so this means the pool is covered.  Launches: one for the seeds, two per pick — a recount
 * (rows in contiguous chunks of 64, a wave striding a row's span of nbr, each chunk writing its (largest degree, lowest row)) and
 * a pick (ONE workgroup combines the chunks in ascending order, writes pick and gain, marks ball(pick) with plain byte stores
 * of 1).  Recounting streams the E edges per pick (alink_ranked_batch streams the pool per pick).  A neighbour outside
 * 0 .. N - 1 is neither counted nor marked.  dev_scratch >= alink_max_coverage_scratch_bytes(N, k).
 * All three calls enqueue on `stream` and return: the stream's order is the only ordering between workgroups — no cooperative
 * launch, no grid barrier, no atomics, nothing read back, no host synchronisation; results are bit-identical from run to run;
 * the (N x N) scores never exist in memory.  ALINK_EINVAL, nothing launched and no output touched: a NULL required argument
 * (dev_x, dev_scratch; every output of the count; dev_offsets, dev_nbr, dev_mismatch of the fill; dev_offsets, dev_nbr,
 * dev_covered, dev_picks, dev_gain of the greedy; dev_seed with S > 0), dev_t_other / dev_j_other without dev_group, a pair form
 * without dev_r / dev_ri, N outside 1 .. 2^31 - 1, D outside 1 .. 8192, radius2 not finite or <= 0, E < 0, k < 1, S < 0, dev_scratch
 * not 256-byte aligned.  Not here: distances stored with the edges, skipping tiles by a spatial bound (every workgroup walks the
 * whole pool), an incremental-degree greedy, a cosine metric, balls round a separate set of centres (alink_knn_rect has the
 * rectangular product; a ball form of it does not exist), several ranks' pools in one call. */
size_t alink_ball_scratch_bytes(int64_t N, int D);
int alink_ball_count(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D,
                     const int32_t* dev_group, float radius2,
                     int32_t* dev_deg,                     /* (N) or NULL */
                     float* dev_t_other,                   /* (N) or NULL */
                     int32_t* dev_j_other,                 /* (N) or NULL */
                     void* dev_scratch, void* stream);
int alink_ball_fill(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D,
                    const int32_t* dev_group, float radius2, const int64_t* dev_offsets, int64_t E,
                    int32_t* dev_nbr,                      /* (E) */
                    int32_t* dev_mismatch,                 /* (1) */
                    void* dev_scratch, void* stream);
size_t alink_max_coverage_scratch_bytes(int64_t N, int k);
int alink_max_coverage(const int64_t* dev_offsets, const int32_t* dev_nbr, int64_t N, const int32_t* dev_seed, int64_t S, int k,
                       uint8_t* dev_covered,               /* (N) in / out */
                       int32_t* dev_picks,                 /* (k) picks in order, -1 = the pool is covered */
                       int32_t* dev_gain,                  /* (k) */
                       void* dev_scratch, void* stream);
/* EXTENSION — facility-location batches: the k rows of a pool that minimise sum_n min_(s in S) |x_n - x_s|^2,
 * by the greedy of largest gain, plain or stochastic (Mirzasoleiman et al. 2015, "Lazier Than Lazy Greedy"): the selection rule of
 * FASS (Wei, Iyer & Bilmes 2015, "Submodularity in Data Subset Selection and Active Learning"), of CRAIG's coresets and of the
 * SIMILAR family (a-link_amd/facility.py).  The pool as alink_knn takes it: an (N, D) row table dev_x (dev_li == NULL), or row
 * n = |dev_x[dev_li[n]] - dev_r[dev_ri[n]]| formed on the fly.  The rule:
 *   score       dot(n, j) = x_n . x_j — float32, ONE fused multiply-add per element from 0 in ascending element order, the chain
 *               of alink_kmeans / alink_knn;  xn_j = |x_j|^2 — float32, alink_knn's value;  t(n, j) = fmaf(-2, dot(n, j),
 *               xn_n + xn_j), the same bits as alink_ball_count's and the same for (n, j) and (j, n);  w(n, j) = 0 if t < 0, else
 *               t: a NaN stays NaN.  There is no self-exemption: w(p, p) is whatever the formula gives.
 *   term        term(n, c) = d if d > 0, else 0, with d = cur_n - w(n, c) as ONE float32 subtraction: a NaN on either side gives
 *               0.  A row whose xn is not finite gives 0 to every candidate.  dev_cur (N) float32 is the caller's: each row's
 *               squared distance to its nearest facility so far.
 *   gain        gain(c) = sum_n term(n, c) in float64, in an order that is a function of (N, R) alone: the pool is cut into S
 *               contiguous slabs of rows (S and the slab length, a multiple of 128, functions of (N, R)); within a slab a
 *               candidate's terms are added in a fixed order by two lanes whose sums meet once; the slabs' partials are added in
 *               ascending order.  Bit-identical from run to run, exact wherever the terms are integers.  Candidate position r
 *               names row dev_cand[r] (int32; dev_cand NULL: row r, and then R must equal N).  A candidate index outside
 *               0 .. N - 1, or a candidate whose xn is not finite, has gain 0.
 *   pick        the candidate POSITION of largest gain wins, by `>` from 0: ties go to the lower position in the candidate list;
 *               pick = dev_cand[position].  If no gain is > 0 the pick is -1 with gain 0, cur is unchanged and later steps go on:
 *               a later sample may still gain.
 *   cover       cur_n <- w(n, s) where w(n, s) < cur_n — strict, so a NaN never enters and a NaN cur_n stays — for every s of an
 *               index list.  An s outside 0 .. N - 1 (-1 among them), or whose xn is not finite, is ignored; a row whose xn is
 *               not finite keeps its cur.  The gains and the cover pass form w in one device function, and the chain and the
 *               addition commute: after a pick p, cur_p <= w(p, p) bit for bit, so p's gain is exactly 0 in every later step; a
 *               labelled row covered before the first pick is never picked either.
 * alink_facility_gains writes dev_gain (R) float64: three launches (norms, the gains pass over a grid of ceil(R / 128) candidate
 * tiles x S slabs whose workgroups write partial gains to scratch with plain stores, the sum of the slabs).  alink_facility_cover
 * updates dev_cur in place for the S rows of dev_sel (int32): two launches; S = 0 launches nothing.  alink_facility_select runs k
 * picks: one norm pass, then per pick t three launches — the gains pass over the candidates dev_cand + t R (dev_cand (k, R) int32,
 * one list per step; NULL: every row at every step), a ONE-workgroup launch that adds the slabs in ascending order, takes the
 * argmax by the rule above and writes dev_picks[t] (int32) and dev_gain[t] (float64), and the cover pass with that pick.  One
 * select of k1 + k2 picks equals a select of k1 and one of k2 from the cur the first left.  dev_scratch >=
 * alink_facility_scratch_bytes(N, D, R, k) (0 for sizes the calls refuse; the cover needs what R = 1 gives).
 * All three enqueue on `stream` and return: the stream's order is the only ordering between workgroups — no cooperative launch,
 * no grid barrier, no atomics, nothing read back, no host synchronisation; the (N x R) scores never exist in memory.
 * ALINK_EINVAL, nothing launched and no output touched: a NULL required argument (dev_x, dev_cur, dev_scratch; dev_gain; dev_picks),
 * a pair form without dev_r / dev_ri, N outside 1 .. 2^31 - 1, D outside 1 .. 8192, R outside 1 .. N, dev_cand NULL with R != N,
 * k < 1, S < 0, dev_sel NULL with S > 0, dev_scratch not 256-byte aligned.  Not here: lazy-greedy bounds, row weights, a cosine
 * metric, the cover of pick t fused into the gains pass of pick t + 1, several ranks' pools in one call. */
size_t alink_facility_scratch_bytes(int64_t N, int D, int64_t R, int k);
int alink_facility_gains(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D,
                         const float* dev_cur,             /* (N) */
                         const int32_t* dev_cand,          /* (R) or NULL */
                         int64_t R,
                         double* dev_gain,                 /* (R) */
                         void* dev_scratch, void* stream);
int alink_facility_cover(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D,
                         float* dev_cur,                   /* (N) in / out */
                         const int32_t* dev_sel,           /* (S), NULL with S = 0 */
                         int64_t S, void* dev_scratch, void* stream);
int alink_facility_select(const float* dev_x, const float* dev_r, const int32_t* dev_li, const int32_t* dev_ri, int64_t N, int D,
                          float* dev_cur,                  /* (N) in / out */
                          const int32_t* dev_cand,         /* (k, R) or NULL */
                          int64_t R, int k,
                          int32_t* dev_picks,              /* (k) picks in order, -1 = no candidate of that step gained */
                          double* dev_gain,                /* (k) */
                          void* dev_scratch, void* stream);
/* Identification over a (P, G, C) score array — P probes, G gallery entries, C scores per pair — one row reduction per probe
 * (code/ALINK_MTP.py:285-287: np.argmax of the squeezed (G, 2) scores of one probe, compared with the person id).  Any of the
 * three outputs may be NULL; every result is a pure function of the row (no atomics, fixed reduction order):
 *   dev_flat_argmax[p] = np.argmax of row p FLATTENED to G * C: the first maximum.  This is the index the reference compares
 *                        with the person id (its quirk: gallery g wins through column c at index g * C + c).
 *   dev_best[p]        = the lowest g that maximises scores[p][g][col]                                     (EXTENSION)
 *   dev_rank[p]        = the 0-based position of gallery dev_true[p] in a STABLE descending sort of column col: the number
 *                        of g with a strictly larger score plus the number of g < dev_true[p] with an equal one; -1 when
 *                        dev_true[p] is outside 0 .. G - 1 (the row is not read at that index).  Needs dev_true.  (EXTENSION)
 * Comparisons are `>`: a NaN never wins (np.argmax would return it) and counts as neither larger nor equal.
 * 0 <= col < C, G >= 1, G * C < 2^31; P == 0 writes nothing. */
int alink_identify_rows(const float* dev_scores, int P, int G, int C, int col, const int32_t* dev_true,
                        int32_t* dev_flat_argmax, int32_t* dev_best, int32_t* dev_rank, void* stream);

/* ------------------------------------------------------------------------------------------------
 * DFW protocol evaluation (utilities/ROC_precompute.py:19-63): over the strict upper triangle of an
 * n x n score matrix, pairs are genuine / impostor by the protocol mask (codes 1,2 genuine; 3,4
 * impostor) and roc_case (1: codes 1 vs 3; 2: 2 vs 4; 3: {1,2} vs {3,4}).  dev_hist receives
 * [2][n_thr+1] counts: hist[k][c] = number of class-k (0 genuine, 1 impostor) scores with exactly c
 * of the ASCENDING thresholds <= score.  True/false positives at the threshold of rank t are the
 * suffix sums over c > t (a-link_amd/evaluation.py); the call zeroes dev_hist itself.
 * ---------------------------------------------------------------------------------------------- */
int alink_roc_counts(const float* dev_scores, const uint8_t* dev_mask, int n,
                     const double* dev_thr_sorted, int n_thr, int roc_case,
                     unsigned long long* dev_hist, void* stream);

/* ------------------------------------------------------------------------------------------------
 * A2-LINK perturbation stage (code/noise.py, code/attack.py:5-29, code/committee.py:22-37).
 * Images are float32 (n, H, W, C) as everywhere upstream of the models.  Random draws come from a
 * counter-based Philox4x32-10 keyed by (seed, element index): results do not depend on the launch
 * shape, and `offset` (elements; any value) / `first_image` (images) let a caller process a row range of one
 * logical array — a chunk, or one rank's shard of the pair batch (a-link_amd/alink_loop.py with `group`) —
 * and get exactly what the whole array would have drawn there.
 * The reference draws from the unseeded np.random global stream, so only the distributions are
 * contractual.  In-place (dev_out == dev_in) is allowed for every call except alink_resize_bilinear.
 * ---------------------------------------------------------------------------------------------- */
/* noise.Gaussian.addIndividualNoise (code/noise.py:40-45): out = x + N(mean, sigma) */
int alink_noise_gaussian(const float* dev_in, float* dev_out, int64_t count, float mean, float sigma,
                         uint64_t seed, uint64_t offset, void* stream);
/* noise.Speckle.addIndividualNoise (code/noise.py:83-88): out = x + x * N(0,1) / divisor (15) */
int alink_noise_speckle(const float* dev_in, float* dev_out, int64_t count, float divisor,
                        uint64_t seed, uint64_t offset, void* stream);
/* EXTENSION (the random start of noise.PGD; no counterpart in code/noise.py): out = x + U(lo, hi), the element's
 * 24-bit uniform from the same (seed, element) keying */
int alink_noise_uniform(const float* dev_in, float* dev_out, int64_t count, float lo, float hi,
                        uint64_t seed, uint64_t offset, void* stream);
/* Dropout keep-masks for alink_smallres_train_step (Keras Dropout(0.25) after each pool of the SmallRes tower,
 * code/siamese.py:146,153; TensorFlow draws them with an op-level generator that cannot be reproduced — only the keep
 * probability is contractual): dev_out[e] = 1 with probability `keep`, from the same (seed, element) Philox keying. */
int alink_keep_masks(uint8_t* dev_out, int64_t count, float keep, uint64_t seed, void* stream);
/* ... elements first, first + 1, ... of that stream of masks: a rank that trains rows lo : hi of a pair batch draws exactly the
 * masks the whole-batch step draws for those rows (the data-parallel SmallRes step) */
int alink_keep_masks_at(uint8_t* dev_out, int64_t count, float keep, uint64_t seed, uint64_t first, void* stream);
/* noise.SaltPepper.addIndividualNoise (code/noise.py:54-65), tuple-index semantics: per image n_salt
 * elements (r,c,ch) <- 1 then n_pepper elements <- 0, r in [0,H-2], c in [0,W-2], ch in [0,C-2]. */
int alink_noise_saltpepper(const float* dev_in, float* dev_out, int n_images, int H, int W, int C,
                           int n_salt, int n_pepper, uint64_t seed, uint64_t first_image, void* stream);
/* noise.Poisson.addIndividualNoise (code/noise.py:72-76): per image vals = 2^ceil(log2(#unique)),
 * out = Poisson(x * vals) / vals.  dev_vals (optional, n_images) receives vals. */
size_t alink_noise_poisson_scratch_bytes(int n_images, int64_t per_image);
int alink_noise_poisson(const float* dev_in, float* dev_out, int n_images, int64_t per_image,
                        uint64_t seed, uint64_t first_image, void* dev_scratch, size_t scratch_bytes,
                        float* dev_vals, void* stream);
/* noise.Perlin (code/noise.py:95-150): three octaves ns3[0..2] of gradient noise on square
 * size x size images, the same noise added to every channel.  dev_vec holds the unit gradient
 * vectors [n_images][alink_perlin_nodes(size, ns3)][2], octave after octave, row-major grids of
 * (size/ns + 1)^2 nodes (code/noise.py:100-107); alink_perlin_vectors fills it with random ones. */
int alink_perlin_nodes(int size, const int* ns3);
int alink_perlin_vectors(int n_images, int nodes_total, uint64_t seed, uint64_t first_image, float* dev_vec,
                         void* stream);
int alink_noise_perlin(const float* dev_in, float* dev_out, int n_images, int size, int C,
                       const int* ns3, const float* dev_vec, void* stream);
/* committee.Bagging.resize (code/committee.py:22-26): cv2.resize(image, (Wo, Ho)), INTER_LINEAR */
/* EXTENSION (FGSM / PGD, not in the reference whose only attack is the few-pixel search of code/attack.py): one
 * signed-gradient step and the projection back into the eps-ball of the clean image and the pixel range, in place:
 *   adv <- clip(clip(adv + step * sign(grad), clean - eps, clean + eps), lo, hi)      (n float32 elements; 16-byte
 * aligned buffers take 16-byte lane accesses, any other alignment the scalar form; pass -INFINITY / INFINITY for no pixel
 * clip; step < 0 descends). */
int alink_pgd_step(float* dev_adv, const float* dev_clean, const float* dev_grad, int64_t n, float step, float eps,
                   float lo, float hi, void* stream);
int alink_resize_bilinear(const float* dev_in, float* dev_out, int n, int H, int W, int C, int Ho,
                          int Wo, void* stream);
/* EXTENSION: the exact adjoint of alink_resize_bilinear — dev_din (n, H, W, C) = Ry^T . dev_dout (n, Ho, Wo, C) . Rx with the
 * forward's own tap positions and weights — for gradients that must reach the pixels BEFORE a resize (noise.FGSM / PGD on a
 * SmallRes student fed resized pairs).  Gather form, fixed summation order, no atomics: bit-reproducible, and exactly 0.0 on
 * source elements no destination tap touches.  Runs on the device that owns the buffers; not in place. */
int alink_resize_bilinear_grad(const float* dev_dout, float* dev_din, int n, int H, int W, int C, int Ho, int Wo,
                               void* stream);
/* attack.perturb_image (code/attack.py:5-29): n candidates x k pixels (x, y, r, g, b) as float64
 * (the DE population, truncated like astype(int)) written into n copies of dev_img (Hc, W, 3).
 * split = 0: dev_out is (n, Hc, W, 3); split = 1: dev_out is [2][n][Hc/2][W][3], the top and
 * bottom halves as two contiguous batches (noise.PredictionWrappedModel.predict, code/noise.py:158-168). */
int alink_perturb_images(const float* dev_img, const double* dev_xs, int n, int k, int Hc, int W,
                         int split, float* dev_out, void* stream);
/* The same for the candidates of SEVERAL searches in one launch (PixelAttacker.attack_all, code/attack.py:91-103, advances
 * K pairs' differential-evolution searches in lock-step): dev_imgs is a table [n_img][Hc][W][3] of stacked pair images,
 * candidates [g * group, (g + 1) * group) perturb image dev_img_of[g] (int32, device; NULL: image 0 for all). */
int alink_perturb_images_multi(const float* dev_imgs, const int* dev_img_of, int group, const double* dev_xs, int n,
                               int k, int Hc, int W, int split, float* dev_out, void* stream);
/* alink_perturb_images_multi(split = 1) followed by alink_resize_bilinear of each half to (Ho, Wo), bit for bit, in ONE pass that
 * never materialises a source-resolution candidate (device memory of the call: the image table and dev_out): dev_out is
 * [2][n][Ho][Wo][3].  Same truncation of coordinates and colours, out-of-range pixels skipped, a later list entry overwrites an
 * earlier one at the same position; taps and weights by the resize's own rule, each half an image of its own (no tap crosses
 * the seam).  Ho == Hc / 2 and Wo == W gives the plain perturb.  One workgroup per candidate: the result does not depend on
 * the launch.  Limits (ALINK_EINVAL beyond): k <= 128 pixels per candidate, Ho and Wo <= 512, Hc even. */
int alink_perturb_resize_multi(const float* dev_imgs, const int* dev_img_of, int group, const double* dev_xs, int n,
                               int k, int Hc, int W, int Ho, int Wo, float* dev_out, void* stream);
/* helpers.augment_data (code/helpers.py:114-141): the affine resampling behind keras_preprocessing's random_rotation /
 * random_shear / random_shift, i.e. scipy.ndimage.affine_transform(channel, A, offset, order, mode='nearest') on every
 * channel, for n_out output images in one launch.  Output i reads image dev_src[i] (int32, device; NULL: image i) of the
 * table dev_in (n_in, H, W, C) float32; its pixel (r, c) samples the source at
 *   y = (r m00 + c m01) + m02,  x = (r m10 + c m11) + m12      (dev_mat[i] = {m00, m01, m02, m10, m11, m12}, float64)
 * with each coordinate clamped to [0, n - 1]; order 1 interpolates bilinearly, order 0 takes the nearest tap.  All of it in
 * float64 with scipy's operation order: the float32 results equal scipy's bit for bit.  dev_copy[i] != 0 (uint8, device;
 * NULL: none) makes output i a byte copy of its source (Keras returns the input untouched when a drawn parameter is 0).  A
 * source index outside [0, n_in) yields a row of NaN.  dev_out (n_out, H, W, C) must not overlap dev_in. */
int alink_affine_warp(const float* dev_in, int n_in, const int32_t* dev_src, const double* dev_mat, const uint8_t* dev_copy,
                      int n_out, int H, int W, int C, int order, float* dev_out, void* stream);
/* EXTENSION — the raw-photo front end (code/face_preprocess.py:46-111 — the call code/face_model.py:81 comments out — and the
 * crop + resize of code/readDFW.py:28-62,82) for a RAGGED batch: n photos, each of its own size, become n faces of Ho x Wo in
 * one launch.  dev_pixels is one packed table of total_elems elements (src_dtype 0: uint8, 1: float32) holding HWC photos end
 * to end; descriptor i places photo i in it and names its route: */
typedef struct AlinkIngestDesc {
    int64_t offset;   /* first element of the photo in the table */
    int32_t H, W;     /* its size; it occupies H * W * C elements */
    int32_t mode;     /* 0: crop `box`, then resize;  1: affine warp by `m` */
    int32_t box[4];   /* mode 0: x0, y0, x1, y1, half-open, inside the image */
    double m[6];      /* mode 1: OUTPUT pixel (ox, oy) -> source (sx, sy) = ((ox m0 + oy m1) + m2, (ox m3 + oy m4) + m5) */
} AlinkIngestDesc;
/*   mode 0: what alink_resize_bilinear gives for the sub-image `box` resized to (Ho, Wo), bit for bit — the same tap rule and
 *           roundings (csrc/resize_taps.h) relative to the box; no tap leaves the box.
 *   mode 1: bilinear interpolation at (sx, sy) with a black border, in float64 with scipy's operation order: per axis
 *           w0 = 1 - (s - floor s), w1 = 1 - w0; t = 0 + sum over the 2 x 2 taps (row-major) of (v * wy) * wx with v = 0 for a
 *           tap outside the image; exactly 0 when sx <= -1, sx >= W, sy <= -1 or sy >= H; out = (float) t.  Equal bit for bit
 *           to scipy.ndimage.affine_transform(channel, [[m4, m3], [m1, m0]], offset=[m5, m2], output_shape=(Ho, Wo), order=1,
 *           mode='grid-constant', cval=0, output=float32).
 * dev_out is (n, Ho, Wo, C) for layout 0 (NHWC) or (n, C, Ho, Wo) for layout 1 (NCHW), float32, unrounded.  The kernel never
 * reads outside the table: a descriptor with offset < 0, offset + H W C > total_elems, H or W < 1, an unknown mode or, in
 * mode 0, a box that is empty or leaves the image yields a row of NaN (callers validate on the host: a-link_amd/
 * face_preprocess.py).  ALINK_EINVAL: C, Ho, Wo < 1, an unknown layout or src_dtype, 2^31 or more workgroups
 * (n * ceil(Ho Wo / 256)), dev_out overlapping the table.  Runs on the device that owns dev_out. */
int alink_ingest_faces(const void* dev_pixels, int src_dtype, int64_t total_elems, const AlinkIngestDesc* dev_desc, int n, int C,
                       int Ho, int Wo, int layout, float* dev_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * EXTENSIONS — named by BASELINE.json's north_star, ABSENT from the reference: the reference
 * cuts the ArcFace checkpoint at fc1_output and never builds the margin head (code/face_model.py:35-36,53),
 * and trains its pair scorer with binary cross-entropy on |l - r| (code/siamese.py:27-35), not with a
 * contrastive loss.  Provided for callers that fine-tune the backbone's embedding space; checked against torch
 * autograd (tests/test_gpu_extensions.py), not against the reference.
 * ---------------------------------------------------------------------------------------------- */
/* Additive angular margin softmax (ArcFace): loss = mean_i CE(softmax(s * cos(theta_ij + m [j == y_i])), y_i) over
 * L2-normalised embeddings (N x D) and class centres (C x D); where theta + m would pass pi the target logit is
 * cos(theta) - m sin(pi - m) (easy_margin: cos(theta) itself for cos(theta) <= 0).  dev_demb (N x D) / dev_dW (C x D)
 * receive the gradients w.r.t. the RAW (un-normalised) inputs, or are NULL. */
size_t alink_arcface_margin_workspace_bytes(int N, int D, int C);
int alink_arcface_margin_loss(const float* dev_emb, const float* dev_W, const int32_t* dev_labels, int N, int D,
                              int C, float s, float m, int easy_margin, float* dev_loss, float* dev_demb,
                              float* dev_dW, void* dev_workspace, size_t workspace_bytes, void* stream);
/* Pairwise-L2 contrastive loss: d_p = sqrt(max(|L_p - R_p|^2, 1e-7)),
 * loss = mean_p [ y_p d_p^2 + (1 - y_p) max(margin - d_p, 0)^2 ]  (y = 1: same identity).
 * dev_pair_loss (P) receives the per-pair terms; dev_dL / dev_dR (P x D) the gradients, or both NULL. */
int alink_contrastive_loss(const float* dev_L, const float* dev_R, const float* dev_y, int64_t P, int D,
                           float margin, float* dev_loss, float* dev_pair_loss, float* dev_dL, float* dev_dR,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* ALINK_HIP_H */
