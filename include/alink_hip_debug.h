/* alink_hip_debug.h — the A/B and diagnostic switches libalink_hip.so exports BESIDE the product ABI (include/alink_hip.h).
 *
 * Nothing in the reference maps to these (it has no native code: SURVEY.md §0); they exist so that a measurement can run the
 * same binary with one kernel form swapped for another (bench.py's A/B flags, tools/layer_profile.py, tests that assert two
 * forms bit-identical) and so that tools/ can read in-kernel stamps.  Contract:
 *   - PROCESS-GLOBAL and NOT thread-safe: a switch changes which kernel form every handle of the process launches from the
 *     next call on (a few are read once, at alink_backbone_create: noted below).  Set them before the work they are meant
 *     for, from one thread, and set them back.
 *   - No switch changes a RESULT beyond what the product documents: every alternative form is bit-identical to the default
 *     (asserted in tests/test_gpu_backbone.py, tests/test_gpu_conv.py) except where noted.
 *   - A product build may drop them (`make DEBUG_SWITCHES=0` is not implemented: they cost one global each); product code in
 *     a-link_amd/ calls none of them outside tests, tools and bench.py's A/B flags.
 * tests/test_abi.py fails on any exported `alink_*` symbol that neither this header nor alink_hip.h declares. */
#ifndef ALINK_HIP_DEBUG_H
#define ALINK_HIP_DEBUG_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- which convolution kernel a layer takes (csrc/backbone.hip's dispatch) --------------------------------------------- */
/* bit mask of widths on the linear-tile kernel (bit0 56, bit1 28, bit2 14, bit3 7 wide maps); default all; a width whose
 * bit is clear takes conv3x3_direct_kernel.  Cannot enable the kernel on a device whose LDS out-of-range probe failed. */
void alink_debug_set_linear(int mode);
/* 1: the linear-tile kernel with its run-time-flag epilogue everywhere (default 0: compile-time epilogues where they exist) */
void alink_debug_set_generic_epilogue(int on);
/* 0: never conv3x3_direct_kernel (everything it would take goes to the implicit GEMM) */
void alink_debug_set_direct(int on);
/* 0: conv3x3_direct_kernel's one-workgroup-per-CU variants only (default 1: the two-per-CU variants where they exist) */
void alink_debug_set_pair(int on);
/* 0: the 112-wide 64 -> 64 layer on the tile kernels instead of the rolling-row kernel (conv3x3_c64.hip) */
void alink_debug_set_c64(int on);
/* 0: stage1_unit1's stride-2 conv2 (+ shortcut) on the implicit GEMM instead of the direct stride-2 kernel (conv3x3_s2c64.hip) */
void alink_debug_set_s2direct(int on);
/* 0: stem and stage1_unit1 conv1 as two launches instead of the fused front kernel (front_c64.hip) */
void alink_debug_set_fuse_stem(int on);
/* plain 56 x 56 x 64 residual units (stage 1) in one launch, conv1's output kept in LDS (unit_c64.hip; 16-bit forward only):
 * 0 = never (two conv3x3_linear launches), 1 = from the batch size the dispatch picks (default), 2 = at every batch size */
void alink_debug_set_fuse_unit(int mode);
/* the stem and the whole of stage1_unit1 (conv1, stride-2 conv2 + shortcut) in one launch, neither conv1's output nor the
 * shortcut's operand leaving LDS (unit1_c64.hip; 16-bit inference forward at 112 x 112 only): 0 = never (the fused front
 * kernel + the direct stride-2 kernel), 1 = from the batch size the dispatch picks (default), 2 = at every batch size.
 * alink_debug_set_fuse_stem(0) and alink_debug_set_s2direct(0) each turn it off as well. */
void alink_debug_set_fuse_unit1(int mode);
/* 0: projection shortcuts as launches of their own instead of extra K-steps of conv2.  READ AT alink_backbone_create. */
void alink_debug_set_fuse_shortcut(int on);
/* 0: the implicit GEMM stages its tiles through registers (global_load -> ds_write) instead of LDS-DMA */
void alink_debug_set_dma(int on);
/* largest 128-channel grid (workgroups) that still takes the 64-channel form of the linear-tile kernel (default 384) */
void alink_debug_set_fine_max(int n);
/* 0: the 64- / 128-channel form chosen per shard, blind to the call's other shards */
void alink_debug_set_sibling_aware(int on);
/* launches of at most this many output pixels take the latency form (conv3x3_lat.hip); 0 = never; default 1600 */
void alink_debug_set_latency_form(int max_pixels);
/* latency form's block shape: -1 by size (default), 0 = 16 x 16 per wave, 1 = 32 x 16, 2 = 32 x 32 */
void alink_debug_set_latency_tiles(int form);
/* start delay (x 1024 cycles) of the second workgroup on a CU in the linear-tile kernel (default 0; measured out) */
void alink_debug_set_stagger(int n);
/* 0: the linear-tile kernel refills its single input buffer after a 64-channel chunk's last K-step and waits with nothing
 * else in flight (default 1: the refill is requested inside that K-step, under its MFMAs) */
void alink_debug_set_early_refill(int on);
/* in-call shards start one after the other's front (default 0; measured out) */
void alink_debug_set_shard_stagger(int on);

/* ---- the pair head (csrc/head.hip) ------------------------------------------------------------------------------------ */
/* 0: batches <= 32 on the generic train chain instead of the three-launch tiny step */
void alink_debug_set_tiny_step(int on);
/* 0: alink_head_train_step_input_grads on the generic chain (train step, then input gradients) for SmallRes' head shape too */
void alink_debug_set_mini_step(int on);
/* 0: the bf16 compute mode's predict on the f32-input kernel with in-flight rounding instead of head_fwd_bf16_kernel */
void alink_debug_set_head_bf16_mfma(int on);

/* ---- SmallRes (csrc/smallres.hip) -------------------------------------------------------------------------------------- */
/* 0: the weight gradients of a train step on the caller's stream, after their dz, instead of a side stream beside the dz chain */
void alink_debug_set_smallres_overlap(int on);
/* 0: a train step ends with two update launches (the tower's, the head's) instead of one (the same bits) */
void alink_debug_set_smallres_one_update(int on);

/* ---- diagnostics ------------------------------------------------------------------------------------------------------ */
/* alink_embed returns after this many convolution launches (0 = the whole chain): per-layer timing by difference.
 * CHANGES THE RESULT (the embedding is garbage): tools only. */
void alink_debug_set_stop_after(int n);
/* alink_embed_profile launches every kernel this many times back to back between its two events (default 4) */
void alink_debug_set_profile_reps(int n);
/* ablation builds of the rolling-row kernels (1 = no stores, 2 = no MFMA, ...: tools/experiments).  CHANGES THE RESULT. */
void alink_debug_set_ablate(int a);
/* device buffer (8 x u64 per workgroup) that the STAMP builds of the tile kernels fill with s_memtime readings; NULL = off */
void alink_debug_set_stamps(void* dev_u64);
/* the hardware contract the linear-tile kernel rests on: a DS read beyond the workgroup's LDS allocation returns zero.
 * Writes 516 probe values to dev_out516 (tests/test_gpu_conv.py reads them); returns ALINK_OK or an error code. */
int alink_debug_lds_oob_probe(float* dev_out516, void* stream);
/* 1 if that probe passed on the current device at alink_init (the linear-tile kernel is used only then) */
int alink_debug_linear_contract_ok(void);


/* ---- what the input-gradient passes read from the caller's workspace (read-only queries: nothing is launched or changed) - */
/* The cached forwards (alink_resnet50_embed_cached, alink_embed_cached) keep activations in the gradient workspace the caller
 * owns; the backward takes its ReLU / PReLU masks and max-pool winners from them.  These tell a test where they are, so that
 * a reference can use the SAME masks (tests/test_gpu_grad_masked.py).  Entry `index` of the layout for n_images images: byte
 * offset from the (256-byte aligned) workspace pointer, shape [n_images][H][W][C] in the network's 16-bit type, and a name.
 * Return the number of entries (also for index < 0, which fills nothing), or -1 with alink_last_error set.  Any out pointer
 * may be NULL.
 *   ResNet-50: "stem" (conv1/7x7_s2 after ReLU), "pool" (max-pool output), then per unit "convS_U_reduce", "convS_U_3x3"
 *   (after ReLU) and "convS_U_out" (the unit's output, after the ReLU of the sum).
 *   IR backbone: "stem" (after PReLU), per unit "stageS_unitU_conv1" (after PReLU), and last "norms": FLOAT32 [n_images]
 *   (H = W = C = 1), the row norms the L2 normalisation divided by. */
struct alink_resnet50;
struct alink_backbone;
int alink_debug_resnet50_grad_cache_info(const struct alink_resnet50* r, int n_images, int index, size_t* byte_offset, int* H,
                                         int* W, int* C, char* name_buf, int name_len);
int alink_debug_backbone_grad_cache_info(const struct alink_backbone* bb, int n_images, int index, size_t* byte_offset, int* H,
                                         int* W, int* C, char* name_buf, int name_len);

/* ---- the VGG-16 forward stopped early (csrc/vgg16.hip) ------------------------------------------------------------------- */
/* alink_vgg16_embed's own op loop, run for ops [0, n_ops) only, on the caller's workspace: the arguments of alink_vgg16_embed,
 * then n_ops and what op n_ops - 1 wrote.  The network is 18 ops in execution order: "conv1_1" (the stem), twelve
 * convolutions "convB_L" and the five pools "pool1" .. "pool5", each behind its block.  Reported for op n_ops - 1: the byte
 * offset of its output from the workspace pointer, its shape [n_images][H][W][C] in the handle's 16-bit type, its name, the
 * ConvKernel chosen at finalize (csrc/conv_kernel.h; -1 for the stem and the pools) and the form that serves this launch, by
 * the rule alink_conv_nhwc_ex reports by (0 = that kernel, 1 = conv3x3_lat_kernel, 2 = conv_gemm_lat_kernel).  With
 * n_ops = 18 the output is the float32 features in dev_out ([n_images][H * W * C]; byte_offset is 0); a shorter prefix does
 * not touch dev_out, which may then be NULL.  Any out pointer may be NULL.  Returns the number of ops, or -1 with
 * alink_last_error set; with n_ops <= 0 nothing is launched and nothing filled.  Tests only (tests/test_gpu_vgg16.py). */
struct alink_vgg16;
int alink_debug_vgg16_embed_prefix(struct alink_vgg16* r, const float* dev_in, int n_images, int preprocessed, float* dev_out,
                                   void* ws, size_t ws_bytes, void* stream, int n_ops, size_t* byte_offset, int* H, int* W,
                                   int* C, char* name_buf, int name_len, int* kernel, int* form);

/* ---- the ResNet-50 forward stopped early (csrc/resnet50.hip) --------------------------------------------------------------- */
/* alink_resnet50_embed's own op loop, run for ops [0, n_ops) only, on the caller's workspace: the arguments of
 * alink_resnet50_embed, then n_ops and what op n_ops - 1 wrote.  The network is 55 ops in execution order: "conv1/7x7_s2" (the
 * stem), "max_pool", the 52 convolutions (per unit "convS_U_1x1_reduce", "convS_U_3x3", on a stage's first unit
 * "convS_U_1x1_proj", then "convS_U_1x1_increase") and "avg_pool"; the names are alink_resnet50_op_name's.  Reported for op
 * n_ops - 1: the byte offset of its output from the workspace pointer, its shape [n_images][H][W][C] in the handle's 16-bit
 * type (split precision: [n_images][H][W][2 C] halves, each 64-channel chunk [hi 64 | lo 64]), its name, the ConvKernel chosen
 * at finalize (csrc/conv_kernel.h; -1 for the stem and the pools), the form that serves this launch (0 = that kernel,
 * 1 = conv3x3_lat_kernel, 2 = conv_gemm_lat_kernel) and, in split precision, the exponent e of that output (stored value =
 * true value x 2^e; 0 in the 16-bit types and for the features).  With n_ops = 55 the output is the float32 features in
 * dev_out ([n_images][2048], H = W = 1, byte_offset 0); a shorter prefix does not touch dev_out, which may then be NULL.  Any
 * out pointer may be NULL.  Returns the number of ops, or -1 with alink_last_error set; with n_ops <= 0 nothing is launched
 * and nothing filled.  Tests only (tests/test_gpu_resnet50_layers.py). */
int alink_debug_resnet50_embed_prefix(struct alink_resnet50* r, const float* dev_in, int n_images, int preprocessed, float* dev_out,
                                      void* ws, size_t ws_bytes, void* stream, int n_ops, size_t* byte_offset, int* H, int* W,
                                      int* C, char* name_buf, int name_len, int* kernel, int* form, int* scale_exp);

#ifdef __cplusplus
}
#endif
#endif /* ALINK_HIP_DEBUG_H */
