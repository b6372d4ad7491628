/* vk_unet.h — C ABI of libvkunet.so: the MI355X (gfx950) implementation of the one compute path of
 * ZooMEISTER/vickers-hardness-Unet: ResNet-34-encoder U-Net forward / BCE+Dice loss / backward /
 * AdamW on NHWC tensors, as hand-written HIP kernels.
 *
 * The reference has no FFI layer of its own: the path sits behind the Python nn.Module / loss /
 * optimizer protocol.  Each entry point below names the reference call it replaces:
 *
 *   vk_unet_create / vk_unet_param_info ....... smp.Unet(...) construction   train.py:372-378, infer_pth_gui.py:31-33
 *   vk_unet_forward ........................... model(x)                     train.py:436, 510, 693; infer_pth_gui.py:51
 *   vk_unet_loss .............................. bce(logits,y)+dice(logits,y) train.py:438, 513 (600-601)
 *   vk_unet_backward .......................... loss.backward()              train.py:443, 448
 *   vk_unet_set_trainable ..................... p.requires_grad_(False) before backward (fine-tuning with a frozen encoder)
 *   vk_unet_set_bn_frozen ..................... module.eval() of single BatchNorm layers inside a training forward
 *   vk_unet_set_input_grad .................... x.requires_grad_() (x.grad: saliency maps)
 *   vk_unet_create_in / vk_input_mix .......... smp.Unet(in_channels=1..4) (train.py:375 passes 3) and the 3-channel data path's bridge to it
 *   vk_seg_metrics ............................ dice_coef / iou_coef (validate) train.py:230-281, 518-522
 *   vk_seg_metrics_multi ...................... the same per class for Unet(classes=C): counts tp/fp/fn/tn, Dice / IoU per class
 *   vk_sweep_hist / vk_sweep_curves ........... validate's Dice / IoU at every threshold of a grid from one pass (the reference's GUIs
 *                                               hand-pick 0.50 and 0.45), plus the precision-recall and ROC curves
 *   vk_comm_* / vk_allreduce_bucket ........... (no reference counterpart: the 8-GPU data-parallel exchange)
 *   vk_adamw_step ............................. optimizer.step()/zero_grad   train.py:428, 449 (606)
 *   vk_amp_check_inf / vk_amp_unscale_check /
 *   vk_adamw_step_amp ......................... GradScaler unscale + inf check + skipped step  train.py:441-445 (610-611)
 *   vk_adamw_step_amp_segments ................ the same over the tensors that have a gradient (frozen ones are skipped)
 *   vk_adamw_step_groups / vk_grad_norm_segments  param groups ([dict(params=..., lr=...)]) and clip_grad_norm_ (no reference line:
 *                                               the standard fine-tuning recipe around train.py:606)
 *   vk_avg_update / vk_avg_swap ............... EMA / SWA of the weights and BatchNorm statistics over the flat buffers, and the in-place
 *                                               exchange that evaluates with them (no reference line: AveragedModel / ModelEmaV2)
 *   vk_adamw_step_amp_avg ..................... vk_adamw_step_amp with that average updated in the same launch
 *   vk_conv_fwd / vk_conv_wgrad / ... ......... the ATen operators the reference dispatches to
 *                                               (conv2d, batch_norm, relu, max_pool2d, interpolate, cat)
 *   vk_conv_fwd_splitk ........................ the same convolutions at batch 1 (predict_mask / Segmenter.infer)
 *   vk_letterbox_preprocess ................... letterbox + BGR->RGB + normalise   infer_pth_gui.py:17-24, 46-49;
 *                                               ui_infer_quadrilateral.py:197-216, 662-678; ui_infer_rectangle.py:225-245, 520-535
 *   vk_letterbox_postprocess_mask ............. sigmoid, threshold, un-letterbox  infer_pth_gui.py:26-29, 50-53
 *   vk_letterbox_postprocess_prob ............. sigmoid, un-letterbox, clip       ui_infer_quadrilateral.py:219-231, 705-711
 *   vk_letterbox_postprocess_labels / _mask_multi / _prob_multi  the same for C class planes: argmax label map, per-class masks,
 *                                               per-class sigmoid or softmax probabilities
 *   vk_geom_minarearect ....................... postprocess_minarearect_multi      ui_infer_rectangle.py:291-381
 *   vk_geom_quadrilateral ..................... postprocess_minarearect_multi + robust_quadrilateral_from_contour  ui_infer_quadrilateral.py:262-530
 *   vk_letterbox_u8 / _mask_u8 / vk_augment_batch  VickersDataset.__getitem__ + albumentations pipeline  train.py:67-113, 173-200
 *   vk_patch_index / vk_patch_batch ........... random S x S training patches of the full-resolution images (no counterpart: the
 *                                               reference trains on letterboxed images only)
 *   vk_cp_boxes / vk_cp_alpha / vk_cp_paste ... instance copy-paste between the letterboxed items (no counterpart: the reference never
 *                                               composes images)
 *   vk_mg_render .............................. synthetic indentation micrographs with exact masks, rendered into the uint8 slot that
 *                                               vk_augment_batch reads (no counterpart: the reference has its 183 photographs)
 *   vk_edt_sq / vk_boundary_phi / _stats / _loss  distance maps, surface-distance metrics and the boundary loss (no counterpart)
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types cross this boundary.
 *   - every device buffer is owned by the caller (PyTorch's allocator in the Python host);
 *     the library allocates nothing on the device and keeps no pointer after a call returns,
 *     except those bound to a vk_unet handle by vk_unet_bind (valid until rebind / destroy).
 *   - all work is enqueued on the hipStream_t passed in (void* stream); no hidden synchronisation.
 *   - return value: 0 = success, <0 = argument/shape error found on the host (VK_ERR_*),
 *     >0 = hipError_t from a launch.  vk_last_error_string() gives the text.  Nothing throws.
 *   - activations are NHWC; weights are KRSC ([K_out][R][S][C_in], i.e. torch channels_last of OIHW).
 */
#ifndef VK_UNET_H
#define VK_UNET_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VK_ABI_VERSION 1
/* BatchNorm partial sums are spread over this many replicas ([R][2][K] doubles) so that tens of thousands of
 * workgroups do not serialise on the same 2K addresses; vk_bn_finalize adds the replicas up. */
#define VK_STATS_REPLICAS 32

typedef enum { VK_F32 = 0, VK_BF16 = 1, VK_F16 = 2 } vk_dtype;

enum { VK_OK = 0, VK_ERR_ARG = -1, VK_ERR_STATE = -2, VK_ERR_UNSUPPORTED = -3 };

int vk_version(void);
const char* vk_last_error_string(void);
/* 1 if the code object for gfx950 is present in this build (always true for a product build) */
int vk_has_gfx950_code(void);
/* Measurement aid (bench.py): a bare loop of independent v_mfma_f32_16x16x32_bf16 on register operands, `waves_per_simd` waves on
 * every SIMD of the chip, `iters` x 8 MFMAs each — what the matrix pipes deliver at the clock the chip sustains under that load.
 * FLOPs issued = *flops_out (when not null); time it with events on `stream`.  sink: 4 floats of device scratch. */
int vk_probe_mfma_rate(int iters, int waves_per_simd, float* sink, double* flops_out, void* stream);
/* Data-parallel runs: while a communication library's kernels hold compute units, launches sized to exactly one workgroup per CU
 * (the weight-gradient kernels: <= 256 persistent workgroups that split the pixel tiles among themselves) fall into a second round.
 * n > 0 sizes those grids for (CUs - n) instead; 0 (default) restores the full chip.  Process-wide, read per launch; the Python host
 * sets it only for the backward stages that overlap a collective (parallel.py).  Returns the previous value. */
int vk_set_reserved_cus(int n);
/* Measurement aid (tests/diag/cu_hold.py): occupy compute units the way a communication library's channel kernels do while a step
 * runs on another stream.  Launches `workgroups` workgroups of `threads` threads (64..1024) with `lds_bytes` of LDS each
 * (lds_bytes = 163840 takes a whole CU: no tile kernel fits beside it; a small value lets other workgroups co-reside and only
 * competes for issue slots / memory queues) that spin for `microseconds` of wall time (s_memrealtime deadline: every wave exits by
 * itself) and, when `traffic` != 0, keep streaming 16-byte loads from it (traffic_bytes, a power of two >= 64 KiB) meanwhile.
 * sink: 4 floats of device scratch. */
int vk_debug_hold_cus(int workgroups, int threads, int lds_bytes, int microseconds, const void* traffic, size_t traffic_bytes,
                      float* sink, void* stream);

/* Per-launch timing (off by default): while enabled every launch made through this library is bracketed
 * by two hipEvents on its own stream.  vk_prof_collect synchronises those events and writes one line per
 * kernel family into buf: "tag count total_ms total_algorithmic_flops total_algorithmic_bytes\n";
 * returns the number of bytes written (or <0).  Used by bench.py for the live roofline figure. */
/* diagnostic builds only (make stamp): buffer receiving per-wave s_memtime segment totals of the tile kernels */
int vk_debug_set_stamp_buffer(void* device_buffer);
int vk_prof_enable(int on);
int vk_prof_collect(char* buf, size_t buflen);

/* ------------------------------------------------------------------------------------------------
 * Operator level (used by the engine below and by the per-kernel parity tests)
 * ---------------------------------------------------------------------------------------------- */

/* One input source of a convolution gather.  The convolution reads a *virtual* input
 *   V[n][h][w][c] = act( src[n][h >> up][w >> up][c] * scale[c] + shift[c] )
 * i.e. nearest-x2 upsample (up=1), train/eval BatchNorm apply (scale/shift != NULL) and ReLU (relu=1)
 * are fused into the operand load; zero padding is applied AFTER that transform.
 * relu is honoured only together with scale / shift: a source with scale == NULL is read as it is (identity), whatever relu says —
 * every kernel applies the ReLU inside its affine prologue (convolutions, both heads, their weight gradients alike). */
typedef struct {
  const void* ptr;      /* NHWC, dtype of the conv, [N][H>>up][W>>up][C] */
  int C;                /* channels of this source (multiple of 8; 16 allowed) */
  int up;               /* 0 or 1 */
  const float* scale;   /* [C] or NULL (identity) */
  const float* shift;   /* [C] or NULL */
  int relu;             /* apply max(.,0) after the affine */
} vk_src;

typedef struct {
  vk_dtype dtype;       /* element type of activations and packed weights */
  int N, H, W;          /* virtual input spatial size (after the optional upsample) */
  int Ho, Wo;           /* output spatial size */
  int K;                /* output channels */
  int R, S, stride, pad;
  int transposed;       /* 0: y[p] = sum_r V[p*stride - pad + r] w[r]   (forward)
                           1: y[p] = sum_r V[(p + pad - r)/stride] w[r] (data gradient; V = dz) */
  vk_src src0, src1;    /* src1.ptr == NULL when there is no channel concat; C = src0.C + src1.C */
} vk_conv_desc;

/* y = conv(V, w).  w: [K][R][S][C] of `dtype`.  y: [N][Ho][Wo][K] of `dtype`.
 * If K >= split_k1 > 0 the output channels [split_k1, K) go to y1 (leading dim K - split_k1) and
 * [0, split_k1) to y (leading dim split_k1): the two halves of a concat gradient.
 * accumulate: y (+)= result.  stats: optional double[VK_STATS_REPLICAS][2][K] receiving (spread over the replicas) sum / sum of squares over
 * N*Ho*Wo of the stored (rounded) outputs — train-mode BatchNorm partials (must be zeroed by caller). */
int vk_conv_fwd(const vk_conv_desc* d, const void* w, void* y, void* y1, int split_k1, int accumulate,
                double* stats, void* stream);

/* Data gradient of a decoder conv1 with the nearest-x2 upsample backward fused in: like vk_conv_fwd with
 * transposed=1, but the first output part (channels [0, split_k1), or all K when split_k1 == 0) is summed over
 * 2x2 pixel groups and written to y_half [N][Ho/2][Wo/2][.]; the skip part still goes to y1 at full resolution.
 * Returns VK_ERR_UNSUPPORTED for shapes outside the 3x3 stride-1 tile kernels (caller then uses
 * vk_conv_fwd + vk_upsample2x_bwd). */
int vk_conv_dgrad_pool2(const vk_conv_desc* d, const void* w, void* y_half, void* y1, int split_k1, int accumulate,
                        void* stream);

/* The 3x3 stride-1 tile kernels read their weights in the "halo pack": [red/CK][9 taps][rows][CK] (CK = 64 bytes of
 * channels), 16-byte pieces pre-swizzled for the LDS image, so that a pipeline stage is three linear 1-KiB-per-wave copies.
 * vk_halo_pack builds it from plain [rows][3][3][red] weights of `dtype` (forward: rows = K, red = C; data gradient: the
 * transposed weights, rows = C, red = K).  vk_conv_uses_halo_pack tells whether a descriptor runs on those kernels
 * (then vk_conv_fwd_packed / vk_conv_dgrad_fused / vk_conv_dgrad_pool2 expect the pack; layers with C == 16 in a 16-bit
 * type keep plain weights).  vk_conv_fwd with plain weights always works (tap-by-tap kernel) but is slower. */
int vk_halo_pack(vk_dtype dtype, int rows, int red, const void* src, void* dst, void* stream);
int vk_conv_uses_halo_pack(const vk_conv_desc* d);
int vk_conv_fwd_packed(const vk_conv_desc* d, const void* w_halo, void* y, void* y1, int split_k1, int accumulate, double* stats,
                       void* stream);

/* vk_conv_fwd_packed without statistics for SMALL grids (batch-1 inference, predict_mask / Segmenter.infer:
 * infer_pth_gui.py:51, ui_infer_quadrilateral.py:705-707): when the layer has fewer than 128 output tiles the channel
 * reduction is cut into up to 32 slices that run as separate workgroups, write fp32 partial tiles into `workspace`
 * ([slices][N*H*W][K] floats; fewer slices when it is smaller, none when NULL) and are added up in slice order by a second
 * launch — same result on every run.  Larger grids run exactly as vk_conv_fwd_packed. */
#define VK_SPLITK_WORKSPACE_BYTES (32u << 20)
int vk_conv_fwd_splitk(const vk_conv_desc* d, const void* w_halo, void* y, void* workspace, size_t workspace_bytes, void* stream);

/* BatchNorm+ReLU backward reduce fused into the kernel that produces the gradient: with y the gradient w.r.t. the
 * activated tensor relu(z*scale+shift), the kernel stores g = y * [z*scale+shift > 0] instead of y and adds sum(g),
 * sum(g*z) into sums [VK_STATS_REPLICAS][2][C] (caller zeroes).  Phase 2 is vk_bn_bwd_apply_fused with mask_mode 0. */
typedef struct {
  const void* z;        /* raw conv output the gradient belongs to, same shape as the gradient */
  const float* scale;
  const float* shift;
  double* sums;
  /* r04 — the tail of a residual block, out = relu(bn2(z) + shortcut) (reference: torchvision BasicBlock.forward behind train.py:436):
   * mask != NULL: the ReLU mask is [mask > 0] (mask = the block's stored output, same shape and type as the gradient) instead of
   * [z*scale+shift > 0]; scale / shift may then be NULL.  accumulate != 0: the convolution result is ADDED to the previous content
   * of y first (the shortcut gradient that is already there), then masked, summed and stored (with split_k1 > 0 the channels that go
   * to y1 are likewise added to the previous content of y1, unmasked).  Together they move the BatchNorm
   * backward reduce of block b into the data gradient of block b+1's conv1, which produces block b's output gradient. */
  const void* mask;
  int accumulate;
} vk_bnr;

/* Data gradient with optional fusions on the first output part (channels [0, split_k1), or all of them):
 * pool2 (see vk_conv_dgrad_pool2) and/or bnr.  VK_ERR_UNSUPPORTED outside the 3x3 stride-1 tile kernels. */
int vk_conv_dgrad_fused(const vk_conv_desc* d, const void* w, void* y, void* y1, int split_k1, int pool2, const vk_bnr* bnr,
                        void* stream);

/* Pointwise convolutions (R = S = 1, pad 0, stride 1 or 2; one source, no upsample): the Bottleneck conv1 / conv3 and the downsample
 * shortcuts of the resnet50 encoder, as MFMA GEMMs over NHWC pixels (fp32: v_mfma_f32_16x16x4_f32).  VK_ERR_UNSUPPORTED for any other
 * descriptor.  Channels (src0.C and K) are multiples of 4 (fp32) / 8 (16-bit); scale / shift 16-byte aligned.
 * vk_conv1x1_fwd, transposed = 0: y[p][k] (+)= sum_c V[p*stride][c] * w[k][c], w [K][C]; stats as vk_conv_fwd's (caller zeroes).
 *                transposed = 1: the data gradient, src0 = dz [N][H][W][src0.C] (H, W: the forward's output grid), K = the forward's
 *                input channels, w = the transposed weights [K][src0.C] (vk_conv_fwd's data-gradient layout), y [N][Ho][Wo][K];
 *                at stride 2 the pixels no tap reaches are written as zero, or left untouched with accumulate.
 * vk_conv1x1_wgrad: dw[K][C] (fp32, +=) = sum_p dz[p][k] * V[p*stride][c], split over pixels with per-split partial tiles in
 *                `workspace` (16-byte aligned; NULL or too small: one split) added up in a fixed order — same bits on every run. */
int vk_conv1x1_fwd(const vk_conv_desc* d, const void* w, void* y, int accumulate, double* stats, void* stream);
int vk_conv1x1_wgrad(const vk_conv_desc* d, const void* dz, float* dw, void* workspace, size_t workspace_bytes, void* stream);

/* Stem: 7x7 stride-2 pad-3 convolution of x4 [N][H][W][4] (the channels past the model's in_channels are zero padding: channel 3
 * of the 3-channel model) with packed weights wp [64][7][32] (tap row r, 8 columns x 4 channels, zero padded).  The kernel multiplies
 * all four channels whatever the model's count is. */
int vk_stem_fwd(vk_dtype dtype, int N, int H, int W, const void* x4, const void* wp, void* y, double* stats,
                void* stream);

/* dw[K][R][S][C] (fp32, +=; caller zeroes once per step) = sum_pixels dz[n][p][q][k] * V[n][p*stride-pad+r][..][c].
 * workspace (optional, 16-byte aligned, VK_WGRAD_WORKSPACE_BYTES is always enough; dw 16-byte aligned): when given, every
 * kernel (3x3 stride-1 tile kernel, tap-by-tap kernel for stride 2 / 1x1, stem) writes per-split partial results there and
 * a second launch adds them up in a fixed order (bit-reproducible gradients); otherwise fp32 atomics. */
#define VK_WGRAD_WORKSPACE_BYTES (64u << 20)
int vk_conv_wgrad(const vk_conv_desc* d, const void* dz, float* dw, void* workspace, size_t workspace_bytes, void* stream);
/* Weight gradients of SEVERAL layers in ONE launch (r03): every layer must be of the class vk_conv_wgrad runs on its 64 x 64 tap-split
 * tile kernel — 16-bit, 3x3 stride 1 pad 1, K >= 64, every source a multiple of 64 channels (vk_conv_wgrad_batch_supports says so).
 * The (layer, output tile, 128-pixel tile) units of all layers are cut into `workgroups` equal ranges (0: one per usable CU); ranges
 * that cross an output tile leave partial tiles in `workspace`, which a second kernel adds in range order: same bits on every run.
 * At most 40 layers.  Replaces the per-layer launches of a backward stage (the reference: autograd's per-layer convolution-backward-weight calls behind
 * train.py:443 / :448).  `tables`: device scratch of VK_WGRAD_BATCH_TABLE_BYTES, filled (synchronously) by the call; dw[l] += result.
 * The call waits for `stream` (hipStreamSynchronize) before it refills `tables`, so the same tables / workspace may be passed to
 * consecutive calls; buffers shared with work on OTHER streams are the caller's to order. */
#define VK_WGRAD_BATCH_TABLE_BYTES (128u << 10)
int vk_conv_wgrad_batch_supports(const vk_conv_desc* d);
int vk_conv_wgrad_batch(const vk_conv_desc* descs, const void* const* dz, float* const* dw, int n, int workgroups, void* tables,
                        size_t tables_bytes, void* workspace, size_t workspace_bytes, void* stream);
int vk_stem_wgrad(vk_dtype dtype, int N, int H, int W, const void* x4, const void* dz, float* dw_krsc3, void* workspace,
                  size_t workspace_bytes, void* stream);
/* The same with the stem BatchNorm's backward apply folded in (16-bit types; VK_ERR_UNSUPPORTED otherwise: run vk_bn_bwd_apply +
 * vk_stem_wgrad): g = the masked upstream gradient (what vk_maxpool_bwd_bn_reduce stored), z = the stem convolution's output,
 * coef_abc = [3][64] from vk_bn_bwd_coeffs; the kernel forms dz = a*g + b*z + c while it stages its operand — the stem has no data
 * gradient, so dz has no other reader and the 3-tensor apply pass (reference: autograd's batch_norm backward node behind
 * train.py:448 -> encoder.bn1) disappears. */
int vk_stem_wgrad_bn(vk_dtype dtype, int N, int H, int W, const void* x4, const void* g, const void* z, const float* coef_abc,
                     float* dw_krsc3, void* workspace, size_t workspace_bytes, void* stream);
/* The stem weight gradient for a model of cin input channels, 1 <= cin <= 4 (anything else: VK_ERR_ARG before any launch): dw is KRSC
 * [64][7][7][cin], the columns of x4's channels >= cin are dropped in the epilogue; the partial results in `workspace` are
 * 64 * 49 * cin floats each.  vk_stem_wgrad / vk_stem_wgrad_bn are cin = 3 of these (the same code, the same bits). */
int vk_stem_wgrad_c(vk_dtype dtype, int N, int H, int W, int cin, const void* x4, const void* dz, float* dw_krsc, void* workspace,
                    size_t workspace_bytes, void* stream);
int vk_stem_wgrad_bn_c(vk_dtype dtype, int N, int H, int W, int cin, const void* x4, const void* g, const void* z, const float* coef_abc,
                       float* dw_krsc, void* workspace, size_t workspace_bytes, void* stream);
/* BatchNorm-backward apply + data gradient + weight gradient of one small-channel convolution in ONE pass over its tensors: 16-bit
 * types, 3x3 stride 1 pad 1, one source: up = 0 with (src0.C, K) = (16, 16) or (32, 32), or up = 1 (nearest x2) with (src0.C, K) =
 * (32, 16) and H, W even; VK_ERR_UNSUPPORTED for everything else (fp32, odd H or W and every other upsampled shape included) before any
 * launch — run vk_bn_bwd_apply, vk_conv_dgrad_fused and vk_conv_wgrad then.
 * d_fwd: the layer's FORWARD descriptor (src0 = its input z1 with scale / shift / relu).  g: the masked upstream gradient, z: the layer's
 * own convolution output, both [N][H][W][K]; coef_abc = [3][K] from vk_bn_bwd_coeffs / _frozen: the kernel forms
 * dz = a*g + b*z + c (vk_bn_bwd_apply's fp32 expression, rounded to the element type) in LDS and never stores it.  w_dgrad: what
 * vk_conv_dgrad_fused takes for this layer.  y [N][H][W][C] receives g1 = dgrad(dz) * [bn(z1) > 0], bit for bit what vk_bn_bwd_apply +
 * vk_conv_dgrad_fused store; with up = 1 the source z1 and y are [N][H/2][W/2][32] and g1 is the 2x2-pooled data gradient (what
 * vk_conv_dgrad_fused with pool2 stores); bnr: z = d_fwd->src0.ptr, scale, shift, sums as for vk_conv_dgrad_fused, mask NULL, accumulate 0.
 * dw [K][3][3][C] += the weight gradient; workspace (required, 16-byte aligned, VK_WGRAD_WORKSPACE_BYTES is always enough) holds one
 * partial result per workgroup, added in a fixed order: the same bits on every run. */
int vk_conv_bwd_onepass(const vk_conv_desc* d_fwd, const void* g, const void* z, const float* coef_abc, const void* w_dgrad, void* y,
                        const vk_bnr* bnr, float* dw, void* workspace, size_t workspace_bytes, void* stream);
/* Data gradient of the stem, i.e. the gradient of the model's input: dx fp32 NCHW [N][3][H][W] is WRITTEN (not accumulated) from
 * dz [N][H/2][W/2][64] (activation dtype) and the fp32 KRSC stem weight w [64][7][7][3].  coef_abc NULL: g is dz.  Otherwise g is the
 * masked upstream gradient, z the stem convolution's output and coef_abc = [3][64] (vk_bn_bwd_coeffs / _frozen): the kernel forms
 * dz = a*g + b*z + c while it loads its operand.  H % 8 == 0, W % 32 == 0. */
int vk_stem_dgrad(vk_dtype dtype, int N, int H, int W, const void* g, const void* z, const float* coef_abc, const float* w_krsc3,
                  float* dx, void* stream);
/* The same for cin input channels, 1 <= cin <= 4 (anything else: VK_ERR_ARG before any launch): w is KRSC [64][7][7][cin], dx fp32 NCHW
 * [N][cin][H][W].  The 2 x 2 pixels x cin channels of an output block are columns uv * cin + c of the 16-wide tile (four channels fill
 * it); a column's sum does not depend on where it sits.  vk_stem_dgrad is cin = 3. */
int vk_stem_dgrad_c(vk_dtype dtype, int N, int H, int W, int cin, const void* g, const void* z, const float* coef_abc, const float* w_krsc,
                    float* dx, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The steps either side of model(x) in the inference wrappers, one fused pass each.
 * The caller decides the geometry (the reference has two conventions: image in the top-left corner with
 * scale = min(S/h, S/w), infer_pth_gui.py:17-24; image centred with scale = min(S/max(h,w), 1),
 * ui_infer_quadrilateral.py:197-216) and passes it in the descriptor; the library does the pixel work with
 * cv2.resize's arithmetic (8-bit INTER_LINEAR in 11-bit fixed point, float INTER_LINEAR, INTER_NEAREST).
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int h, w;             /* original image size */
  int src_stride;       /* bytes per row of the original BGR image (>= 3*w); unused by the post-processing calls */
  int size;             /* side S of the square network input / logit map */
  int nh, nw;           /* size of the resized image inside the square */
  int top, left;        /* its position inside the square */
  int pad_value;        /* border value 0..255, applied before the normalisation */
} vk_letterbox_desc;

/* uint8 BGR [h][w][3] (device) -> float32 [3][S][S] RGB planes, ((v/255) - mean) / std with the ImageNet constants */
int vk_letterbox_preprocess(const vk_letterbox_desc* d, const uint8_t* bgr, float* x_nchw, void* stream);
/* logits [S][S] -> uint8 [h][w] in {0,255}: (sigmoid >= thresh), crop, INTER_NEAREST back to the original size.
 * The comparison is >=: a sigmoid exactly on the threshold is foreground (a zero logit at 0.5; every logit from 17 up at 1.0, where
 * the float32 sigmoid is exactly 1; every logit at 0.0).  vk_seg_metrics below uses the strict >, as the reference's metrics do.
 * A NaN logit is background at every threshold (NaN >= t is false); +-inf give sigmoid 1 / 0.
 * mask_hw needs no alignment: rows are stored as 32-bit words only when w % 4 == 0 and mask_hw is 16-byte aligned, bytes otherwise. */
int vk_letterbox_postprocess_mask(const vk_letterbox_desc* d, const float* logits, float thresh, uint8_t* mask_hw, void* stream);
/* logits [S][S] -> float32 [h][w] in [0,1]: sigmoid, crop, INTER_LINEAR back to the original size (copy when equal), clip.
 * A NaN logit gives NaN in every output pixel one of whose four taps reads it, also where that tap's weight is 0 (NaN * 0), as
 * numpy's arithmetic and np.clip give: the clip keeps a NaN, it does not turn it into 0.  Small and large outputs take two kernels
 * that evaluate the same expression: the same bits.  prob_hw needs 4-byte alignment only (16-byte stores when it has it and w % 4 == 0). */
int vk_letterbox_postprocess_prob(const vk_letterbox_desc* d, const float* logits, float* prob_hw, void* stream);
/* The same for a C-class logit map [C][S][S] (fp32 class planes, 1 <= C <= 16), same descriptor and arithmetic; with C == 1 the mask
 * and multi-label probability calls give the bits of the two calls above.
 * labels: argmax over the classes at the model's resolution (ties to the lowest index), crop, INTER_NEAREST -> uint8 [h][w]
 * masks:  per class (sigmoid >= thresh) * 255, crop, INTER_NEAREST -> uint8 [C][h][w]
 * probs:  mode VK_LOSS_MULTILABEL: per-class sigmoid; VK_LOSS_MULTICLASS (C >= 2): softmax over the classes (shift by the max, expf,
 *         sum in class order, divide) at each source pixel; then crop, INTER_LINEAR (copy when equal), clip -> fp32 [C][h][w] */
int vk_letterbox_postprocess_labels(const vk_letterbox_desc* d, int C, const float* logits, uint8_t* labels_hw, void* stream);
int vk_letterbox_postprocess_mask_multi(const vk_letterbox_desc* d, int C, const float* logits, float thresh, uint8_t* masks_chw,
                                        void* stream);
int vk_letterbox_postprocess_prob_multi(const vk_letterbox_desc* d, int C, int mode, const float* logits, float* probs_chw, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Sliding-window inference at the image's own resolution, with D4 test-time augmentation: the uint8 image is cut into
 * overlapping T x T tiles on the device, every tile in 1, 2, 4 or 8 views, and the per-tile logits are blended back into one map.
 * Grid, per axis of length L with stride s = T - overlap: n = 1 if L <= T else ceil((L - T) / s) + 1 origins,
 * origin[i] = min(i * s, max(L - T, 0)) (the last tile is pulled back flush with the edge; padding only where L < T).  Tile index
 * t = iy * nx + ix.  View v = 4*tr + 2*fy + fx of a tile A: A_v[i][j] = A[i0][j0] with (a, b) = tr ? (j, i) : (i, j),
 * i0 = fy ? T-1-a : a, j0 = fx ? T-1-b : b.  view_mask is 0x01 (no augmentation), 0x03 (+ horizontal flip), 0x0f (the four flips) or
 * 0xff (all of D4); the views of a tile are stored in ascending v.
 * Both calls check the descriptor on the host first (VK_ERR_ARG and the error string: sizes, 0 <= overlap <= T/2, at most
 * VK_TILE_MAX_ORIGINS origins per axis and exactly those of the rule above, the view mask), before anything touches the stream or the
 * outputs.
 * ---------------------------------------------------------------------------------------------- */
#define VK_TILE_MAX_ORIGINS 64
#define VK_TILE_MAX_SIDE 4096
#define VK_BLEND_PROB 0
#define VK_BLEND_LOGIT 1
typedef struct {
  int h, w;             /* image size */
  int src_stride;       /* bytes per row of the BGR image (>= 3*w); unused by the blend */
  int T;                /* tile side, 1..VK_TILE_MAX_SIDE */
  int overlap;          /* 0..T/2 */
  int ny, nx;           /* origins per axis */
  int ys[VK_TILE_MAX_ORIGINS], xs[VK_TILE_MAX_ORIGINS];
  int view_mask;        /* bit v set = view v present */
  int pad_value;        /* value 0..255 of the pixels outside the image, applied before the normalisation; unused by the blend */
  int C;                /* logit planes per tile, 1..16; unused by the pre-processing */
} vk_tile_desc;

/* uint8 BGR [h][w][3] (device) -> float32 [ntiles*nviews][3][T][T] (tile major, view minor): view map, source pixel or pad_value,
 * BGR->RGB, ((v/255) - mean) / std with the expressions of vk_letterbox_preprocess (the same bits) */
int vk_tile_preprocess(const vk_tile_desc* d, const uint8_t* bgr, float* x, void* stream);
/* logits fp32 [ntiles*nviews][C][T][T] -> out_chw fp32 [C][h][w] and / or mask_chw uint8 {0,255} [C][h][w] (one of them may be NULL).
 * Per pixel and plane, in this order: the covering tiles in ascending t; per tile q = (1/nviews) * (sum over ascending v of f(logit at
 * the view's image of the pixel)); a pixel in exactly one tile takes q, otherwise acc += w*q, wsum += w and the value is acc / wsum
 * with w = w1(ty) * w1(tx), w1(t) = (float)min(t+1, T-t, R) / (float)R, R = overlap (1 when overlap is 0).  No atomics, no fused
 * multiply-add: the result does not depend on the launch.
 * mode VK_BLEND_PROB: f = sigmoid, value clipped to [0,1], mask = value >= thresh.  VK_BLEND_LOGIT: f = identity (the blended raw
 * logits: the mode for multi-class models, whose softmax stays with the caller), mask = sigmoid(value) >= thresh. */
int vk_tile_blend(const vk_tile_desc* d, int mode, const float* logits, float thresh, float* out_chw, uint8_t* mask_chw, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Geometry post-processing of batched probability maps: what the reference's GUIs do with
 * Segmenter.infer's output to obtain the indentation diagonals — ui_infer_rectangle.py:291-381 postprocess_minarearect_multi
 * (steps 1-3 are shared by ui_infer_quadrilateral.py:446-490): (prob >= bin_thresh) -> morphologyEx OPEN, CLOSE with the
 * MORPH_ELLIPSE k x k element -> 8-connected components, area >= min_area -> per component the minimum-area enclosing rectangle
 * (cv2.minAreaRect + boxPoints + astype(int32)) -> the two diagonals.  All steps run on the device for `batch` maps of one size.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int h, w;             /* size of every probability map (h <= 4096) */
  float bin_thresh;     /* BIN_THRESH: 0.50 (rectangle GUI) / 0.45 (quadrilateral GUI); compared in float32 */
  int morph_kernel;     /* MORPH_KERNEL: odd 1..7, side of the MORPH_ELLIPSE element (3 = cross); 1 = no morphology */
  int open_iter;        /* OPEN_ITER */
  int close_iter;       /* CLOSE_ITER */
  int min_area;         /* max(200, int(MIN_AREA_FRAC * h * w)) in the reference (ui_infer_rectangle.py:322) */
  int max_components;   /* capacity of the per-map detection list, 1..4096 (further kept components stay in `clean` and in `counts`) */
} vk_geom_desc;
/* Limits: h 1..4096, w 1..16384, h * w < 2^30, open_iter / close_iter 0..16 (ignored when morph_kernel is 1), min_area >= 1.  A map
 * of one row, one column or one pixel is valid.  Pixels outside the map never win an erosion or a dilation.  NaN compares as
 * background, +-0 as foreground only for bin_thresh <= 0; denormal probabilities are compared as they are. */

typedef struct {
  int label;            /* connected-component id as cv2 / scipy number them: 1 + raster rank of the component's first pixel */
  int area;             /* pixels */
  int box[8];           /* x0,y0 .. x3,y3: rectangle corners truncated to int32 (order around the rectangle; not TL/TR/BR/BL) */
  float cx, cy;         /* rectangle centre */
  float rw, rh;         /* side lengths: along the supporting hull edge / across it */
  float ux, uy;         /* unit direction of that edge */
  int hull_n;           /* convex-hull vertices of the component (strictly convex ones; 1 for one pixel, 2 for a straight one-pixel line) */
  int reserved;         /* written as 0 */
  double d1, d2, d_mean;/* diagonals of the int32 box (longest pair first) and their mean, float64 as numpy computes them */
} vk_geom_det;

int64_t vk_geom_workspace_bytes(const vk_geom_desc* d, int batch);      /* < 0: bad descriptor */
/* prob: float32 [batch][h][w] in [0,1] (device).  clean: uint8 [batch][h][w] in {0,255}.  dets: [batch][max_components], filled in
 * label order (the host sorts by area like ui_infer_rectangle.py:379).  counts: int32 [batch] = kept components per map.
 *
 * counts[b] is the number of components with area >= min_area, also when it exceeds max_components: then the list holds the first
 * max_components of them in label order (raster order of each component's first pixel) and `clean` still shows all of them.  Only the
 * slots 0 .. min(counts[b], max_components) - 1 of a map are written; every byte of the slots above, and nothing outside `clean`,
 * `dets`, `counts` and the first vk_geom_workspace_bytes() bytes of the workspace, is left as the caller had it.  The workspace need
 * not be cleared.
 *
 * Degenerate hulls.  One pixel (hull_n 1): all four corners are the pixel, cx, cy its coordinates, rw = rh = 0, (ux, uy) = (1, 0),
 * d1 = d2 = d_mean = 0.  Two hull vertices (hull_n 2, a straight one-pixel line): the rectangle on the segment from the top-most (then
 * left-most) vertex to the other one: (ux, uy) its unit direction, rw its length, rh the float32 residue of projecting the two points
 * on the normal (0, or a few 1e-6 on a diagonal), corners 0/3 and 1/2 coincide up to that residue, and d1, d2 are the distances of the
 * truncated corner pairs as for any other box (for a horizontal or vertical line both equal its length).  The corners are truncated,
 * not rounded: an end point that comes out as 8.999999 is stored as 8. */
int vk_geom_minarearect(const vk_geom_desc* d, int batch, const float* prob, uint8_t* clean, vk_geom_det* dets, int* counts,
                        void* workspace, size_t workspace_bytes, void* stream);

/* The newer GUI's post-processing (ui_infer_quadrilateral.py:423-530 `postprocess_minarearect_multi` with its helpers :262-420):
 * steps 1-3 as above (bin_thresh 0.45 there), then per kept component: dilate by the (2 fit_outset_px + 1)^2 MORPH_ELLIPSE element
 * (fit only: `clean` and `area` are untouched), external border (cv2.findContours RETR_EXTERNAL / CHAIN_APPROX_SIMPLE), convex hull,
 * cv2.approxPolyDP epsilon bisection to exactly four vertices on both polygons, the sub-sampling and extreme-point fall-backs,
 * (quality, area) ranking of the candidates, clockwise ordering, int32 corners and the two diagonals. */
typedef struct {
  int label;            /* as vk_geom_det */
  int area;             /* pixels of the component (before the fit dilation) */
  int box[8];           /* x0,y0 .. x3,y3: the quadrilateral, ordered by _order_quad_cw (:266-277), starting at its top-most corner */
  float cx, cy;         /* mean of the four corners */
  int valid;            /* 0: no quadrilateral was found (the reference drops such a component from its list) */
  int branch;           /* which step produced the candidates: 1 epsilon bisection, 2 four consecutive vertices of the 1 % polygon, 3 extreme points */
  int n_candidates;
  int contour_n;        /* points of the CHAIN_APPROX_SIMPLE border */
  int hull_n;           /* convex-hull vertices of the dilated component */
  int flags;            /* 0 on an ordinary component; see below */
  double quality;       /* _quad_quality of the chosen candidate */
  double d1, d2, d_mean;
} vk_geom_quad;

/* flags.  Bit 0 (1): the CHAIN_APPROX_SIMPLE border has more than 16,384 points.  contour_n still reports the full length; the
 *   border polygon is left out of the epsilon bisection and of the sub-sampling, while the hull's bisection, the hull's sub-sampling
 *   and the extreme points run as usual: the fit is robust_quadrilateral_from_contour with the hull as its only polygon, and
 *   n_candidates counts what that produced.
 * Bit 1 (2): the hull has more than 4,096 vertices; the hull is left out in the same way (with both bits set nothing is fitted).
 * Bit 2 (4): border following was stopped (more than 2^21 steps, or no neighbour found); handled as bit 0.
 * A component whose border has fewer than four points (one pixel, a straight one-pixel line without outset) is reported with
 * valid = 0, branch = 0, n_candidates = 0, a zero box, and its label, area, contour_n and hull_n; so is one for which no step yields
 * a quadrilateral of area > 10 (branch 0 = none).  counts, the slots that are written and the buffers are as for vk_geom_minarearect. */
/* as vk_geom_minarearect (same workspace size: vk_geom_workspace_bytes); fit_outset_px 0..3 (reference default 2) */
int vk_geom_quadrilateral(const vk_geom_desc* d, int fit_outset_px, int batch, const float* prob, uint8_t* clean, vk_geom_quad* dets,
                          int* counts, void* workspace, size_t workspace_bytes, void* stream);

/* The label map of the latest geometry call, as slots of its detection list.
 *
 * Contract: after vk_geom_minarearect or vk_geom_quadrilateral returns, the workspace holds the flattened label image and the slot of
 * every component's representative, and neither call writes them after its labelling front end.  They stay valid until the next call
 * that is given the same workspace.  This call reads the workspace exactly as that latest call left it: the descriptor, `batch` and
 * the stream must be the same as in that call (the same stream orders it after the kernels that fill the workspace).  It writes
 * nothing but `slots`, device int32 [batch][h][w]:
 *   s >= 0   the pixel belongs to the component in slot s of that map's detection list (slots are in label order, the order in which
 *            `dets` is filled), so slot s covers exactly dets[s].area pixels;
 *   -1       background, or a component with area < min_area (absent from `clean`);
 *   -2       a kept component beyond max_components: it shows in `clean` and in `counts` but has no record.
 * A workspace that no geometry call has filled gives a meaningless map, never an access outside the buffers. */
int vk_geom_slot_map(const vk_geom_desc* d, int batch, const void* workspace, size_t workspace_bytes, int32_t* slots, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Training-time augmentation on the device: VickersDataset.__getitem__ (train.py:173-200) with the
 * albumentations pipeline of train.py:67-113.  The dataset is letterboxed ONCE into uint8 tensors that stay in HBM
 * (vk_letterbox_u8 / vk_letterbox_mask_u8: LongestMaxSize + PadIfNeeded, train.py:70-75, geometry in the descriptor); every
 * step vk_augment_batch turns n dataset items + n sets of random draws (made by the host, as albumentations makes them) into
 * the network input x float32 [n][3][S][S] and target y float32 [n][1][S][S] in one fused pass.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int d4;               /* OneOf(flips, rot90), train.py:81-85: 0 none, 1 HorizontalFlip, 2 VerticalFlip, 3 + k = np.rot90(k), k = 0..3 */
  int rotate;           /* Rotate(limit=180, BORDER_CONSTANT), train.py:89: 1 = applied */
  float cos_a, sin_a;   /* of the angle (counter-clockwise, cv2.getRotationMatrix2D about (S/2 - 0.5, S/2 - 0.5)) */
  int photo;            /* OneOf, train.py:96-100: 0 none, 1 RandomBrightnessContrast, 2 CLAHE, 3 GaussianBlur */
  float alpha, beta;    /* RandomBrightnessContrast: v' = trunc(clip(v * alpha + beta * 255, 0, 255)) */
  int blur_ksize;       /* GaussianBlur: 3 or 5 (sigma 0 -> cv2's binomial kernels), BORDER_REFLECT_101 */
  float noise_scale;    /* GaussNoise, train.py:104: sigma / 65536 on the 0..255 scale; 0 = not applied */
  uint32_t noise_seed;  /* seed of the counter-based noise field of this sample */
  int clahe_limit;      /* CLAHE, train.py:98: OpenCV's integer clip limit max(1, int(clip * (S/8)^2 / 256)), clip ~ U(1, 2) */
} vk_aug_params;

/* CLAHE works on the L channel of an 8-bit RGB <-> L*a*b* conversion done in integer fixed point through three tables the
 * host builds once (vickers-hardness-unet_amd/augment.py: color_tables) and keeps on the device as int32 [VK_AUG_TABLE_INTS]:
 * LIN [256] sRGB decode x 4096 | FT [4097] Lab f(t / 4096) x 32768 | ENC [4097] sRGB encode of lin / 4096. */
#define VK_AUG_TABLE_INTS (256 + 4097 + 4097)
/* bytes of scratch vk_augment_batch needs for n samples when any of them draws CLAHE: per sample the geometric result as
 * L, a, b, mask uint8 [S][S][4] and the 8 x 8 tile LUTs uint8 [64][256] */
size_t vk_augment_workspace_bytes(int n, int size);

/* uint8 BGR [h][w][3] -> uint8 RGB [S][S][3]: cv2.resize(INTER_LINEAR) to nh x nw at (top, left), constant border */
int vk_letterbox_u8(const vk_letterbox_desc* d, const uint8_t* bgr, uint8_t* rgb_sq, void* stream);
/* uint8 mask [h][w] (row stride d->src_stride bytes) -> {0,1} [S][S]: (m > 0), cv2.resize(INTER_NEAREST), border 0 (pad_value is not
 * used).  Both calls read w (3 * w) bytes of a row and never its padding up to src_stride; a descriptor with nh or nw below 1 (a 1 x 50
 * image at size 8 under the train convention) is VK_ERR_ARG before any launch. */
int vk_letterbox_mask_u8(const vk_letterbox_desc* d, const uint8_t* mask_hw, uint8_t* mask_sq, void* stream);
/* images_rgb uint8 [n_items][S][S][3], masks uint8 [n_items][S][S] in {0,1} (device); index_dev int32 [n] (device): the dataset
 * item of every sample; params_host [n]: validated on the host, then copied to params_dev (device scratch, n * sizeof).
 * color_tables (device, int32 [VK_AUG_TABLE_INTS]) and workspace (device, vk_augment_workspace_bytes(n, size)) are needed only
 * when a sample has photo == 2 and may be null otherwise; CLAHE needs size % 8 == 0 (8 x 8 tiles without padding).
 * index_dev[i] is clamped to 0 .. n_items - 1 on the device: an index below 0 gives item 0, one above the store its last item, the
 * same bits as that item asked for by its own index; nothing outside the store is read.
 * workspace: written only when a sample has photo == 2, and then only inside sample i's own slot of
 * vk_augment_workspace_bytes(1, size) bytes at i times that size, for the samples that drew CLAHE; every byte read is written first by
 * the same call, so its previous contents never reach the result and it need not be cleared.  x and y are written in full
 * (n * 3 * size * size and n * size * size floats), nothing either side of them. */
int vk_augment_batch(int n, int size, int n_items, const uint8_t* images_rgb, const uint8_t* masks, const int* index_dev,
                     const vk_aug_params* params_host, void* params_dev, const int* color_tables, void* workspace,
                     size_t workspace_bytes, float* x, float* y, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Native-resolution patch training: the training-side half of the sliding-window inference above.  The images stay
 * on the device at their OWN size — uint8 BGR [h][w][3], concatenated in one store, every item starting on a multiple of 4 bytes and
 * padded to one; masks [h][w] in a second store (any non-zero byte is foreground) — and every step cuts n random S x S patches out of
 * them into the uint8 RGB [n][S][S][3] / mask {0,1} [n][S][S] buffers that vk_augment_batch then reads with index = 0..n-1.
 * Every byte offset is 64-bit: the store may exceed 2^31 bytes.
 *
 * Origin of a sample (int32 (y0, x0), the patch's top-left corner in source pixels).  With k >= 0 and a non-empty mask: k is clamped
 * to count - 1, (py, px) is the k-th foreground pixel of the item in raster order, and (y0, x0) = (py - oy, px - ox); otherwise
 * (y0, x0) = (oy, ox).  Then per axis of length L: L >= S: o = min(max(o, 0), L - S); L < S: o = -((S - L) / 2) (integer division: the
 * image centred in the patch, as PadIfNeeded centres it).
 * Crop, float32 without fused multiply-add, for output pixel (y, x): c = S*0.5f - 0.5f, dx = x - c, dy = y - c, cx = (float)x0 + c,
 * cy = (float)y0 + c, u = ((cos*dx - sin*dy) * zoom) + cx, v = ((sin*dx + cos*dy) * zoom) + cy.  Image: the four bilinear taps at
 * (floor(v), floor(u)) combined as vk_augment_batch's rotation combines them (top = t00*(1-wx) + t01*wx, bot likewise,
 * top*(1-wy) + bot*wy), taps outside the IMAGE read 0, rintf, clamp to 0..255, BGR -> RGB.  Mask: nearest, at
 * (floor(v + 0.5f), floor(u + 0.5f)), 0 outside.  A sample with cos == 1, sin == 0, zoom == 1 is copied row by row instead; the bits are
 * the same (every coordinate is then an exact integer or half-integer below 2^23); VK_PATCH_FORCE_GENERAL sends it down the general path.
 * ---------------------------------------------------------------------------------------------- */
typedef struct {
  int64_t img_off;      /* byte offset of the item's BGR pixels in the image store, a multiple of 4 */
  int64_t msk_off;      /* byte offset of its mask in the mask store, a multiple of 4 */
  int h, w;             /* 1..16384 */
  int64_t row_off;      /* index of its first entry in the row table (h entries) */
} vk_patch_item;

typedef struct {
  int item;             /* 0..n_items-1 */
  int k;                /* foreground rank, or < 0: (oy, ox) is the origin itself */
  int oy, ox;           /* k >= 0: where in the patch the chosen pixel lands, 0..S-1; k < 0: the origin (before clamping); 0..16384 */
  float zoom;           /* source pixels per output pixel, 0.25..4 */
  float cos_a, sin_a;   /* rotation about the patch centre, as vk_aug_params */
  int reserved;         /* 0 */
} vk_patch_params;

#define VK_PATCH_FORCE_GENERAL 1

/* Once per dataset: checks items_host[n_items] (sizes, alignment, every item — its image padded to whole dwords — inside images_bytes /
 * masks_bytes / rowcum_len; VK_ERR_ARG before anything touches the stream), copies the table to items_dev (device,
 * n_items * sizeof(vk_patch_item)) and fills rowcum (device, int32): rowcum[row_off + r] = foreground pixels of rows 0..r of the item,
 * so rowcum[row_off + h - 1] is its total.  Integer sums only: deterministic.  masks must be 4-byte aligned. */
int vk_patch_index(int n_items, const vk_patch_item* items_host, void* items_dev, size_t images_bytes, const uint8_t* masks,
                   size_t masks_bytes, int32_t* rowcum, size_t rowcum_len, void* stream);
/* Per step: checks on the host (n 1..65535, size 1..16384, every item in range, zoom in [0.25, 4], |cos^2 + sin^2 - 1| < 1e-3, offsets,
 * flags, no null buffer, images 4-byte aligned; VK_ERR_ARG before anything touches the stream), copies params_host[n] to params_dev
 * (device scratch, n * sizeof), then writes origins int32 [n][2] (device; readable by the caller), patches_rgb and patches_mask.
 * items_dev and rowcum are those vk_patch_index filled. */
int vk_patch_batch(int n, int size, int n_items, const void* items_dev, const uint8_t* images, const uint8_t* masks, const int32_t* rowcum,
                   const vk_patch_params* params_host, void* params_dev, int flags, int32_t* origins, uint8_t* patches_rgb,
                   uint8_t* patches_mask, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Instance copy-paste: a compose step between the letterboxed uint8 store of vk_letterbox_u8 / _mask_u8 and
 * vk_augment_batch.  All arithmetic is integer: the results are bytes a numpy restatement gives again (tests/copypaste_ref.py).
 *
 * vk_cp_boxes: slots int32 [batch][h][w] as vk_geom_slot_map writes it -> boxes int32 [batch][max_slots][5] = x0, y0, x1, y1
 * (inclusive), area of every slot 0 <= s < max_slots; an empty slot gives (w, h, -1, -1, 0).  Negative slots and slots >= max_slots
 * are ignored.  The call initialises boxes itself.  Per wave, then per workgroup (LDS), then integer min / max / add atomics on
 * boxes: no order to depend on.  batch 1..65535, h, w 1..16384, max_slots 1..256.
 *
 * vk_cp_alpha: kept = (slot >= 0) and alpha, uint8 [batch][h][w] each.  acc = sum over dy, dx in -3..3 of b[dy] b[dx] kept(y + dy,
 * x + dx), b = (1, 6, 15, 20, 15, 6, 1), taps outside the map 0, so acc is in 0..4096; alpha = min(255, (acc * 2040 + 2048) >> 12): a
 * gain of 8 — 255 from one eighth of the full sum on, 0 beyond Chebyshev distance 3 of every kept pixel.
 *
 * vk_cp_paste: the stores are uint8, images_rgb [n_items][S][S][3] and masks, kept, alpha [n_items][S][S] (masks in {0, 1}).  Sample k
 * of n starts as a copy of item base_index_dev[k] (device int32 [n], clamped to the store as vk_augment_batch clamps its index) and
 * takes the counts_host[k] <= VK_CP_MAX_PASTES records recs_host[k][0 ..] in list order (recs_host: host [n][VK_CP_MAX_PASTES], every
 * entry readable).  recs_dev: device scratch of VK_CP_RECS_DEV_BYTES(n), 4-byte aligned: the records, then the counts.
 *   T = rot90(P[:, ::-1] if d4 & 4 else P, d4 & 3) (counter-clockwise quarter turns, numpy's rot90) of the donor box P of a map of
 *   item `donor`, th x tw.  For column i and row j of the destination box: U = ((2 i + 1) * tw * 256) / (2 dw) - 128 clipped to
 *   [0, (tw - 1) * 256], V likewise from j, th, dh; x0 = U >> 8, fx = U & 255, x1 = min(x0 + 1, tw - 1), y alike.  Per colour channel and
 *   for alpha: top = p00 (256 - fx) + p01 fx, bot = p10 (256 - fx) + p11 fx, val = (top (256 - fy) + bot fy + 32768) >> 16.
 *   k = T_kept[min((V + 128) >> 8, th - 1)][min((U + 128) >> 8, tw - 1)].  Then, a being the alpha value, per channel
 *   cur = (a val + (255 - a) cur + 127) / 255 and m |= k.  Pixels of the box outside the image are dropped.
 * Every pixel of out_rgb [n][S][S][3] and out_mask [n][S][S] is written exactly once and depends on the stores alone: no atomics, no
 * workspace but recs_dev.  Host checks (VK_ERR_ARG before anything touches the stream): n 1..65535, S 1..4096, n_items >= 1, no null
 * buffer, stores / outputs / recs_dev 4-byte aligned, counts in 0..VK_CP_MAX_PASTES, and per used record: donor in 0..n_items-1, the
 * donor box inside [0, S) with sw, sh >= 1, d4 in 0..7, dw, dh in 1..2S, dx0, dy0 in [-2S, 2S].
 * ---------------------------------------------------------------------------------------------- */
#define VK_CP_MAX_PASTES 8
#define VK_CP_MAX_SLOTS 256
#define VK_CP_MAX_SIDE 4096
typedef struct vk_cp_rec {
  int32_t donor;                /* item of the stores the instance is taken from */
  int32_t sx0, sy0, sw, sh;     /* donor box */
  int32_t d4;                   /* bit 2: mirror the columns first; bits 0-1: counter-clockwise quarter turns */
  int32_t dx0, dy0, dw, dh;     /* destination box; may leave the image */
} vk_cp_rec;
#define VK_CP_RECS_DEV_BYTES(n) ((size_t)(n) * (VK_CP_MAX_PASTES * sizeof(vk_cp_rec) + sizeof(int32_t)))
int vk_cp_boxes(int batch, int h, int w, const int32_t* slots, int max_slots, int32_t* boxes, void* stream);
int vk_cp_alpha(int batch, int h, int w, const int32_t* slots, uint8_t* kept, uint8_t* alpha, void* stream);
int vk_cp_paste(int n, int S, int n_items, const uint8_t* images_rgb, const uint8_t* masks, const uint8_t* kept, const uint8_t* alpha,
                const int32_t* base_index_dev, const int32_t* counts_host, const vk_cp_rec* recs_host, void* recs_dev, uint8_t* out_rgb,
                uint8_t* out_mask, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Synthetic micrographs: scenes of Vickers indentations rendered on the device into uint8 pixels [n][S][S][3] and a
 * {0, 1} mask [n][S][S] — the buffers vk_augment_batch reads.  A scene is one fixed-layout record set per image; all geometry is
 * fixed point, 1/16 pixel, int32, the centre of pixel (x, y) being (16 x, 16 y).  All arithmetic is integer: the outputs are the bytes
 * tests/micrographs_ref.py gives again.  Formulas (>> is the arithmetic shift, / the division of non-negative integers):
 *   mix(h): h ^= h >> 16; h *= 0x7feb352d; h ^= h >> 15; h *= 0x846ca68b; h ^= h >> 16 (uint32).
 *   Background level of pixel (x, y), any integers:  L = base + ((grad_x (x - grad_cx) + grad_y (y - grad_cy)) >> 8)
 *     - ((vig ((x - vig_cx)^2 + (y - vig_cy)^2)) >> 16) + T,  T = ((val - 128) tex_amp) >> 8, val the bilinear lattice noise:
 *     u = x tex_cos + y tex_sin, v = y tex_cos - x tex_sin (Q14); iu = u >> (14 + tex_lu), fu = (u >> (6 + tex_lu)) & 255, iv, fv
 *     alike with tex_lv; g(i, j) = mix(i * 0x9E3779B1 + j * 0x85EBCA77 + tex_seed) & 255;
 *     val = ((g(iu, iv) (256 - fu) + g(iu + 1, iv) fu) (256 - fv) + (g(iu, iv + 1) (256 - fu) + g(iu + 1, iv + 1) fu) fv + 32768) >> 16.
 *   Scratches, in list order: with q = (16 x - s.x, 16 y - s.y), c = q.x s.dy - q.y s.dx, t = q.x s.dx + q.y s.dy: the pixel is
 *     covered iff c^2 <= hw^2 (dx^2 + dy^2) and t0 <= t <= t1; L += depth.
 *   Blobs: d2 = |q|^2 from the centre; if d2 < r^2: L -= (dark min(256, (r^2 - d2) / (r^2 >> 8))) >> 8.
 *   Indentations, in list order, e_i = v_(i+1) - v_i, cr(a, b) = a.x b.y - a.y b.x:
 *     inside (the mask) iff cr(e_i, p - v_i) >= 0 for the four i.  Inside, the facet f is the one i with cr(v_i - a, p - a) >= 0 and
 *     cr(v_(i+1) - a, p - a) < 0 (p = a: facet 0); k = 256 cr(e_f, p - v_f) / cr(e_f, a - v_f) (0 at the edge, 256 at the apex);
 *     L = shade[f] + ((slope[f] k) >> 8) + (T >> 1), and L += ridge if for some i, with w = v_i - a, q = p - a:
 *     0 <= q.w <= |w|^2 and cr(w, q)^2 <= ridge_hw^2 |w|^2.
 *     Outside, when halo_r > 0: d2 = min over the edges of the squared distance to the segment (cr^2 / |e|^2 where the foot lies on
 *     it, else to the nearer end); if d2 < halo_r^2: L -= (halo_depth min(256, (halo_r^2 - d2) / (halo_r^2 >> 8))) >> 8.
 *   Channel c of the ideal image: clamp((L tint[c] + 128) >> 8, 0, 255).
 *   Optics: the separable binomial of radius blur_r (weights C(2 r, k), sum 4^r per axis) over the ideal image, which is defined
 *     beyond the frame by the same formulas; (acc + (16^r >> 1)) >> 4 r.  Then noise: h = mix(((y S + x) 3 + c) * 0x9E3779B1 +
 *     noise_seed), t = the sum of the four bytes of h - 510, value = clamp(value + ((t noise_amp + 128) >> 8), 0, 255).
 *   Rects, in list order, after blur and noise, never in the mask: pixels with x0 <= x <= x1, y0 <= y <= y1, all of them when
 *     thickness = 0, else those not inside (x0 + th .. x1 - th, y0 + th .. y1 - th); the colour replaces the pixel.
 * One launch; a workgroup owns a 64 x 16 tile, evaluates the ideal image over the tile and a 3-pixel apron in LDS, blurs out of LDS and
 * writes every output byte exactly once: no atomics, no workspace but scenes_dev (VK_MG_SCENES_DEV_BYTES(n), 4-byte aligned).
 * Host checks (VK_ERR_ARG before anything touches the stream): no null buffer, buffers 4-byte aligned, n 1..65535, S in
 * 16..VK_MG_MAX_SIDE, scenes_dev_bytes, every count within its limit, and per used record the ranges that keep every product inside
 * int64 (VK_MG_MAX_SIDE is the largest S for which they do): coordinates in [-VK_MG_COORD_MARGIN, 16 S + VK_MG_COORD_MARGIN], a
 * convex clockwise quadrilateral (cr(e_i, e_(i+1)) > 0, x to the right, y down), the apex strictly inside it, half widths and radii in
 * 0..32767 (a blob's and a non-zero halo's from 16), |dx|, |dy| <= 16384 and not both 0, levels in -1024..1024, gains 0..1024, vig and
 * noise_amp 0..255, tex_lu and tex_lv 0..8, |tex_cos|, |tex_sin| <= 16384, the gradient's and the vignette's centre in [-512, S + 512]
 * pixels, rect corners within +-4096 pixels, blur_r 0..3.
 * ---------------------------------------------------------------------------------------------- */
#define VK_MG_MAX_INDENTS 8
#define VK_MG_MAX_SCRATCHES 64
#define VK_MG_MAX_BLOBS 8
#define VK_MG_MAX_RECTS 4
#define VK_MG_MAX_SIDE 1024
#define VK_MG_MIN_SIDE 16
#define VK_MG_COORD_MARGIN 8192
typedef struct vk_mg_indent {
  int32_t vx[4], vy[4];         /* vertices, clockwise */
  int32_t ax, ay;               /* apex */
  int32_t shade[4], slope[4];   /* facet i lies between the apex and the edge v_i v_(i+1) */
  int32_t ridge, ridge_hw;      /* level added along the four apex-to-vertex segments, and their half width */
  int32_t halo_r, halo_depth;
  int32_t reserved[2];
} vk_mg_indent;
typedef struct vk_mg_scratch {
  int32_t x, y, dx, dy;         /* a point and the direction (Q14 cosines) */
  int32_t hw, depth;
  int32_t t0, t1;               /* extent along the direction, in units of 1/16 pixel times |d|; INT32_MIN / INT32_MAX: none */
} vk_mg_scratch;
typedef struct vk_mg_blob {
  int32_t x, y, r, dark;
} vk_mg_blob;
typedef struct vk_mg_rect {
  int32_t x0, y0, x1, y1;       /* whole pixels, inclusive */
  int32_t thickness;            /* 0: filled */
  int32_t color[3];
} vk_mg_rect;
typedef struct vk_mg_scene {
  int32_t n_indents, n_scratches, n_blobs, n_rects;
  int32_t base, tint[3];
  int32_t grad_x, grad_y, grad_cx, grad_cy;
  int32_t vig_cx, vig_cy, vig;
  int32_t tex_amp, tex_cos, tex_sin, tex_lu, tex_lv;
  uint32_t tex_seed;
  int32_t blur_r, noise_amp;
  uint32_t noise_seed;
  int32_t reserved[8];
  vk_mg_indent indents[VK_MG_MAX_INDENTS];
  vk_mg_scratch scratches[VK_MG_MAX_SCRATCHES];
  vk_mg_blob blobs[VK_MG_MAX_BLOBS];
  vk_mg_rect rects[VK_MG_MAX_RECTS];
} vk_mg_scene;
#define VK_MG_SCENES_DEV_BYTES(n) ((size_t)(n) * sizeof(vk_mg_scene))
size_t vk_mg_scenes_dev_bytes(int n);
int vk_mg_render(int n, int S, const vk_mg_scene* scenes_host, void* scenes_dev, size_t scenes_dev_bytes, uint8_t* rgb, uint8_t* mask,
                 void* stream);

/* ------------------------------------------------------------------------------------------------
 * Distance maps of masks: the exact squared Euclidean distance transform, the signed map of the boundary loss
 * (Kervadec et al., MIDL 2019), surface-distance statistics of a prediction against its label, and the boundary loss.  Distances are
 * integers: the results are the numbers a numpy restatement gives again (tests/boundary_ref.py).
 *
 * vk_edt_sq: src [batch][h][w], uint8 (foreground: != 0) or fp32 (foreground: v > thresh; thresh is ignored for uint8) ->
 * d2 int32 [batch][h][w] = min over the site pixels (y', x') of the same image of (y - y')^2 + (x - x')^2; 0 on a site; VK_EDT_NONE
 * everywhere in an image without a site.  Sites: VK_EDT_FG the foreground, VK_EDT_BG the background, VK_EDT_EDGE the inner boundary:
 * foreground pixels with at least one of their four neighbours inside the image in the background (beyond the border counts as
 * foreground, so a mask that fills the image has no boundary).  1 <= h, w <= VK_EDT_MAX_SIDE, so a true value is at most
 * 2 * 4095^2 < 2^25.  Two passes: columns (workspace int32 [batch][h][w]: the squared distance inside the column, 2^30 where the
 * column holds no site), then rows from LDS with one wave per row: an outward search per pixel that stops at dx^2 >= best where
 * the column distances of the row promise short walks, else the lower envelope of parabolas; sites | VK_EDT_ROWS_SEARCH or
 * sites | VK_EDT_ROWS_ENVELOPE forces one form for every row.  Both are exact and give the same map.
 * workspace: vk_edt_workspace_bytes (0 for sizes the call refuses), 4-byte aligned, as are d2 and an fp32 src.
 *
 * vk_boundary_phi: phi fp32 [batch][h][w] from the two maps of one mask: (float)sqrt((double)d2_fg) on a background pixel
 * (d2_fg > 0), (float)(1.0 - sqrt((double)d2_bg)) on a foreground pixel, 0 where the needed map says VK_EDT_NONE (an empty or a full
 * image is 0 everywhere).  The fp64 square root is correctly rounded: phi equals numpy's float64 sqrt cast to float32.
 *
 * vk_boundary_stats: one vk_boundary_rec per image from pred and gt (each with its own kind and threshold, as vk_edt_sq).  With
 * E(.) the inner boundary and d2(p, S) the squared distance of pixel p to the set S: n_* = |E(.)|, area_* the foreground counts,
 * max2_pg = max over E(pred) of d2(p, E(gt)), q95_2_pg its k-th smallest value, k = (95 n_pred + 99) / 100 (nearest rank: not numpy's
 * interpolated percentile), sum_pg = sum of sqrt(d2) in fp64, within_pg[k] = |{p in E(pred): d2 <= tol2[k]}| for k < n_tol (0 beyond);
 * *_gp the same from E(gt) to E(pred).  max2, q95_2 are -1 and the sums 0 when either boundary is empty.  band_inter / band_union:
 * of the sets {q in A : d2(q, background of A) <= band2}, A = pred and gt (Boundary IoU, Cheng et al., CVPR 2021).  flags: bit 0
 * pred holds no foreground, bit 1 gt holds none.  tol2 is a host array of n_tol <= 8 non-negative integers: a radius tau is
 * floor(tau^2), since d <= tau iff d^2 <= floor(tau^2) for an integer d^2.  Integer atomics only; the fp64 sums are per-workgroup
 * partials added in a fixed order, so two calls give the same bits.  out: device, 8-byte aligned, every byte written.  workspace:
 * vk_boundary_stats_workspace_bytes, 8-byte aligned.
 *
 * vk_boundary_loss: loss_out[0] = (1 / count) sum of sigmoid(logits) phi over logits, phi fp32 [n][c][hw], count = n c hw,
 * 1 <= c <= 16, with the sigmoid expression of vk_seg_loss; products and sums in fp64 (per-workgroup partials, fixed order), one
 * rounding to fp32.  dlogits (may be NULL) = (float)(((phi p (1 - p)) grad_scale) / count), the bracket in fp64.  workspace:
 * VK_BOUNDARY_LOSS_WS_BYTES, 8-byte aligned.  There is no softmax mode.
 *
 * Every call checks its arguments on the host (VK_ERR_ARG before anything touches the stream): batch 1..65535, the map size, the
 * kinds, sites, no null buffer, alignment, workspace size, n_tol, negative tol2 / band2, c, a NaN threshold.
 * ---------------------------------------------------------------------------------------------- */
#define VK_EDT_MAX_SIDE 4096
#define VK_EDT_NONE 0x7fffffff
#define VK_EDT_FG 0
#define VK_EDT_BG 1
#define VK_EDT_EDGE 2
#define VK_EDT_ROWS_ENVELOPE 0x100
#define VK_EDT_ROWS_SEARCH 0x200
#define VK_EDT_ROWS_MASK 0x300
#define VK_EDT_SRC_U8 0
#define VK_EDT_SRC_F32 1
#define VK_BOUNDARY_LOSS_WS_BYTES 32768
typedef struct vk_boundary_rec {
  int64_t n_pred, n_gt;               /* inner-boundary pixels */
  int64_t area_pred, area_gt;
  int32_t max2_pg, max2_gp;           /* max d^2 from the pred boundary to the gt boundary, and back; -1 if undefined */
  int32_t q95_2_pg, q95_2_gp;         /* k-th smallest d^2, k = (95 n + 99) / 100; -1 if undefined */
  double sum_pg, sum_gp;              /* sum of sqrt(d^2) */
  int64_t within_pg[8], within_gp[8]; /* boundary pixels with d^2 <= tol2[k] */
  int64_t band_inter, band_union;
  int32_t flags, reserved;
} vk_boundary_rec;
size_t vk_edt_workspace_bytes(int batch, int h, int w);
int vk_edt_sq(int batch, int h, int w, const void* src, int src_kind, float thresh, int sites, int32_t* d2, void* workspace,
              size_t workspace_bytes, void* stream);
int vk_boundary_phi(int batch, int h, int w, const int32_t* d2_fg, const int32_t* d2_bg, float* phi, void* stream);
size_t vk_boundary_stats_workspace_bytes(int batch, int h, int w);
int vk_boundary_stats(int batch, int h, int w, const void* pred, int pred_kind, float pred_thresh, const void* gt, int gt_kind,
                      float gt_thresh, int n_tol, const int32_t* tol2, int32_t band2, vk_boundary_rec* out, void* workspace,
                      size_t workspace_bytes, void* stream);
int vk_boundary_loss(int n, int c, int hw, const float* logits, const float* phi, float grad_scale, float* dlogits, float* loss_out,
                     void* workspace, size_t workspace_bytes, void* stream);

/* NCHW fp32 [N][3][H][W] -> NHWC4 `dtype` */
int vk_input_transform(vk_dtype dtype, int N, int H, int W, const float* x, void* x4, void* stream);
/* NCHW fp32 [N][cin][H][W] -> NHWC4 of the activation type, channels >= cin written as zero; 1 <= cin <= 4 (anything else: VK_ERR_ARG
 * before any launch).  One 8- or 16-byte store per pixel.  vk_input_transform is cin = 3. */
int vk_input_transform_c(vk_dtype dtype, int N, int cin, int H, int W, const float* x, void* x4, void* stream);
/* The bridge from the device data path (which emits normalised 3-channel fp32 NCHW everywhere) to a model of cout input channels:
 *   out[n][o][p] = fmaf(M[o][2], x2, fmaf(M[o][1], x1, fmaf(M[o][0], x0, b[o]))),   x_j = x3[n][j][p],  p < hw
 * x3 [N][3][hw] and out [N][cout][hw] are fp32 on the device; M [cout][3] and b [cout] (NULL: zero) are HOST arrays read during the call.
 * 1 <= cout <= 4, N <= 65535.  Each input plane is read once and each output plane written once, with 16-byte accesses where hw % 4 == 0
 * and both tensors are 16-byte aligned (every plane then is), element accesses otherwise.  (vk.inputs.ChannelAdapter: the reference
 * reads its monochrome micrographs with IMREAD_COLOR, i.e. replicated.) */
int vk_input_mix(int N, int cout, size_t hw, const float* x3, const float* M, const float* b, float* out, void* stream);

/* BatchNorm statistics -> per-channel affine.  train=1: from batch sums stats[VK_STATS_REPLICAS][2][C] (count = N*H*W), updates
 * running stats (momentum 0.1, unbiased var) and writes mean/invstd for backward.  train=0: from
 * running stats.  scale = gamma*invstd, shift = beta - mean*scale.  Any C > 0.  In train mode running_mean and running_var are
 * given together or both NULL (nothing to update); count = 1 leaves the variance unscaled. */
int vk_bn_finalize(int C, int train, const double* stats, double count, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, float eps, float momentum, float* scale, float* shift,
                   float* save_mean, float* save_invstd, void* stream);

/* pooled = maxpool3x3s2p1(relu(z*scale+shift)); argmax (uint8 0..8, window scan order) kept for backward */
int vk_bn_relu_maxpool(vk_dtype dtype, int N, int H, int W, int C, const void* z, const float* scale,
                       const float* shift, void* pooled, uint8_t* argmax, void* stream);
/* dy[N][H][W][C] += scatter(dpool) through argmax */
int vk_maxpool_bwd(vk_dtype dtype, int N, int H, int W, int C, const void* dpool, const uint8_t* argmax, void* dy,
                   void* stream);
/* vk_maxpool_bwd and the BatchNorm+ReLU-backward reduce of the tensor under the pool in one pass (stem tail): dy holds the other
 * gradient contributions on entry and g = (dy + maxpool backward) * [relu(z*scale+shift) > 0] on return; sum(g), sum(g*z) are added
 * into sums [VK_STATS_REPLICAS][2][C].  Phase 2 is vk_bn_bwd_apply with mask_mode 0.  C / 4 (fp32) or C / 8 (16-bit) must divide
 * 256, else VK_ERR_ARG with dy and sums untouched (vk_bn_relu_maxpool and vk_maxpool_bwd take any C % 8 == 0). */
int vk_maxpool_bwd_bn_reduce(vk_dtype dtype, int N, int H, int W, int C, const void* dpool, const uint8_t* argmax, const void* z,
                             const float* scale, const float* shift, void* dy, double* sums, void* stream);

/* out = relu(z*scale+shift + (res*rscale+rshift | res)) — BasicBlock tail.
 * C: a multiple of 8 up to 512, or 1024 / 2048.  Any other multiple of 8 returns VK_ERR_UNSUPPORTED, a count that is not a positive
 * multiple of 8 VK_ERR_ARG; both before anything touches the stream (out untouched). */
int vk_bn_add_relu(vk_dtype dtype, size_t pixels, int C, const void* z, const float* scale, const float* shift,
                   const void* res, const float* rscale, const float* rshift, void* out, void* stream);

/* BatchNorm(+ReLU) backward, two phases.  mask_mode 0: none, 1: relu(z*scale+shift) > 0, 2: mask_src > 0.
 * phase 1: sums double[VK_STATS_REPLICAS][2][C] += { sum g, sum g*z } (spread over the replicas),  g = dy * mask.
 * phase 2 (after vk_bn_bwd_coeffs): dz = a*g + b*z + c ; optional g_out (+)= g  (identity shortcut); dz may be dy (in place).
 * C of vk_bn_bwd_reduce, vk_bn_bwd_apply and vk_bn_bwd_apply_fused: a multiple of 8 up to 512, or 1024 / 2048.  Any other multiple
 * of 8 returns VK_ERR_UNSUPPORTED, a count that is not a positive multiple of 8 VK_ERR_ARG; both before anything touches the stream
 * (sums / dz / g_out / dgamma / dbeta untouched).  vk_bn_bwd_coeffs[_frozen]: any C > 0. */
int vk_bn_bwd_reduce(vk_dtype dtype, size_t pixels, int C, const void* dy, const void* z, int mask_mode,
                     const float* scale, const float* shift, const void* mask_src, double* sums, void* stream);
int vk_bn_bwd_coeffs(int C, const double* sums, double count, const float* gamma, const float* save_mean,
                     const float* save_invstd, float* dgamma, float* dbeta, float* coef_abc, void* stream);
int vk_bn_bwd_apply(vk_dtype dtype, size_t pixels, int C, const void* dy, const void* z, int mask_mode,
                    const float* scale, const float* shift, const void* mask_src, const float* coef_abc, void* dz,
                    void* g_out, int g_accumulate, void* stream);
/* phase 1.5 of a BatchNorm with FROZEN statistics (eval-mode layer in a training forward): running_mean / running_invstd are what the
 * forward normalised with (1/sqrt(running_var + eps)).  dgamma += r * sum g*(z - mean), dbeta += sum g;  coef_abc = (gamma*r, 0, 0). */
int vk_bn_bwd_coeffs_frozen(int C, const double* sums, const float* gamma, const float* running_mean, const float* running_invstd,
                            float* dgamma, float* dbeta, float* coef_abc, void* stream);
/* phase 2 with vk_bn_bwd_coeffs folded in: coefficients are derived from `sums` inside the kernel and
 * dgamma/dbeta are accumulated by it, once (one launch less per BatchNorm layer).  C as vk_bn_bwd_apply. */
int vk_bn_bwd_apply_fused(vk_dtype dtype, size_t pixels, int C, const void* dy, const void* z, int mask_mode,
                          const float* scale, const float* shift, const void* mask_src, const double* sums, double count,
                          const float* gamma, const float* save_mean, const float* save_invstd, float* dgamma, float* dbeta,
                          void* dz, void* g_out, int g_accumulate, void* stream);

/* d_low[N][H/2][W/2][C] (+)= 2x2 sums of d_up[N][H][W][C] (nearest-x2 upsample backward) */
int vk_upsample2x_bwd(vk_dtype dtype, int N, int H, int W, int C, const void* d_up, void* d_low, int accumulate,
                      void* stream);

/* Segmentation head: 3x3 pad-1 conv C=16 -> 1 with bias on the activated decoder output; fp32 logits. */
int vk_head_fwd(vk_dtype dtype, int N, int H, int W, const vk_src* src, const float* w9x16, const float* bias,
                float* logits, void* stream);
/* Inference only, 16-bit element types (r03): decoder block 4 conv1 -> BN+ReLU -> conv2 -> BN+ReLU -> head over one overlapping tile —
 * smp's DecoderBlock + SegmentationHead behind `model(x)` in eval mode (infer_pth_gui.py:45-53) without the two 512^2 x 16 tensors
 * between them going through HBM.  src: the 32-channel output of decoder block 3 (raw z + its BatchNorm affine, up = 1); w1_pack: conv1
 * weights as vk_halo_pack(16 rows, 32 channels); w2_plain: conv2 weights [16][3][3][16] of the element type; scale / shift: the folded
 * eval BatchNorm affines; head as in vk_head_fwd.  H, W multiples of 16.  Same bits as the three separate calls. */
int vk_dec4_tail_eval(vk_dtype dtype, int N, int H, int W, const vk_src* src, const void* w1_pack, const float* scale1, const float* shift1,
                      const void* w2_plain, const float* scale2, const float* shift2, const float* head_w9x16, const float* head_bias,
                      float* logits, void* stream);
/* dy [N][H][W][16] (element type) is WRITTEN, dw9x16 / dbias are ADDED to (+=).
 * workspace (optional, VK_HEAD_WORKSPACE_BYTES is always enough): per-workgroup partial weight gradients (rows of 148 floats) that a
 * second launch adds in workgroup order -> dw / dbias are bit-reproducible; NULL (or less than one row): fp32 atomics.  A smaller
 * workspace is used as it is: the grid shrinks to the rows it holds and every workgroup walks more tiles. */
#define VK_HEAD_WORKSPACE_BYTES (1024u * 148u * 4u)
int vk_head_bwd(vk_dtype dtype, int N, int H, int W, const vk_src* src, const float* w9x16, const float* dlogits,
                void* dy, float* dw9x16, float* dbias, void* workspace, size_t workspace_bytes, void* stream);
/* same, with the BatchNorm+ReLU backward reduce of the head's input layer fused into the dy kernel (see vk_bnr; mask and accumulate
 * are not used here).  The ReLU mask is [bnr->z * bnr->scale + bnr->shift > 0] on every route, whatever src->relu says (src->relu
 * only decides what the weight gradient sees); bnr may name a tensor other than the head's source.  The 16-bit types run one
 * matrix-core kernel when bnr names the head's own source and coefficients (the same pointers), which rounds dlogits and the filter
 * to the element type; every other combination, and VK_HEAD_NO_MFMA in the environment, runs the two fp32 kernels. */
int vk_head_bwd_fused(vk_dtype dtype, int N, int H, int W, const vk_src* src, const float* w9x16, const float* dlogits,
                      void* dy, float* dw9x16, float* dbias, const vk_bnr* bnr, void* workspace, size_t workspace_bytes, void* stream);

/* loss = mean BCE-with-logits + binary Dice (smp defaults: batch-global, smooth 0, eps 1e-7).
 * sums: double[8] scratch (zeroed by the call); afterwards sums[0..3] = {sum of the BCE terms, sum p*y, sum p, sum y} over all
 * elements (p = 1 / (1 + expf(-x)); fp32 per thread, fp64 from there on) and sums[4..6] hold the gradient coefficients.
 * loss_out[0] = w_bce*bce + w_dice*dice, [1] = bce, [2] = dice; dice = (1 - 2 sum p*y / max(sum p + sum y, 1e-7)) [sum y > 0].
 * dlogits (optional; NULL: nothing is written) = grad_scale * d(loss_out[0])/dlogits.  16-byte loads when both logits and target are
 * 16-byte aligned, element loads otherwise: any count and alignment is accepted. */
int vk_bce_dice_loss(size_t count, const float* logits, const float* target, double* sums, float* loss_out,
                     float* dlogits, float grad_scale, float w_bce, float w_dice, void* stream);

/* ---- more than one class (1 <= C <= 16): the 16 -> C head and its two losses (multiclass.hip).  The binary model keeps the kernels
 * above; these run for a plan created with vk_unet_create_ex(classes > 1) and for the loss modules of any C.
 * Head filter: KRSC [C][3][3][16] fp32, bias [C]; logits / dlogits fp32 NCHW [N][C][H][W] (class planes); src as in vk_head_fwd. */
int vk_head_fwd_multi(vk_dtype dtype, int N, int H, int W, int C, const vk_src* src, const float* w, const float* bias, float* logits,
                      void* stream);
/* dy[N][H][W][16] (element type) = data gradient of the head input, dw [C][3][3][16] += weight gradient, dbias [C] += bias gradient.
 * bnr (optional): the BatchNorm+ReLU backward reduce of the head's input layer fused into the dy pass, as in vk_head_bwd_fused.
 * workspace (required, vk_head_multi_workspace_bytes(C) is always enough): per-workgroup partials of dw / dbias that a second launch
 * adds in workgroup order, so dw / dbias are bit-reproducible. */
size_t vk_head_multi_workspace_bytes(int C);
int vk_head_bwd_multi(vk_dtype dtype, int N, int H, int W, int C, const vk_src* src, const float* w, const float* dlogits, void* dy,
                      float* dw, float* dbias, const vk_bnr* bnr, void* workspace, size_t workspace_bytes, void* stream);
/* Device scratch of the two losses below for logits [N][C][HW] (8-byte aligned).  It need not be cleared or kept between calls: every
 * row of partials that a call reads it has written first; a workspace of exactly this size is accepted and nothing past it is touched. */
size_t vk_multi_loss_workspace_bytes(int N, int C, int HW);
/* loss = w_bce * BCEWithLogitsLoss()(x, y) + w_dice * smp DiceLoss("multilabel")(x, y); x, y fp32 [N][C][HW].
 * Per class c: I = sum sigmoid(x) y, P = sum sigmoid(x), T = sum y over (N, HW) in fp64 (per-workgroup partials added in a fixed
 * order); dice_c = (1 - 2 I / max(P + T, 1e-7)) [T > 0]; dice = mean over c; bce = mean over N C HW.
 * loss_out float[4] = {total, bce, dice, 0}; dlogits (optional) = grad_scale * d total / dx. */
int vk_multilabel_loss(int N, int C, int HW, const float* logits, const float* target, void* workspace, size_t workspace_bytes,
                       float* loss_out, float* dlogits, float grad_scale, float w_bce, float w_dice, void* stream);
/* loss = w_ce * CrossEntropyLoss()(x, t) + w_dice * smp DiceLoss("multiclass")(x, t); x fp32 [N][C][HW], t int64 [N][HW] in [0, C).
 * Dice as above on softmax(x) against one_hot(t); ce = mean over N HW.  A label outside [0, C) is an argument error reported on the
 * device: loss_out = {NaN, NaN, NaN, number of bad labels} (loss_out[3] = 0 when every label is valid); such pixels add nothing and
 * get a zero gradient. */
int vk_multiclass_loss(int N, int C, int HW, const float* logits, const int64_t* target, void* workspace, size_t workspace_bytes,
                       float* loss_out, float* dlogits, float grad_scale, float w_ce, float w_dice, void* stream);

/* ---- configurable loss (seg_loss.hip): a weighted sum of at most one term of each kind, in one reduction pass, one single-workgroup
 * finalize and one backward pass whatever the number of terms.  x fp32 [N][C][HW], 1 <= C <= 16; mode VK_LOSS_BINARY (C == 1) and
 * VK_LOSS_MULTILABEL: target fp32 [N][C][HW], p = sigmoid of x; VK_LOSS_MULTICLASS (C >= 2): target int64 [N][HW], p = softmax over c.
 * m = validity mask (target != ignore_index when has_ignore; multiclass: per pixel), y = target (multiclass: one-hot), both masked.
 *   pix      BCE-with-logits on the soft target (1 - y) sf + y (1 - sf) with pos_weight as torch (sigmoid modes), or cross-entropy
 *            (1 - sf) nll + (sf / C) sum_c -log p_c (multiclass); ignored entries add 0; divided by ALL entries (pix_denom_valid = 0:
 *            smp SoftBCEWithLogitsLoss / SoftCrossEntropyLoss) or by the VALID ones (1: torch.nn)
 *   focal    b = BCE-with-logits of x against y; (1 - e^-b)^gamma b (alpha y + (1 - alpha)(1 - y) when focal_has_alpha), mean over the
 *            valid entries; multiclass: the sum over c of that loss on plane c against [t == c].  gamma is 0 or >= 1.
 *   dice     s = (2 I + smooth) / max(P + T + smooth, eps)                  I = sum p y, P = sum p, T = sum y over (N, HW) per class
 *   jaccard  s = (I + smooth) / max(P + T - I + smooth, eps)
 *   tversky  s = (I + smooth) / max(I + alpha (P - I) + beta (T - I) + smooth, eps); the class mean is raised to tversky_gamma >= 1
 *            each: l_c = -log max(s, eps) when *_log else 1 - s; l_c = 0 where T_c = 0; mean over the classes of *_classes (bit c =
 *            class c; 0 = all C)
 *   mcc      (mode VK_LOSS_BINARY only) tp = I + eps, fp = P - I + eps, fn = T - I + eps, tn = M - P - T + I + eps, M = valid entries;
 *            1 - (tp tn - fp fn) / sqrt((tp + fp)(tp + fn)(tn + fp)(tn + fn)), eps = mcc_eps > 0
 * A term whose denominator is zero because every entry is ignored is 0.  terms: bit 0 pix, 1 focal, 2 dice, 3 jaccard, 4 tversky,
 * 5 mcc.
 * struct_size must be the size of the structure (versioning). */
typedef struct vk_seg_loss_cfg {
  uint32_t struct_size;
  int32_t mode;
  uint32_t terms;
  int32_t has_ignore, ignore_index;
  float w_pix, w_focal, w_dice, w_jaccard, w_tversky;
  float pix_smooth;
  int32_t pix_denom_valid, has_pos_weight;
  float pos_weight[16];
  int32_t focal_has_alpha;
  float focal_alpha, focal_gamma;
  float dice_smooth, dice_eps;
  int32_t dice_log;
  uint32_t dice_classes;
  float jaccard_smooth, jaccard_eps;
  int32_t jaccard_log;
  uint32_t jaccard_classes;
  float tversky_smooth, tversky_eps;
  int32_t tversky_log;
  uint32_t tversky_classes;
  float tversky_alpha, tversky_beta, tversky_gamma;
  float w_mcc, mcc_eps;    /* appended: no earlier field moved */
} vk_seg_loss_cfg;
size_t vk_seg_loss_cfg_size(void);
/* Device scratch for logits [N][C][HW] in any mode (8-byte aligned).  It need not be cleared or kept between calls; a workspace of
 * exactly this size is accepted and nothing past it is touched. */
size_t vk_seg_loss_workspace_bytes(int N, int C, int HW);
/* loss_out float[8] = {total, pix, focal, dice, jaccard, tversky, bad labels, mcc} (absent terms 0); dlogits (optional) = grad_scale *
 * d total / dx, exactly 0 at ignored entries.  A multiclass label that is neither in [0, C) nor ignore_index is an argument error
 * reported on the device as in vk_multiclass_loss: values NaN, loss_out[6] = their number, zero gradient there, nothing faults.
 * The configuration is checked on the host first (VK_ERR_ARG and vk_last_error_string).  Per-workgroup fp64 partial rows added in a
 * fixed order: the same inputs give the same bits.  16-byte accesses when HW % 4 == 0 and the buffers are 16-byte aligned. */
int vk_seg_loss(const vk_seg_loss_cfg* cfg, int N, int C, int HW, const float* logits, const void* target, void* workspace,
                size_t workspace_bytes, float* loss_out, float* dlogits, float grad_scale, void* stream);

/* ---- Lovasz losses (lovasz.hip): a stable device radix sort of the errors (descending, equal errors by ascending flat index; errors
 * compare as fp32 bit patterns in radix order), an integer prefix count of the labels over that order, the Jaccard increments dJ in
 * closed form and a scatter of the gradient back.  logits fp32 [N][C][HW], 1 <= C <= 16, targets as vk_seg_loss takes them.
 *   VK_LOSS_BINARY / VK_LOSS_MULTILABEL (hinge): e = 1 - x (2 y - 1); entries with y == ignore_index are left out; a segment is the
 *     whole batch or (per_image) one image's C HW entries; segment loss = sum_k relu(e_(k)) dJ_k; the result is the mean over the
 *     segments (a segment without a valid entry is 0).
 *   VK_LOSS_MULTICLASS (softmax): p = softmax over c; per class c present among the valid labels of the segment: e = |[t == c] - p_c|,
 *     class loss = sum_k e_(k) dJ_k; segment loss = mean over the present classes; mean over the segments.  A label that is neither a
 *     class nor ignore_index is counted (loss_out[1]), never used as an index, and makes the value NaN.
 * struct_size must be the size of the structure. */
typedef struct vk_lovasz_cfg {
  uint32_t struct_size;
  int32_t mode, per_image, has_ignore, ignore_index;
} vk_lovasz_cfg;
size_t vk_lovasz_cfg_size(void);
/* Device scratch of vk_lovasz_loss (8-byte aligned; the caller owns it, it is no part of a plan's workspace); 0 for a configuration or
 * shape the call would refuse (more than 2^31 - 1 entries among them). */
size_t vk_lovasz_workspace_bytes(const vk_lovasz_cfg* cfg, int N, int C, int HW);
/* loss_out float[4] = {value, bad labels, 0, 0}; dlogits (optional) = grad_scale * d value / dx, written (accumulate = 0: exactly 0 at
 * ignored entries and where the error is not positive) or added (accumulate = 1: ignored entries are left unchanged).  The same inputs
 * give the same bits.  NaN or infinite logits give meaningless values, never an access outside the buffers. */
int vk_lovasz_loss(const vk_lovasz_cfg* cfg, int N, int C, int HW, const float* logits, const void* target, void* workspace,
                   size_t workspace_bytes, float* loss_out, float* dlogits, float grad_scale, int accumulate, void* stream);
/* The sort / scan / apply core on caller-supplied errors fp32 [S][L] with flag uint8 [S][L] (0 background, 1 foreground, 2 ignored):
 * loss_out float[S] = sum_k relu(e_(k)) dJ_k per segment; derr_out (optional) fp32 [S][L] = dJ at the entry's rank where e > 0, else 0;
 * rank_out (optional) uint32 [S][L] = the entry's position in the sorted order of its segment, 0xFFFFFFFF for ignored entries. */
size_t vk_lovasz_flat_workspace_bytes(int S, int64_t L);
int vk_lovasz_flat(const float* errors, const uint8_t* flag, int S, int64_t L, void* workspace, size_t workspace_bytes, float* loss_out,
                   float* derr_out, uint32_t* rank_out, void* stream);

/* Thresholded Dice / IoU of the reference's validate() (train.py:230-255 `dice_coef`, :259-281 `iou_coef`, :518-522):
 * per image i of `per_image` elements, pred = (p > threshold) as 0/1, I = sum pred*t, P = sum pred, T = sum t;
 * dice_i = (2 I + eps) / (P + T + eps), iou_i = (I + eps) / (P + T - I + eps) in fp32.
 * pred: probabilities, or logits when from_logits != 0 (then p = 1 / (1 + expf(-x)) first).
 * The comparison is the strict >: a probability exactly on the threshold, and a zero logit at 0.5, is a miss (post-processing above
 * uses >=).  pred and target need 4-byte alignment only: 16-byte loads are used when both have it and per_image % 4 == 0.
 * out (device, 2 + 2 n_images floats): [0] mean dice, [1] mean iou, [2 + 2i], [3 + 2i] = image i.
 * workspace: vk_seg_metrics_workspace_bytes(n_images) of 8-byte aligned device scratch; afterwards it holds the
 * fp64 sums {I, P, T} per image.  One pass over both tensors + one single-workgroup launch; bit-reproducible for 0/1 targets. */
size_t vk_seg_metrics_workspace_bytes(int n_images);
int vk_seg_metrics(int n_images, size_t per_image, const float* pred, const float* target, int from_logits, float threshold,
                   float eps, void* workspace, size_t workspace_bytes, float* out, void* stream);
/* The same per class for C = 1..16 class planes (multiclass_eval.hip).  mode VK_LOSS_MULTILABEL: logits fp32 [N][C][per_image],
 * target fp32 [N][C][per_image] of 0/1, pred_c = (sigmoid(x_c) > threshold), or x_c > threshold when from_logits == 0; another target
 * value skips that (pixel, class).  mode VK_LOSS_MULTICLASS (C >= 2): target int64 [N][per_image], pred = argmax_c x_c (ties to the
 * lowest index; from_logits is irrelevant); a label outside [0, C) skips the pixel.  Skipped entries are counted in *bad_labels (device
 * int, zeroed by the call); nothing faults.  Per (image, class): tp, fp, fn and tn = valid pixels - tp - fp - fn as int64 (exact,
 * bit-reproducible); dice / iou as in vk_seg_metrics, so a class absent from both prediction and target scores 1; a class's batch
 * score is the fp64 mean over images rounded once, the overall score the fp64 mean over classes.
 * out (device floats, 2 + 2 C + 2 N C) = [mean dice, mean iou, dice_c[C], iou_c[C], per_image[N][C][2] {dice, iou}];
 * stats (optional, device int64 [4][N][C]) = {tp, fp, fn, tn}.  With C == 1 and 0/1 targets, multilabel gives vk_seg_metrics's bits.
 * workspace: vk_seg_metrics_multi_workspace_bytes(n_images, C) of 8-byte aligned device scratch. */
size_t vk_seg_metrics_multi_workspace_bytes(int n_images, int C);
int vk_seg_metrics_multi(int mode, int n_images, int C, size_t per_image, const float* logits, const void* target, int from_logits,
                         float threshold, float eps, void* workspace, size_t workspace_bytes, int64_t* stats, float* out,
                         int* bad_labels, void* stream);

/* Threshold sweep (sweep.hip): the counts of vk_seg_metrics / vk_seg_metrics_multi (multilabel) for EVERY threshold of a grid from one
 * pass over prediction and target, and the curves that follow from them.
 *
 * vk_sweep_hist.  A plane is one (image, class) map of per_plane elements (1 <= per_plane < 2^31); plane p starts plane_stride elements
 * after plane p - 1 in both tensors (0 = per_plane; a larger stride feeds a part of every plane).  pred fp32: probabilities or scores,
 * or logits when from_logits != 0 (then pv = 1 / (1 + expf(-x)), vk_seg_metrics' expression).  target fp32, or uint8 when target_u8 != 0:
 * 1 is positive, 0 negative, a value equal to ignore_index (when has_ignore != 0) is skipped, any other value is skipped and counted
 * in *bad (device int).  thr_host: K thresholds on the HOST, 1 <= K <= 1024, finite and strictly ascending (checked before anything
 * is launched); thr_dev: the same K floats in device memory, which the kernel reads (garbage there gives garbage counts, never an
 * access outside a buffer).  hist (device int32 [n_planes][2][K + 1]): hist[p][t][b] = number of valid elements of plane p with target t
 * and bin b = #{k : pv > thr[k]} (strict; NaN compares false and lands in bin 0, +inf in bin K).  accumulate == 0 zeroes hist and *bad
 * first, accumulate != 0 adds to them.  Integer atomics only: bit-reproducible.  For threshold k: P = sum over b > k of both rows,
 * I = sum over b > k of row 1, T = sum of row 1 are vk_seg_metrics' sums at threshold thr[k].
 * 16-byte loads of the prediction (and of an fp32 target; 4-byte loads of a uint8 one) when the pointers are aligned to them and
 * per_plane and plane_stride are multiples of 4; otherwise a scalar path.
 *
 * vk_sweep_curves.  hist (device int32 [N][C][2][K + 1]) -> every output listed in vk_sweep_layout, written at its byte offset into
 * `out` (device, 8-byte aligned, at least total_bytes = vk_sweep_curves_out_bytes):
 *   stats       int64 [K][4][N][C] {tp, fp, fn, tn} and per_image fp32 [K][N][C][2] {dice, iou}: row k is what vk_seg_metrics_multi
 *               (multilabel) writes at threshold thr[k], same expressions, same order;
 *   dice, iou   fp32 [K][C]: the class's fp64 mean over the images rounded once (worker j sums images j, j + 64, ...; the 64 partials
 *               are added in j order); mean_dice, mean_iou fp32 [K]: the fp64 mean of the rounded class scores, rounded once;
 *   micro_stats int64 [4][K][C]: the counts pooled over the images; micro fp64 [5][K][C] = precision tp / (tp + fp), recall
 *               tp / (tp + fn), f1 2 tp / (2 tp + fp + fn), iou tp / (tp + fp + fn), fpr fp / (fp + tn); a ratio with a zero denominator
 *               is 1, the fpr 0;
 *   ap, auc     fp64 [C]: AP = sum_k (recall_k - recall_{k+1}) precision_k with recall_K = 0; ROC-AUC by the trapezoid rule over
 *               (1, 1), (fpr_k, recall_k) for k ascending, (0, 0).  Both see only the grid's operating points;
 *   best_dice, best_iou, best_f1 int32 [C]: the lowest k of the best dice[k][c], iou[k][c], micro f1; best_mean int32 [2]: the same
 *               for mean_dice and mean_iou.
 * group (optional, device int32 [N], with n_groups = G in [1, N]) names the validation batch of every image; an image whose value is
 * outside [0, G) belongs to no batch.  Then also group_dice, group_iou fp32 [G][K][C], group_mean_dice, group_mean_iou fp32 [G][K]: the
 * same means over the group's images, numbered from 0 in ascending image index (one vk_seg_metrics call over that batch), and
 * epoch_dice, epoch_iou fp64 [K][C], epoch_mean_dice, epoch_mean_iou fp64 [K]: (sum over g ascending of (double) score_g) / G, the
 * reference's validate (train.py:518-529).  workspace: workspace_bytes of the layout, 8-byte aligned device scratch (none without
 * groups).  N in [1, 65535], C in [1, 16], K in [1, 1024].  Neither call synchronises; contraction is off, every operation is IEEE in
 * a fixed order. */
typedef struct vk_sweep_layout {
  size_t stats, per_image, dice, iou, mean_dice, mean_iou, micro_stats, micro, ap, auc, best_dice, best_iou, best_f1, best_mean;
  size_t group_dice, group_iou, group_mean_dice, group_mean_iou, epoch_dice, epoch_iou, epoch_mean_dice, epoch_mean_iou;
  size_t total_bytes, workspace_bytes;
} vk_sweep_layout;
int vk_sweep_hist(int n_planes, size_t per_plane, size_t plane_stride, const float* pred, const void* target, int target_u8,
                  int from_logits, int has_ignore, int ignore_index, int K, const float* thr_host, const float* thr_dev, int accumulate,
                  int32_t* hist, int* bad, void* stream);
int vk_sweep_curves_layout(int n_images, int C, int K, int n_groups, vk_sweep_layout* layout);
size_t vk_sweep_curves_out_bytes(int n_images, int C, int K, int n_groups);     /* 0 when a size is out of range */
int vk_sweep_curves(int n_images, int C, int K, const int32_t* hist, const int32_t* group, int n_groups, float eps, void* workspace,
                    size_t workspace_bytes, void* out, size_t out_bytes, void* stream);

/* Object-level validation (instances.hip): which indentations were found, and how far off are their diagonals.  The object-level
 * companion of the pixel counts above: integer counts and IEEE operations in a fixed order, contraction off, no call synchronises.
 *
 * vk_inst_contingency.  pred_slots, gt_slots: device int32 [batch][h][w], two outputs of vk_geom_slot_map (h * w < 2^30, batch in
 * 1..65535).  table: device int32 [batch][Mp + 1][Mg + 1], zeroed by the call; Mp, Mg in 1..256.  Index 0 means "none", index 1 + s
 * means slot s; a slot value outside [0, M) (-1, -2, any other negative value, any value >= M) counts as none and never addresses
 * the table.  table[b][i][j] = pixels of map b with pred index i and GT index j; every table sums to h * w, [0][0] included (that cell
 * is derived as h * w minus the rest).  Integer atomics only: bit-reproducible.  16-byte loads when both maps are 16-byte aligned
 * and w is a multiple of 4, otherwise a scalar path.
 *
 * vk_inst_match.  table as above.  n_pred, n_gt: device int32 [batch], the `counts` of the two geometry calls; the call uses
 * min(count, M) slots (a negative count as 0) and flags the image when count > M.  iou_thresholds: K doubles on the HOST, 1 <= K <= 16,
 * finite, strictly ascending, in [0.5, 1), checked before anything is launched and passed by value.  diag_pred, diag_gt (optional,
 * used only when both are given): the float64 d_mean of slot s of image b is at (char*)diag + ((size_t)b * M + s) * stride, stride in
 * bytes and a multiple of 8, so records of vk_geom_det or vk_geom_quad are read in place.
 *   Ap(i) = sum of row i, Ag(j) = sum of column j, each with its "none" cell; I = table[i][j]; U = Ap + Ag - I.
 *   Pred slot s < n_pred_used and GT slot t < n_gt_used are a CANDIDATE iff 3 I > Ap + Ag in int64: IoU > 1/2 exactly, hence at most
 *   one candidate per pred slot and per GT slot, no ties and no greedy order.  iou = (double)I / (double)U.  The pair is MATCHED at
 *   threshold k iff it is a candidate and iou > thr[k] (strict: the panoptic-quality convention).
 * Per pred slot, [batch][Mp]: pair_gt int32 (the candidate's GT slot or -1), pair_iou fp64 (0 without a candidate), pair_derr fp64
 * (dp - dg; 0 without a candidate or without diagonals).  Slots at or above n_pred_used get -1, 0, 0.
 * per_image [batch][K] and totals [K] are vk_inst_stats records.  Per image and threshold: tp, fp = n_pred_used - tp,
 * fn = n_gt_used - tp, and over the matched pairs in ascending pred slot, each sum sequential in fp64: sum_iou, sum_abs_d = sum |dp - dg|,
 * max_abs_d, and over those of them with dg > 0 and dp > 0 (their number is n_rel): sum_rel_d = sum |dp - dg| / dg,
 * sum_signed_rel_d = sum (dp - dg) / dg, sum_hv_rel = sum ((dg / dp) * (dg / dp) - 1.0), the relative error of a hardness that goes as
 * 1 / d^2.  Without diagonals these are 0.  The same for every threshold of an image: n_pred_used, n_gt_used, n_split (GT slots
 * that two or more pred slots touch with I > 0), n_merge (pred slots that two or more GT slots touch), overflow_pred / overflow_gt
 * (1 when count > M), n_images = 1.
 * totals[k] starts from zero, or from its contents when accumulate != 0; then image 0 is added, then image 1, and so on (max_abs_d by
 * maximum): an epoch's totals are one flat sequence over its images and their bits do not depend on how it was cut into batches.
 * One call is two launches: one workgroup per image, then the pass over the images. */
typedef struct vk_inst_stats {
  int64_t tp, fp, fn, n_rel;
  int64_t n_pred_used, n_gt_used, n_split, n_merge, overflow_pred, overflow_gt, n_images;
  double sum_iou, sum_abs_d, sum_rel_d, sum_signed_rel_d, sum_hv_rel, max_abs_d;
} vk_inst_stats;
int vk_inst_contingency(int batch, int h, int w, const int32_t* pred_slots, const int32_t* gt_slots, int Mp, int Mg, int32_t* table,
                        void* stream);
int vk_inst_match(int batch, int Mp, int Mg, const int32_t* table, const int32_t* n_pred, const int32_t* n_gt, int K,
                  const double* iou_thresholds, const void* diag_pred, size_t diag_pred_stride, const void* diag_gt,
                  size_t diag_gt_stride, int32_t* pair_gt, double* pair_iou, double* pair_derr, vk_inst_stats* per_image,
                  vk_inst_stats* totals, int accumulate, void* stream);

/* Sub-pixel vertex refinement of the indentation fit (subpix.hip).  vk_geom_det and vk_geom_quad carry int32 corners, so their
 * diagonals are quantised to a map pixel at either tip.  This call moves each of the four corners of every record to where the
 * probability map the fit was made from puts it, in float64, and forms the diagonals again.  One launch, one 256-thread workgroup per
 * (image, slot), wave k refines vertex k; no workspace, no atomics, no synchronisation.
 *
 * prob: device float32 [batch][h][w], the map the geometry call read (h, w >= 1, h * w < 2^30, batch 1..65535).  records: the
 * geometry call's `dets`, read in place: slot s of image b is at (char*)records + ((size_t)b * max_components + s) * record_stride; it
 * begins with int label, int area, holds int box[8] at box_offset and, when valid_offset >= 0, int valid there (the quadrilateral fit;
 * -1 for the rectangle fit: every record is valid).  record_stride and the offsets are multiples of 4.  counts: device int32 [batch],
 * max_components 1..4096.  affine (optional): device double [batch][3] = (ox, oy, inv_scale), the letterbox geometry of each image;
 * NULL means (0, 0, 1).  out: device vk_subpix_quad [batch][max_components], 8-byte aligned.
 *
 * Only the slots 0 .. min(counts[b], max_components) - 1 are written (a negative count as 0), every byte of them; nothing else is
 * touched.  A record with valid == 0 gives label, area, valid = 0 and zeros in every other field.  Otherwise v holds the refined
 * vertices in map coordinates in the record's order, vs[2 i] = (v[2 i] - ox) * inv_scale, vs[2 i + 1] = (v[2 i + 1] - oy) * inv_scale,
 * and the diagonals follow the rule of the geometry records on v in float64: d = sqrt(dx * dx + dy * dy) of the six pairs in the order
 * (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), the first longest one is the first diagonal, the other two vertices give the second;
 * d1 = dmax * inv_scale, d2 = sqrt(ex * ex + ey * ey) * inv_scale, d_mean = 0.5 * (d1 + d2).
 *
 * Arithmetic: IEEE float64, contraction off, only + - * / sqrt floor fabs and compares on the device; every expression below is
 * evaluated as written, left to right inside its parentheses.
 *   sample(x, y):  x = x > 0 ? x : 0;  x = x < w - 1 ? x : w - 1 (so a NaN becomes 0); y likewise with h;
 *     x0 = min((int)floor(x), w - 2), or 0 when w == 1; x1 = x0 + 1, or 0 when w == 1; y0, y1 likewise; fx = x - x0, fy = y - y0;
 *     top = p[y0][x0] * (1 - fx) + p[y0][x1] * fx;  bot = p[y1][x0] * (1 - fx) + p[y1][x1] * fx;  value = top * (1 - fy) + bot * fy.
 *
 * method VK_SUBPIX_CORNER, gradient orthogonality (the iteration OpenCV documents for cornerSubPix).  win 2..15, zero_zone -1..win - 1,
 * max_iter 1..100, eps > 0, wt[2 win + 1] finite (the caller's exp(-((k - win) / win)^2): no transcendental runs on the device).
 * q = the int32 vertex.  Per iteration: S[j][i] = sample(q.x + (i - win - 1), q.y + (j - win - 1)), i, j = 0 .. 2 win + 2.  For
 * j, i = 0 .. 2 win: px = i - win, py = j - win, m = wt[j] * wt[i], or 0 when zero_zone >= 0 and |px| <= zero_zone and
 * |py| <= zero_zone; gx = S[j+1][i+2] - S[j+1][i], gy = S[j+2][i+1] - S[j][i+1]; gxx = gx * gx, gxy = gx * gy, gyy = gy * gy;
 * the row sums, i ascending from 0.0: ra += m * gxx, rb += m * gxy, rc += m * gyy, r1 += m * (gxx * px + gxy * py),
 * r2 += m * (gxy * px + gyy * py); then a, b, c, bb1, bb2 from 0.0 over the row sums, j ascending.  det = a * c - b * b.  Unless
 * fabs(det) > DBL_EPSILON * DBL_EPSILON and det is finite: flag SINGULAR, stop.  step = ((c * bb1 - b * bb2) / det,
 * (a * bb2 - b * bb1) / det); q += step; iters += 1.  Then, in this order: step.x * step.x + step.y * step.y <= eps * eps: stop
 * (converged); unless 0 <= q.x < w and 0 <= q.y < h: flag LEFT_MAP, stop; iters == max_iter: flag NOT_CONVERGED, stop.  Afterwards,
 * unless fabs(q.x - start.x) <= win and fabs(q.y - start.y) <= win (a NaN fails): q = start, flag RESTORED.
 *
 * method VK_SUBPIX_LINES, the two sides that meet at the vertex.  0 <= lo < hi <= 1, n_stations 3..32, reach R 1..15, level finite,
 * max_shift > 0.  centre = (((x0 + x1) + x2) + x3) * 0.25 of the start vertices, y likewise.  For vertex i, the sides towards
 * j = (i + 1) & 3 and then j = (i + 3) & 3: d = V_j - V_i, L = sqrt(d.x * d.x + d.y * d.y); L < 8: flag SHORT_SIDE.
 * n = (d.y / L, -d.x / L), negated when n.x * (V_i.x - centre.x) + n.y * (V_i.y - centre.y) < 0.  Station k = 0 .. n_stations - 1:
 * f = lo + ((hi - lo) * k) / (n_stations - 1), s = (V_i.x + d.x * f, V_i.y + d.y * f), g_t = sample(s.x + t * n.x, s.y + t * n.y) for
 * t = -R .. R.  For t = -R .. R - 1 ascending, where g_t >= level and level > g_t+1: pos = t + (g_t - level) / (g_t - g_t+1), taken
 * when fabs(pos) is below the best so far (which starts at +inf, so a NaN never wins and the smaller t wins a tie); the station's
 * point is (s.x + pos * n.x, s.y + pos * n.y).  Fewer than three points on a side: flag NO_EDGE.  Otherwise total least squares over
 * the points in station order: sums of x and y from 0.0, centroid c = sum / count; sxx, syy, sxy from 0.0 over dx * dx, dy * dy,
 * dx * dy with dx = x - c.x, dy = y - c.y; hs = (sxx + syy) * 0.5, hd = (sxx - syy) * 0.5, lam = hs + sqrt(hd * hd + sxy * sxy);
 * direction v = (sxy, lam - sxx) when fabs(lam - sxx) > fabs(lam - syy), else (lam - syy, sxy).  With a flag from either side the
 * vertex keeps its start.  Otherwise den = v1.x * v2.y - v1.y * v2.x; unless den * den > 1e-6 * ((v1.x * v1.x + v1.y * v1.y) *
 * (v2.x * v2.x + v2.y * v2.y)): flag PARALLEL, start kept.  e = c2 - c1, u = (e.x * v2.y - e.y * v2.x) / den,
 * q = (c1.x + u * v1.x, c1.y + u * v1.y); unless fabs(q.x - start.x) <= max_shift and fabs(q.y - start.y) <= max_shift: start kept, flag
 * RESTORED.  iters[i] counts the points found on the two sides. */
#define VK_SUBPIX_CORNER 0
#define VK_SUBPIX_LINES 1
#define VK_SUBPIX_MAX_WIN 15
#define VK_SUBPIX_MAX_REACH 15
#define VK_SUBPIX_MAX_STATIONS 32
#define VK_SUBPIX_SINGULAR 1
#define VK_SUBPIX_LEFT_MAP 2
#define VK_SUBPIX_NOT_CONVERGED 4
#define VK_SUBPIX_RESTORED 8
#define VK_SUBPIX_SHORT_SIDE 16
#define VK_SUBPIX_NO_EDGE 32
#define VK_SUBPIX_PARALLEL 64
typedef struct vk_subpix_params {
  int method;                   /* VK_SUBPIX_CORNER / VK_SUBPIX_LINES; the other method's fields are not read */
  int win, zero_zone, max_iter; /* corner */
  double eps;
  double wt[2 * VK_SUBPIX_MAX_WIN + 1];
  int n_stations, reach;        /* lines */
  double lo, hi, level, max_shift;
} vk_subpix_params;
typedef struct vk_subpix_quad {
  int label, area;              /* copied from the source record */
  int valid;                    /* 1, or 0 for a quadrilateral record with valid == 0 */
  int reserved;                 /* written as 0 */
  int flags[4];                 /* per vertex, VK_SUBPIX_* bits; 0: refined without remark */
  int iters[4];
  double v[8];                  /* x0,y0 .. x3,y3 in map coordinates */
  double vs[8];                 /* the same in source-image coordinates */
  double d1, d2, d_mean;        /* in source-image pixels */
} vk_subpix_quad;
int vk_subpix_refine(const vk_subpix_params* params, int batch, int h, int w, const float* prob, const void* records,
                     size_t record_stride, size_t box_offset, int valid_offset, const int32_t* counts, int max_components,
                     const double* affine, vk_subpix_quad* out, void* stream);

/* Vertex heatmaps (keypoints.hip): the targets of a heatmap plane beside the mask, and its read-out.
 *
 * Conventions of the three calls.  Coordinates are those of the geometry records: pixel (x, y) lies at the point (x, y).  Records are
 * read in place as vk_subpix_refine reads them: slot t of map b is at (char*)records + ((size_t)b * max_components + t) * record_stride,
 * and the slots used are t < min(max(counts[b], 0), max_components) with valid != 0 (valid_offset -1: every slot is valid).  A map of
 * image b begins at base + b * image_stride (in elements, at least h * w) and its rows are w elements apart, so plane 1 of a
 * [N][2][h][w] tensor is written or read in place with image_stride = 2 h w.  batch 1..65535, h, w >= 1 with h * w <= 2^30,
 * max_components 1..4096.  No transcendental runs on the device and there is no float atomic; float64 where stated, contraction off,
 * every expression evaluated as written.  Every call checks its arguments on the host and returns VK_ERR_ARG before anything touches
 * the stream.
 *
 * vk_kp_targets: vertex records -> a heatmap.  vert_type VK_KP_VERT_I32 reads int32[8] at vert_offset (box of vk_geom_det and
 * vk_geom_quad; offset and stride multiples of 4): X = 16 * x in int64.  VK_KP_VERT_F64 reads double[8] (v of vk_subpix_quad, or a
 * bare [batch][max_components][8] array with record_stride 64, vert_offset 0 and valid_offset -1; offset and stride multiples of 8,
 * records 8-byte aligned): a vertex is skipped unless fabs(v) <= 2^20 for both coordinates (a NaN fails), else
 * X = (int64)floor(v * 16.0 + 0.5); Y likewise.  table: device float32 [table_len], table_len = R16 * R16 + 1 with
 * 1 <= R16 <= VK_KP_MAX_RADIUS16; the caller builds it (table[k] = float32(exp(-(k / 256) / (2 sigma^2))) for a Gaussian of sigma
 * pixels).  For output pixel (x, y) and every used vertex in ascending (slot, q): D = (16 x - X)^2 + (16 y - Y)^2, exact (a vertex
 * further than R16 in either axis has D >= table_len whatever its size); if D < table_len: v = table[D], if (v > best) best = v.
 * best starts at 0.0f, so a NaN never wins; out[b][y][x] = best.  Every element of the batch planes is written exactly once and
 * nothing else is.  flags: 0 (the library's choice), VK_KP_TABLE_MEMORY or VK_KP_TABLE_LDS (table_len <= VK_KP_TABLE_LDS_MAX): where
 * the table is read from; the bytes written are the same.  out is 4-byte aligned; a 16-byte aligned out with image_stride and w
 * multiples of 4 takes the 16-byte store path, with the same bytes.
 *
 * vk_kp_peaks: a heatmap -> the list of its local maxima.  Pixel (x, y) of value p is a peak iff (double)p >= min_peak (finite), no
 * pixel of the (2 r + 1)^2 window around it inside the map has p' > p, and no raster-earlier pixel of that window has p' == p;
 * r = nms_radius, 1..VK_KP_MAX_NMS.  A NaN is never a peak and never suppresses one.  out: vk_kp_peak records
 * [batch][max_peaks] (max_peaks 1..4096) in raster order, the first max_peaks of each map; counts[b] = the number of all peaks, also
 * above max_peaks; slots at or above min(counts[b], max_peaks) are not touched.  A count pass, an ordered prefix and an emit pass: no
 * atomics.  workspace: vk_kp_peaks_workspace_bytes (0 for arguments out of range) = VK_KP_PEAKS_WS_BYTES, 4-byte aligned; it need
 * not be cleared.
 *
 * vk_kp_refine: first-pass records and a heatmap -> vk_subpix_quad records.  The arguments of vk_subpix_refine with heat and its
 * image_stride in place of prob.  search 1..VK_KP_MAX_SEARCH, cwin 1..VK_KP_MAX_CWIN, min_peak finite, floor_frac in [0, 1).  Per
 * vertex, s = the int32 corner.  Peak: the largest value of the (2 search + 1)^2 window around s clipped to the map, the raster-first
 * pixel among equal values; a NaN never wins.  No pixel in the window (or only NaNs), or (double)peak < min_peak: flag VK_KP_NO_PEAK,
 * the vertex keeps s.  A peak on the border of the unclipped window: flag VK_KP_AT_EDGE, the estimate is kept.  With the peak at
 * (px, py) of value c:
 *   VK_KP_PARABOLA, per axis in float64 on the float32 values l, c, r of the peak's row (column): den = (l - c) + (r - c); the offset
 *     is 0.5 * (l - r) / den when den < 0 and the peak is not on the map's border in that axis, else 0; q = (px + ox, py + oy).
 *   VK_KP_CENTROID: fl = floor_frac * c; over the (2 cwin + 1)^2 window around the peak clipped to the map, j ascending then i
 *     ascending, from 0.0: g = p - fl if that is above 0, else 0 (a NaN gives 0); sw += g, sx += g * (i - px), sy += g * (j - py);
 *     q = (px + sx / sw, py + sy / sw) when sw > 0, else (px, py).
 * A map that holds an infinity can give a NaN estimate (inf - inf), whose sign bit is the hardware's; NaNs and finite values give the
 * same bytes everywhere.
 * After the four vertices: any two that used the same peak pixel both get VK_KP_SHARED and keep s.  iters[q] is 1 where a peak was
 * used, else 0.  label, area, valid, v, vs, d1, d2, d_mean and the record of valid == 0 are those of vk_subpix_refine. */
#define VK_KP_VERT_I32 0
#define VK_KP_VERT_F64 1
#define VK_KP_MAX_RADIUS16 192
#define VK_KP_MAX_NMS 8
#define VK_KP_MAX_SEARCH 31
#define VK_KP_MAX_CWIN 7
#define VK_KP_TABLE_MEMORY 1
#define VK_KP_TABLE_LDS 2
#define VK_KP_TABLE_LDS_MAX 15360
#define VK_KP_PARABOLA 0
#define VK_KP_CENTROID 1
#define VK_KP_NO_PEAK 128     /* beside the VK_SUBPIX_* bits, in the same flags field */
#define VK_KP_AT_EDGE 256
#define VK_KP_SHARED 512
#define VK_KP_PEAKS_WS_BYTES(batch, h, w) ((size_t)(batch) * (((size_t)(h) * (size_t)(w) + 1023) / 1024) * 260)
typedef struct vk_kp_peak {
  int32_t x, y;
  float value;
  int32_t reserved;             /* written as 0 */
} vk_kp_peak;
typedef struct vk_kp_params {
  int method;                   /* VK_KP_PARABOLA / VK_KP_CENTROID */
  int search, cwin;
  double min_peak, floor_frac;
} vk_kp_params;
int vk_kp_targets(int batch, int h, int w, const void* records, size_t record_stride, size_t vert_offset, int vert_type,
                  int valid_offset, const int32_t* counts, int max_components, const float* table, int table_len, float* out,
                  size_t image_stride, int flags, void* stream);
size_t vk_kp_peaks_workspace_bytes(int batch, int h, int w);
int vk_kp_peaks(int batch, int h, int w, const float* heat, size_t image_stride, double min_peak, int nms_radius, int max_peaks,
                vk_kp_peak* out, int32_t* counts, void* workspace, size_t workspace_bytes, void* stream);
int vk_kp_refine(const vk_kp_params* params, int batch, int h, int w, const float* heat, size_t image_stride, const void* records,
                 size_t record_stride, size_t box_offset, int valid_offset, const int32_t* counts, int max_components,
                 const double* affine, vk_subpix_quad* out, void* stream);

/* ---- per-plane pixel losses of a keypoint head (kp_loss.hip).  logits fp32 [N][C][HW], target fp32 [N][C][HW]
 * with values in [0, 1] (the y2 of vk.keypoints.make_targets), 1 <= C <= 16.  Every plane follows one of three rules, given as two
 * disjoint bit masks that are not both empty and name no plane >= C; with e = expf(-|x|), l1p = log1pf(e), p = sigmoid(x) and
 * omp = 1 - p as vk_seg_loss forms them, log p = -(max(-x, 0) + l1p), log(1 - p) = -(max(x, 0) + l1p):
 *   heat plane c  (penalty-reduced focal loss; alpha, beta integers in 0..VK_KP_LOSS_MAX_EXP): an entry is positive iff
 *            y >= pos_threshold;  positive: -omp^alpha log p;  negative: -(1 - y)^beta p^alpha log(1 - p);
 *            S_c = the sum over (N, HW), P_c = the number of positives, plane value = S_c / max(P_c, 1);  heat = mean over the heat
 *            planes.  Powers are left-to-right fp32 products (q^0 = 1, q^1 = q, q^2 = q q, q^3 = (q q) q, ...).
 *            d/dx positive: alpha p omp^alpha log p - omp^(alpha + 1);  negative: (1 - y)^beta (p^(alpha + 1) - alpha p^alpha omp log(1 - p))
 *   BCE plane c   torch BCEWithLogitsLoss(pos_weight): max(x, 0) - x y + l1p + (pw_c - 1) y softplus(-x) per entry, the mean over all
 *            N HW (number of BCE planes) entries;  d/dx = p - y - (pw_c - 1) y omp  (the pixel term of vk_seg_loss at pix_smooth 0)
 *   neither       the plane is not read
 * total = w_heat heat + w_bce bce.  Up to four fp32 element values are added, then accumulated in fp64; per-workgroup partial rows are
 * added in a fixed order; positives are counted in integers; no float atomics: the same inputs give the same bytes.  16-byte accesses
 * when HW % 4 == 0 and the buffers are 16-byte aligned.  Targets outside [0, 1] are the caller's error (not checked); a NaN propagates.
 * struct_size must be the size of the structure. */
#define VK_KP_LOSS_MAX_EXP 8
typedef struct vk_kp_loss_cfg {
  uint32_t struct_size;
  uint32_t heat_planes, bce_planes;
  float w_heat, w_bce;
  int32_t alpha, beta;
  float pos_threshold;              /* in (0, 1] */
  int32_t has_pos_weight;
  float pos_weight[16];
} vk_kp_loss_cfg;
size_t vk_kp_loss_cfg_size(void);
/* Device scratch (8-byte aligned; the caller owns it); 0 for arguments out of range: N, HW >= 1, HW <= 2^28, N C <= 65535,
 * N C HW <= 2^31 - 1.  It need not be cleared or kept between calls; a workspace of exactly this size is accepted and nothing past it
 * is touched. */
size_t vk_kp_loss_workspace_bytes(int N, int C, int HW);
/* loss_out float[8] = {total, heat, bce, 0, ...}; positives (optional) int64[16]: P_c of the heat planes, 0 elsewhere; dlogits
 * (optional) = grad_scale * d total / dx: accumulate = 0 writes every entry (planes with neither rule get 0), accumulate = 1 adds
 * into the planes that have a rule and leaves the others untouched.  Every argument error is found on the host before any launch
 * (VK_ERR_ARG and vk_last_error_string). */
int vk_kp_loss(const vk_kp_loss_cfg* cfg, int N, int C, int HW, const float* logits, const float* target, void* workspace,
               size_t workspace_bytes, float* loss_out, int64_t* positives, float* dlogits, float grad_scale, int accumulate,
               void* stream);

/* Second-pass inference on one window per indentation (zoom.hip).  The first pass detects on the letterboxed
 * map; for every detection one S x S window is cut from the uint8 source image at the finest scale that still shows the indentation
 * whole, the caller segments, fits and refines there (vk_geom_*, vk_subpix_refine with the window's affine row), and vk_zoom_merge
 * puts the result back into the first pass's slot, or keeps the first pass's record.
 *
 * Coordinates: source pixel i covers [i, i + 1) and has its centre at i + 0.5.  A window is (X0, Y0, s): the continuous coordinate of
 * its top-left edge and s source pixels per output pixel.  Output pixel x has its centre at X0 + (x + 0.5) s, the source pixel
 * coordinate u = X0 + (x + 0.5) s - 0.5; as an affine row of vk_subpix_refine that is inv_scale = s, ox = -(X0 + 0.5 s - 0.5) / s.
 * All arithmetic below is IEEE float64 with contraction off, evaluated as written, left to right inside the parentheses.
 *
 * vk_zoom_windows.  records / record_stride / box_offset / valid_offset / counts / max_components: the first pass's records, read in
 * place as vk_subpix_refine reads them.  affine: device double [batch][3] or NULL (0, 0, 1).  sizes: device int32 [batch][2] = (h, w)
 * of the source images.  For slot t < min(max(counts[b], 0), max_components) with valid != 0, in ascending (b, t):
 *   sx_q = (box[2 q] - ox) * inv, sy_q = (box[2 q + 1] - oy) * inv, q = 0 .. 3;  cx = (((sx_0 + sx_1) + sx_2) + sx_3) * 0.25, cy alike;
 *   e = 0; for q = 0 .. 3: e = max(e, fabs(sx_q - cx)), then e = max(e, fabs(sy_q - cy));
 *   raw = (margin * (2 * e)) / S;  s = raw; unless raw >= s_min: s = s_min, bit SCALE_CLAMPED_LO; if raw > s_max: s = s_max, bit
 *   SCALE_CLAMPED_HI;  X0 = (cx + 0.5) - (S * s) * 0.5, Y0 alike;  bit CLIPPED unless X0 >= 0, Y0 >= 0, X0 + S * s <= w and
 *   Y0 + S * s <= h.
 * The first max_windows of them are written to windows[] in that order (no atomics: one workgroup scans the slots); *n_windows (device
 * int32) = min(their number, max_windows).  Nothing else is written.  Host checks (VK_ERR_ARG before anything touches the stream): null
 * or misaligned buffers, the record layout as in vk_subpix_refine, batch 1..65535, max_components 1..4096, S 1..16384,
 * 0.25 <= s_min <= s_max <= 64, margin in [1, 8], max_windows 1..65535.
 *
 * vk_zoom_gather.  windows: device, n of them (1..65535).  images_host: n_images entries, checked on the host (ptr != 0, h, w 1..16384,
 * stride >= 3 w) and copied to images_dev (device, n_images * sizeof(vk_zoom_image)) on the stream; uint8 BGR, row r of image m at
 * ptr + r * stride.  out: device float32 [n][3][S][S], RGB planes.  The value of channel c of output pixel (x, y) is the mean of the
 * piecewise-constant source image over the square of side f = max(s, 1) centred on the pixel's centre:
 *   ax = (X0 + (x + 0.5) * s) - f * 0.5, bx = ax + f; taps i = floor(ax) .. floor(bx), weight wx_i = min(bx, i + 1) - max(ax, i); ay, by,
 *   wy_j alike with Y0 and y.  row_j = sum over i ascending from 0.0 of wx_i * p[j][i][c]; total = sum over j ascending from 0.0 of
 *   wy_j * row_j; value = total / (f * f).  p is pad_value where (i, j) lies outside the image.
 * For s <= 1 this is bilinear interpolation, for s >= 1 the area average, at s = 1 with integer X0, Y0 the source pixel itself.  Then
 * q = min(max((int)rint(value), 0), 255) and out = ((float)q / 255.f - mean) / std, the float32 expression of vk_letterbox_preprocess.
 * A window with map outside 0 .. n_images - 1, s outside [0.25, 64] or fabs(X0), fabs(Y0) above 2^30 (a NaN included) gives pad_value
 * everywhere.  One workgroup per 32 x 8 output tile of one window; every thread takes the sums of its pixel straight from memory.  Under
 * VK_ZOOM_STAGED (flags; the form that measured slower and is kept as a cross-check) the tile's source footprint is staged in LDS as
 * aligned dwords, the horizontal pass leaves row sums in LDS and the vertical pass reads them, unless the footprint does not fit the LDS
 * (s above about 5): the same operations in the same order, the same bits.  Every tap is checked against h, w; every offset is 64-bit.
 *
 * vk_zoom_merge.  windows / n: as above, n >= 0 (host count).  records2 .. max_components2: the second pass's geometry records
 * [n][max_components2] and counts2 [n]; quads2: its vk_subpix_quad [n][max_components2] (all three may be NULL when n == 0).  coarse:
 * the first pass's vk_subpix_quad [batch][max_components]; counts: the first pass's.  For slot t of map b below
 * min(max(counts[b], 0), max_components), the window k with (map, slot) = (b, t) is looked up (binary search: the windows are sorted).
 * Candidates: u < min(max(counts2[k], 0), max_components2) with valid != 0 in the record and in quads2, whose int32 polygon contains the
 * window centre: with P = (S, S) and the doubled corners A_q = 2 * box_q, the four cross products (A_q+1 - A_q) x (P - A_q) in int64 are
 * all >= 0 or all <= 0 (a point on an edge is inside).  Target: the candidate of largest area, the lowest u on a tie.  out[b][t] is
 * quads2[k][target] with label and area of coarse[b][t], and status ZOOMED, when a target exists (else NO_TARGET), none of its four
 * flags has a bit of VK_ZOOM_FAIL_MASK (else REFINE_FAILED) and fabs(d_mean - coarse d_mean) <= agree * coarse d_mean (else DISAGREES);
 * in every other case, and when there is no window (NO_WINDOW), out[b][t] = coarse[b][t].  status [batch][max_components] int32 is the
 * case or-ed with the window's bits, scale [batch][max_components] double the window's s (0 without a window); both are written for
 * every slot, NO_WINDOW and 0 from min(count, max_components) on, where out is not touched.  One thread per slot, no atomics, no
 * workspace.  Host checks: as vk_zoom_windows, plus agree finite and >= 0. */
#define VK_ZOOM_CLIPPED 1
#define VK_ZOOM_SCALE_CLAMPED_LO 2
#define VK_ZOOM_SCALE_CLAMPED_HI 4
#define VK_ZOOM_ZOOMED 16
#define VK_ZOOM_NO_TARGET 32
#define VK_ZOOM_REFINE_FAILED 64
#define VK_ZOOM_DISAGREES 128
#define VK_ZOOM_NO_WINDOW 256
#define VK_ZOOM_FAIL_MASK 0x7f   /* every VK_SUBPIX_* bit */
#define VK_ZOOM_STAGED 1
typedef struct vk_zoom_params {
  int S, max_windows;
  double margin, s_min, s_max;
} vk_zoom_params;
typedef struct vk_zoom_window {
  int map, slot, status, pad;
  double X0, Y0, s;
} vk_zoom_window;
typedef struct vk_zoom_image {
  uint64_t ptr;                 /* device address of pixel (0, 0) */
  int h, w;
  int64_t stride;               /* bytes between rows, >= 3 w */
} vk_zoom_image;
int vk_zoom_windows(const vk_zoom_params* params, int batch, const void* records, size_t record_stride, size_t box_offset,
                    int valid_offset, const int32_t* counts, int max_components, const double* affine, const int32_t* sizes,
                    vk_zoom_window* windows, int32_t* n_windows, void* stream);
int vk_zoom_gather(int n, int S, const vk_zoom_window* windows, int n_images, const vk_zoom_image* images_host, void* images_dev,
                   int pad_value, int flags, float* out, void* stream);
int vk_zoom_merge(int S, double agree, int n, const vk_zoom_window* windows, const void* records2, size_t record_stride2,
                  size_t box_offset2, int valid_offset2, const int32_t* counts2, int max_components2, const vk_subpix_quad* quads2,
                  int batch, int max_components, const int32_t* counts, const vk_subpix_quad* coarse, vk_subpix_quad* out,
                  int32_t* status, double* scale, void* stream);

/* Validation panels and detection overlays (render.hip): the last stage of the reference's three programs, the
 * drawing of what was measured, without leaving the device.  Everything below is integer arithmetic or float arithmetic in a fixed
 * order with contraction off, so a restatement from this text gives the same bytes (tests/render_ref.py).  The thick-line rule, the
 * font and the absence of antialiasing are this library's own; they are not OpenCV's.  No kernel uses atomics or a workspace; every
 * read and write is checked against the sizes given, every byte offset is 64-bit.  All host checks return VK_ERR_ARG before anything
 * touches the stream.
 *
 * The blend of a base byte a and an overlay byte c (vk_render_blend: colour BGR, alpha the weight of the base, beta of the overlay):
 *   q = sat_u8(rint(((float)a * alpha + (float)c * beta) + gamma)): float32, every operation rounded on its own, rint to nearest with
 *   ties to even, then 0 for r <= 0 and 255 for r >= 255.  This is the definition cv2.addWeighted documents for 8-bit images.  alpha,
 *   beta and gamma lie in [-1e6, 1e6].
 *
 * vk_render_val_panels: train.py's four-panel image.  x: device float32 [N][3][H][W] (RGB planes, normalised), y and prob: float32
 * [N][1][H][W]; mean, std: host double[3], |.| <= 1e6; N 1..65535, H, W 1..16384.  out: device uint8, row r of image n at
 * out + (n * H + r) * row_stride, row_stride >= 12 W (and <= 2^31); a row holds four panels of W pixels of three bytes, bytes from 12 W
 * on are never written.  Panel 0: per RGB plane k, v = (((double)x * std[k]) + mean[k]) * 255.0 in float64 as written; the byte is 0
 * unless v > 0 (so for a NaN), 255 for v >= 255, else (int)v (truncation); stored B, G, R.  Panel 1: p = y * 255.f in float32; 0 unless
 * p > 0, 255 for p >= 255.f, else (int)p; three times.  Panel 2: the same from prob.  Panel 3: per channel the blend of panel 0's
 * byte with blend.color where panel 2's byte is > 127, with 0 elsewhere.  Under VK_RENDER_RGB (flags) the three bytes of every pixel
 * of every panel are stored in the reverse order.
 *
 * vk_render_primitives: the drawing list, from the records in place.  records / record_stride / valid_offset / counts /
 * max_components / affine: as in vk_subpix_refine, but record_stride is a multiple of 8 and records is 8-byte aligned.  diag_offset: a
 * double (d_mean) in the record.  coord_mode and box_offset: VK_RENDER_COORD_BOX: int32 box[8] at box_offset and float cx, cy at
 * center_offset; VK_RENDER_COORD_V: double v[8] at box_offset; VK_RENDER_COORD_VS: double vs[8] at box_offset, which are source
 * coordinates already: the affine row is not applied.  center_offset is read in BOX mode only.  With (ox, oy, inv) the affine row, or
 * (0, 0, 1): m_x = ((double)c_x - ox) * inv, m_y = ((double)c_y - oy) * inv for the four corners and, in BOX mode, for (cx, cy); in the
 * other modes cx = (((m_x0 + m_x1) + m_x2) + m_x3) * 0.25, cy alike.  A slot t < min(max(counts[b], 0), max_components) with
 * valid != 0 is skipped (counted in skipped[b], takes no part in what follows) unless fabs of all eight m and of cx, cy is
 * <= VK_RENDER_MAX_COORD = 2^20 (a NaN fails); otherwise it is drawn: corner = (int32)rint(m) (ties to even), anchor =
 * ((int)cx + 6, (int)cy - 6) (truncation).
 *   rank = the number of drawn slots u of the map with area_u > area_t, or area_u == area_t and u < t (area: the int at byte 4);
 *   idx = rank + 1, the number detections.sort(key=area, reverse=True) gives.  color = palette[rank % 8].
 *   diag = (i1, j1, i2, j2): among the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3) of corners the first one of largest squared distance
 *   in int64, and the other two corners ascending.
 *   label = "#<idx> mean=<D>px", D = the digits of printf("%.1f", d_mean) for 0 <= d_mean < 1e6, else "?":  hi = d * 10.0,
 *   lo = fma(d, 10.0, -hi), f = floor(hi), r = ((hi - f) - 0.5) + lo; n = f + 1 when r > 0, f when r < 0, the even one of the two when
 *   r == 0; D = n / 10, '.', n % 10.  (-0.0 prints 0.0.)  label_len characters, the rest of label[] is 0.
 *   bbox = (x0, y0, x1, y1), inclusive, with p = (thickness + 1) / 2 and L = label_len: x0 = min(min corner x - p, anchor x),
 *   y0 = min(min corner y - p, anchor y - 7 text_scale + 1), x1 = max(max corner x + p, anchor x + 6 text_scale L - 1),
 *   y1 = max(max corner y + p, anchor y).
 * prims: device vk_render_prim [batch][max_components], 8-byte aligned; the record of rank r of map b is written to prims[b][r], every
 * byte of it (pad = 0); drawn[b] = their number, skipped[b]: device int32 [batch].  Nothing else is written.  Host checks: null or
 * misaligned buffers, batch 1..65535, max_components 1..4096, the offsets inside the record and aligned, thickness and text_scale 1..8.
 *
 * vk_render_draw: views_host: batch entries of vk_render_view, checked on the host (h, w 1..16384; src, mask != 0; every stride at
 * least its row and <= 2^31; a float mask 4-byte aligned; at least one output) and copied to views_dev (device, 8-byte aligned,
 * batch * sizeof(vk_render_view)) on the stream.  src: uint8 BGR, row r at src + r * src_stride.  mask: VK_RENDER_MASK_U8: uint8,
 * foreground where != 0; VK_RENDER_MASK_F32: float32, foreground where value > thresh in float32.  out[0] (vis_o): the source.  out[1]
 * (vis_b): 255 on the foreground, 0 elsewhere, three times.  out[2] (vis_v): per channel the blend of the source byte with blend.color on
 * the foreground and with 0 elsewhere.  An output address of 0 is not wanted.  prims / drawn / max_components: the list of
 * vk_render_primitives, or NULL for none; the first min(max(drawn[b], 0), max_components) records of map b are painted over every
 * output in list order, per record the four sides (0-1, 1-2, 2-3, 3-0) in color, then the two diagonals in diag_color, then the label in
 * color: per pixel the last one that covers it wins.  A record is not painted at all unless thickness and text_scale are 1..8, label_len
 * <= 24, every diag index < 4, every corner within +-2^20 and the anchor within +-2^21; and only inside its bbox.
 *   Segment A-B at thickness t covers pixel P iff 4 * dist^2(P, segment) <= t^2, in integers: d = B - A, e = P - A, L = d.d, u = e.d;
 *   if L == 0 or u <= 0: 4 e.e <= t^2; else if u >= L: 4 |P - B|^2 <= t^2; else 4 * cross(d, e)^2 <= t^2 * L, cross = d.x e.y - d.y e.x.
 *   With corners within +-2^20 and pixels in 0..16383: |d| components <= 2^21, |e| < 2^21, so L <= 2^43, |u| and |cross| < 2^44 and
 *   4 e.e < 2^45 fit int64; t^2 L <= 2^49, so a |cross| >= 2^26 cannot satisfy the test and is refused before it is squared, and
 *   4 cross^2 < 2^54 otherwise.
 *   Text: with s = text_scale, u = P.x - anchor.x, v = P.y - (anchor.y - 7 s + 1): inside when 0 <= u < 6 s label_len and 0 <= v < 7 s;
 *   cell = u / s, row = v / s, character k = cell / 6, column c = cell % 6; covered when c < 5 and bit (4 - c) of row `row` of the glyph of
 *   label[k] (vk_render_glyph) is set.  The anchor is the bottom-left pixel of the text.  A character without a glyph paints nothing.
 * One workgroup per 32 x 8 tile of one map tests the records' bboxes against its tile and keeps the hits in LDS in list order (ballot and
 * prefix count), then every pixel walks that list from its end; under VK_RENDER_DIRECT (flags; the form that measured slower, kept as a
 * cross-check) every pixel walks the whole list: the same bytes.
 *
 * vk_render_reduce: src uint8 [h][w][3] with src_stride -> dst [ceil(h / k)][ceil(w / k)][3] with dst_stride, k 1..16; per channel
 * (sum + n / 2) / n in integers over the n source pixels of the block (rows k Y .. min(k Y + k, h) - 1, columns alike).
 *
 * vk_render_glyph: host only; rows[7] of the 5 x 7 glyph of ch, top row first, bit 4 the left column; VK_ERR_ARG for a character the
 * label cannot contain (it contains "#0123456789 mean=.px?"). */
#define VK_RENDER_RGB 1
#define VK_RENDER_DIRECT 1
#define VK_RENDER_MASK_U8 0
#define VK_RENDER_MASK_F32 1
#define VK_RENDER_COORD_BOX 0
#define VK_RENDER_COORD_V 1
#define VK_RENDER_COORD_VS 2
#define VK_RENDER_MAX_COORD 1048576
#define VK_RENDER_LABEL_MAX 24
typedef struct vk_render_blend {
  uint8_t color[3];             /* B, G, R */
  uint8_t pad;
  float alpha, beta, gamma;
} vk_render_blend;
typedef struct vk_render_style {
  uint8_t palette[8][3];        /* B, G, R */
  uint8_t diag[3];
  uint8_t pad;
  int thickness, text_scale;    /* 1..8 each */
} vk_render_style;
typedef struct vk_render_prim {
  int32_t rank, slot;
  int32_t corner[8];            /* x0,y0 .. x3,y3 on the image that is drawn on */
  int32_t anchor[2];
  int32_t bbox[4];              /* x0, y0, x1, y1, inclusive */
  uint8_t diag[4];              /* i1, j1, i2, j2 */
  uint8_t color[3], label_len;
  uint8_t diag_color[3], thickness;
  uint8_t text_scale, pad[3];
  char label[VK_RENDER_LABEL_MAX];
} vk_render_prim;
typedef struct vk_render_view {
  uint64_t src;                 /* device addresses; 0 in out[] = not wanted */
  int64_t src_stride;
  uint64_t mask;
  int64_t mask_stride;          /* bytes */
  uint64_t out[3];              /* vis_o, vis_b, vis_v */
  int64_t out_stride[3];
  int h, w;
} vk_render_view;
int vk_render_val_panels(int N, int H, int W, const float* x, const float* y, const float* prob, const double* mean, const double* stdv,
                         const vk_render_blend* blend, int flags, uint8_t* out, int64_t row_stride, void* stream);
int vk_render_primitives(int batch, const void* records, size_t record_stride, size_t box_offset, int valid_offset, int diag_offset,
                         int center_offset, int coord_mode, const int32_t* counts, int max_components, const double* affine,
                         const vk_render_style* style, vk_render_prim* prims, int32_t* drawn, int32_t* skipped, void* stream);
int vk_render_draw(int batch, const vk_render_view* views_host, void* views_dev, int mask_kind, float thresh, const vk_render_blend* blend,
                   const vk_render_prim* prims, const int32_t* drawn, int max_components, int flags, void* stream);
int vk_render_reduce(int h, int w, int k, const uint8_t* src, int64_t src_stride, uint8_t* dst, int64_t dst_stride, void* stream);
int vk_render_glyph(int ch, uint8_t rows[7]);

/* AdamW (decoupled decay) over a flat fp32 parameter buffer; optionally emits the 16-bit working copy.
 * inv_scale multiplies the gradient first (GradScaler unscale / data-parallel averaging).
 * found_inf (optional int*): when *found_inf != 0 on the device the step is skipped: param, the moments and lowp_copy stay unwritten.
 * lowp_copy (optional) receives the updated parameters rounded to lowp_dtype (VK_BF16 / VK_F16); with VK_F32 it is not written. */
int vk_adamw_step(size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr,
                  float beta1, float beta2, float eps, float weight_decay, int step, float inv_scale,
                  const int* found_inf, void* lowp_copy, vk_dtype lowp_dtype, void* stream);
/* *found_inf |= any(!isfinite(grad)) */
int vk_amp_check_inf(size_t n, const float* grad, int* found_inf, void* stream);

/* The GradScaler protocol of the reference's CUDA branch (train.py:441-445, 610-611: scaler.scale(loss).backward();
 * scaler.step(optimizer); scaler.update()) without a host round trip.  torch.amp.GradScaler keeps its scale and its
 * found_inf flag as fp32 device scalars and hands them to an optimizer that declares _step_supports_amp_scaling:
 *
 * vk_amp_unscale_check = torch._amp_foreach_non_finite_check_and_unscale_ over the ONE flat gradient buffer:
 *   grad *= *inv_scale (device fp32; NULL or a value of exactly 1 leaves the buffer unwritten), *found_inf = 1.0f if any
 *   element is inf / nan (never cleared here: the caller zeroes it, as GradScaler does).  n % 4 == 0, grad 16-byte aligned.
 *   The product is IEEE: a result below 2^-126 is rounded to the subnormal grid, not flushed to zero.
 * vk_adamw_step_amp = vk_adamw_step with everything step-dependent read on the device: *found_inf != 0 (the test is `!= 0.0f`: 1, -1
 *   and NaN all skip) skips the update (param, moments and lowp_copy unwritten) and
 *   leaves *step_count (int32) as it is — GradScaler does not call optimizer.step() on an overflow; otherwise *step_count is
 *   incremented first and drives the bias corrections, and the gradient is multiplied by inv_scale / *grad_scale
 *   (grad_scale NULL: by inv_scale).  scratch4: float[4] device scratch owned by the caller. */
int vk_amp_unscale_check(size_t n, float* grad, const float* inv_scale, float* found_inf, void* stream);
int vk_adamw_step_amp(size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                      float beta2, float eps, float weight_decay, int* step_count, float inv_scale, const float* grad_scale,
                      const float* found_inf, float* scratch4, void* lowp_copy, vk_dtype lowp_dtype, void* stream);
/* Per-tensor AdamW (fine-tuning: torch skips a parameter whose grad is None and keeps one state["step"] per parameter).
 * segments (device): int64 [n_segments][3] = {elem_begin, elem_end, tensor_index} of the flat buffers, each tensor_index at most
 * once; step_counts (device): int32 per tensor_index, advanced like vk_adamw_step_amp's *step_count (not on an overflow) and driving
 * that segment's bias corrections.  blocks (device): int32 [n_blocks][2] = {segment, chunk}, one workgroup per chunk of
 * VK_ADAMW_SEGMENT_CHUNK elements, as vk_adamw_segment_blocks builds it on the host.  scratch: float[4 + 2 n_segments] device
 * scratch.  Element arithmetic, GradScaler protocol (grad_scale / found_inf / inv_scale) and skip rule are vk_adamw_step_amp's.
 * vk_adamw_segment_blocks (host only): writes the block table of `segments_host` into blocks_host (capacity rows; NULL: count
 * only) and returns the number of rows, or <0 on a bad segment. */
#define VK_ADAMW_SEGMENT_CHUNK 4096
int vk_adamw_segment_blocks(int n_segments, const int64_t* segments_host, int32_t* blocks_host, int capacity);
int vk_adamw_step_amp_segments(int n_segments, const int64_t* segments, int n_blocks, const int32_t* blocks, float* param,
                               const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1, float beta2, float eps,
                               float weight_decay, int* step_counts, float inv_scale, const float* grad_scale,
                               const float* found_inf, float* scratch, void* stream);
/* Param groups and global-norm gradient clipping (torch.optim param groups; torch.nn.utils.clip_grad_norm_ without a second write of
 * the gradient buffer).
 * vk_adamw_step_groups = vk_adamw_step_amp_segments with the five hyper-parameters of segment s taken from
 *   groups_host[segment_group[s]] (segment_group: device int32 [n_segments], 0 <= g < n_groups; groups_host: HOST array of n_groups
 *   entries, 1 <= n_groups <= VK_ADAMW_MAX_GROUPS, copied into the launch, so a scheduler may change it between calls), and with an
 *   optional clip coefficient: clip_coef (device fp32 scalar, or NULL) multiplies the gradient factor, which is
 *     (float)(((double)inv_scale / (double)*grad_scale) * (double)*clip_coef)   with grad_scale,
 *     (float)((double)inv_scale * (double)*clip_coef)                           without,
 *   and exactly that of vk_adamw_step_amp_segments when clip_coef is NULL.  Tables, counters, scratch (float[4 + 2 n_segments]),
 *   element arithmetic and skip rule (*found_inf != 0: nothing written, no counter advanced) are those of the call above; with one
 *   group and no coefficient the results are the same bits.
 * vk_grad_norm_segments: the norm of inv_scale * grad over the listed segments only (same segment and block tables; gaps and unlisted
 *   ranges are never read; any segment begin is allowed).  norm_kind VK_NORM_L2: sqrt of the sum of squares, squared and summed in
 *   double; VK_NORM_INF: the largest |g|, NaN if any element is NaN.  out (device float[2]): out[0] = total = norm * |inv_scale|,
 *   out[1] = min(max_norm / (total + 1e-6), 1), a NaN kept: torch.nn.utils.clip_grad_norm_'s coefficient, evaluated in double.
 *   partials: device double[n_blocks] scratch, fully overwritten by every call.  No atomics: the same input gives the same bits.
 *   max_norm must be a number >= 0. */
#define VK_ADAMW_MAX_GROUPS 8
typedef struct {
  float lr, beta1, beta2, eps, weight_decay;
} vk_adamw_group;
int vk_adamw_step_groups(int n_segments, const int64_t* segments, const int32_t* segment_group, int n_blocks, const int32_t* blocks,
                         float* param, const float* grad, float* exp_avg, float* exp_avg_sq, int n_groups,
                         const vk_adamw_group* groups_host, int* step_counts, float inv_scale, const float* grad_scale,
                         const float* found_inf, const float* clip_coef, float* scratch, void* stream);
#define VK_NORM_L2 0
#define VK_NORM_INF 1
int vk_grad_norm_segments(int n_segments, const int64_t* segments, int n_blocks, const int32_t* blocks, const float* grad,
                          int norm_kind, float inv_scale, float max_norm, double* partials, float* out, void* stream);

/* Averaged weights (vk.averaging: torch.optim.swa_utils.AveragedModel / timm's ModelEmaV2 over the flat buffers).
 * One element rule, with a the average, p the current value and w the fp32 weight of this update:
 *     w == 1:     a' = p                       (the first SWA sample, or decay 0: a copy, exactly)
 *     otherwise:  a' = fma(p - a, w, a)        (the difference rounded once, the fused multiply-add once)
 * The weight is resolved on the device by a one-workgroup prepare step from *count (device int32: updates already taken):
 *   *found_inf != 0 (the test of vk_adamw_step_amp: 1, -1 and NaN all skip): the average and *count stay as they are; otherwise
 *   t = *count + 1 is stored and w is formed in double and rounded once:
 *     VK_AVG_EMA: w = (float)(1.0 - d), d = (double)decay, or with warmup min((double)decay, (1 + t) / (10 + t))   (timm's rule);
 *     VK_AVG_SWA: w = (float)(1.0 / t).
 *   scratch: float[2] device scratch owned by the caller (scratch[0] = skip flag, scratch[1] = w).
 * vk_avg_update: ranges_host[0 .. n_ranges) (HOST array, 1 <= n_ranges <= VK_AVG_MAX_RANGES, copied into the launch; a range with
 *   n == 0 is skipped), all in ONE grid-stride launch after the prepare step: 16-byte accesses where avg and src of a range share their
 *   offset from a 16-byte boundary, scalar head and tail (or the whole range) otherwise.  No atomics, no workspace beyond scratch.
 *   avg and src of a range must not overlap and are 4-byte aligned.  found_inf: optional device fp32.
 * vk_avg_swap: exchanges avg[i] and src[i] over the same kind of ranges in one launch (src IS written here): each thread reads both
 *   values, then writes both.
 * vk_adamw_step_amp_avg = vk_adamw_step_amp followed by vk_avg_update({avg, param, n}, {extra_avg, extra_src, extra_n}) with the same
 *   found_inf, in two launches instead of four: each element of the parameter buffer runs the AdamW update and then the rule above on
 *   the value it just wrote; the grid-stride loop then runs on over the extra range (extra_n == 0: none) with the rule alone.  A
 *   skipped step skips both halves and advances neither counter.  Same element functions, same w: the same bits as the two calls.
 * Argument errors (null pointers, n_ranges outside 1..4, a misaligned range, decay outside [0, 1) or not a number, an unknown kind) return
 *   VK_ERR_ARG before anything touches the stream. */
#define VK_AVG_EMA 0
#define VK_AVG_SWA 1
#define VK_AVG_MAX_RANGES 4
typedef struct {
  int kind;      /* VK_AVG_EMA or VK_AVG_SWA */
  float decay;   /* in [0, 1); read by VK_AVG_EMA only */
  int warmup;    /* nonzero: VK_AVG_EMA's decay at update t is min(decay, (1 + t) / (10 + t)) */
} vk_avg_rule;
typedef struct {
  float* avg;
  const float* src;
  size_t n;
} vk_avg_range;
int vk_avg_update(int n_ranges, const vk_avg_range* ranges_host, vk_avg_rule rule, int* count, const float* found_inf, float* scratch2,
                  void* stream);
int vk_avg_swap(int n_ranges, const vk_avg_range* ranges_host, void* stream);
int vk_adamw_step_amp_avg(size_t n, float* param, const float* grad, float* exp_avg, float* exp_avg_sq, float lr, float beta1,
                          float beta2, float eps, float weight_decay, int* step_count, float inv_scale, const float* grad_scale,
                          const float* found_inf, float* scratch4, void* lowp_copy, vk_dtype lowp_dtype, float* avg, int* avg_count,
                          vk_avg_rule rule, float* avg_scratch2, float* extra_avg, const float* extra_src, size_t extra_n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Engine level: the whole network as one plan
 * ---------------------------------------------------------------------------------------------- */
typedef struct vk_unet vk_unet;

typedef struct {
  int N, size;          /* batch per GPU and input HEIGHT (size % 32 == 0) */
  vk_dtype dtype;       /* compute/storage type of activations: VK_F32 (exact path) or VK_BF16 / VK_F16 */
  int training;         /* 1: plan keeps everything backward needs */
  int width;            /* input WIDTH (width % 32 == 0); 0 = size, the square inputs every reference script produces (train.py:70-75,
                           infer_pth_gui.py:17-24 letterbox to img_size x img_size) — smp itself accepts any H, W divisible by 32 (r04) */
} vk_unet_config;

typedef struct {
  char name[96];        /* smp state_dict key, e.g. "encoder.layer1.0.conv1.weight" */
  int kind;             /* 0 conv weight (KRSC in the flat buffer), 1 vector param (bn weight/bias, head bias),
                           2 fp32 buffer (running_mean/var), 3 int64 buffer (num_batches_tracked) */
  int dims[4];          /* logical torch shape: OIHW for kind 0, [C] for 1/2, [] for 3 */
  int ndim;
  int64_t offset;       /* element offset in the flat param buffer (kind 0/1), the flat fp32 buffer
                           (kind 2) or the int64 counter array (kind 3) */
  int64_t numel;
} vk_tensor_info;

int vk_unet_create(const vk_unet_config* cfg, vk_unet** out);
/* smp.Unet(..., classes=C) for 1 <= C <= 16: segmentation_head.0 is [C][16][3][3] + bias [C], the logits [N][C][S][S].
 * vk_unet_create is classes = 1 (the binary model: same kernels, launches and workspace as before). */
int vk_unet_create_ex(const vk_unet_config* cfg, int classes, vk_unet** out);
int vk_unet_num_classes(const vk_unet* h);
/* smp.Unet(encoder_name=...) for the ResNet encoders the reference's config offers (train.py:357-379, 747-749): VK_ENC_RESNET18
 * (BasicBlocks 2-2-2-2), VK_ENC_RESNET34 (3-4-6-3: vk_unet_create_ex, the same plan) and VK_ENC_RESNET50 (torchvision v1.5 Bottlenecks
 * 3-4-6-3, expansion 4, its 1x1 layers on vk_conv1x1_*).  The tensor table, gradient buckets and the flag counts of
 * vk_unet_set_trainable / vk_unet_set_bn_frozen follow the encoder (vk_unet_num_tensors, vk_unet_num_buckets). */
#define VK_ENC_RESNET18 18
#define VK_ENC_RESNET34 34
#define VK_ENC_RESNET50 50
int vk_unet_create_enc(const vk_unet_config* cfg, int classes, int encoder, vk_unet** out);
int vk_unet_encoder(const vk_unet* h);
/* smp.Unet(in_channels=c), 1 <= c <= 4 (anything else: VK_ERR_ARG): encoder.conv1.weight is [64][c][7][7] (64 * 49 * c floats, the first
 * tensor of the flat buffer), vk_unet_forward reads x as [N][c][H][W] and vk_unet_set_input_grad's buffer is [N][c][H][W].  The stem's
 * kernels run on the same NHWC4 input whatever c is.  vk_unet_create_enc is in_channels = 3. */
int vk_unet_create_in(const vk_unet_config* cfg, int classes, int encoder, int in_channels, vk_unet** out);
int vk_unet_in_channels(const vk_unet* h);
void vk_unet_destroy(vk_unet* h);
/* Optional: run a training plan's weight-gradient kernels on a second, library-owned HIP stream beside the caller's stream
 * (fork per layer once dz is final, join at the end of every backward stage, before the stage's gradient bucket may be
 * read); the only host-side state the library keeps.  Measured +1.3 % step throughput on one GPU, but the overlapping
 * kernels slow each other (per-kernel durations grow by 30-90 %), and with RCCL's stream as a third party the split measured
 * slower — so it is OFF by default (enable = 1, or VK_SIDE_STREAM=1 in the environment, turns it on). */
int vk_unet_set_side_stream(vk_unet* h, int enable);
int vk_unet_num_tensors(const vk_unet* h);
int vk_unet_tensor_info(const vk_unet* h, int index, vk_tensor_info* out);
int64_t vk_unet_param_numel(const vk_unet* h);        /* flat param/grad/moment buffer length (padded) */
int64_t vk_unet_buffer_numel(const vk_unet* h);       /* flat fp32 BN-buffer length */
int64_t vk_unet_workspace_bytes(const vk_unet* h);
/* gradient buckets for data-parallel all-reduce, in backward completion order */
int vk_unet_num_buckets(const vk_unet* h);
int vk_unet_bucket_range(const vk_unet* h, int bucket, int64_t* elem_begin, int64_t* elem_end);

/* params/grads: flat fp32 [param_numel]; bn_buffers: flat fp32 [buffer_numel]; nbt: int64[46];
 * workspace: workspace_bytes.  grads may be NULL for an inference plan. */
int vk_unet_bind(vk_unet* h, float* params, float* grads, float* bn_buffers, int64_t* nbt, void* workspace,
                 size_t workspace_bytes);
/* re-pack the compute copies of the weights after the fp32 master changed (load_state_dict, optimizer step) */
int vk_unet_refresh_weights(vk_unet* h, void* stream);

/* x: fp32 NCHW [N][3][S][S] ([N][in_channels][S][S] for a plan of vk_unet_create_in); logits: fp32 [N][C][S][S] (C = classes).  training=1: batch statistics + running-stat update */
int vk_unet_forward(vk_unet* h, const float* x, float* logits, int training, void* stream);
/* target fp32 [N][1][S][S]; loss_out float[3]; computes dlogits for backward when the plan is a training plan */
int vk_unet_loss(vk_unet* h, const float* logits, const float* target, float* loss_out, float grad_scale,
                 float w_bce, float w_dice, void* stream);
/* Loss of any plan: mode VK_LOSS_BINARY (classes == 1; = vk_unet_loss), VK_LOSS_MULTILABEL (target fp32 [N][C][S][S]; with one class
 * it is the binary loss) or VK_LOSS_MULTICLASS (classes >= 2; target int64 [N][S][S], see vk_multiclass_loss for bad labels).  A mode
 * that does not fit the plan's classes is refused.  w_ce weighs the BCE / cross-entropy term. */
#define VK_LOSS_BINARY 0
#define VK_LOSS_MULTILABEL 1
#define VK_LOSS_MULTICLASS 2
int vk_unet_loss_ex(vk_unet* h, int mode, const void* logits, const void* target, float* loss_out, float grad_scale, float w_ce,
                    float w_dice, void* stream);
/* Loss of any plan from a configuration structure as vk_seg_loss takes it: C = the plan's classes, target per cfg->mode, loss_out float[8].  A
 * training plan's dlogits are left in the workspace for vk_unet_backward, as the two calls above do. */
int vk_unet_loss_cfg(vk_unet* h, const vk_seg_loss_cfg* cfg, const void* logits, const void* target, float* loss_out,
                     float grad_scale, void* stream);
/* The fused step with a Lovasz term: runs vk_seg_loss on seg_cfg as vk_unet_loss_cfg does (seg_cfg may be NULL: no such part), then
 * adds w_lovasz times the Lovasz gradient into the plan's dlogits and w_lovasz times its value into the total.  workspace: of
 * vk_lovasz_workspace_bytes(lovasz_cfg, N, classes, S S), the caller's.  loss_out float[16]: [0, 8) as vk_seg_loss (total and bad
 * labels include the Lovasz part), [8] the Lovasz value, [9] its bad labels. */
int vk_unet_loss_lovasz(vk_unet* h, const vk_seg_loss_cfg* seg_cfg, const vk_lovasz_cfg* lovasz_cfg, float w_lovasz, const void* logits,
                        const void* target, void* workspace, size_t workspace_bytes, float* loss_out, float grad_scale, void* stream);
/* The fused step with per-plane keypoint losses: vk_unet_loss_lovasz with the second part exchanged.  Runs vk_seg_loss on seg_cfg
 * (binary or multilabel; NULL: no such part, the first 8 floats are cleared), then vk_kp_loss adding into (or, without a seg part,
 * writing) the plan's dlogits.  workspace: of vk_kp_loss_workspace_bytes(N, classes, S S), the caller's.  loss_out float[16]: [0, 8)
 * as vk_seg_loss with the kp total added to [0], [8] heat, [9] bce, [10] the kp total.  Both configurations are checked before any
 * launch. */
int vk_unet_loss_kp(vk_unet* h, const vk_seg_loss_cfg* seg_cfg, const vk_kp_loss_cfg* kp_cfg, const void* logits, const void* target,
                    void* workspace, size_t workspace_bytes, float* loss_out, float grad_scale, void* stream);
/* dlogits: fp32 [N][C][S][S] gradient of the loss wrt the logits, or NULL to use the one vk_unet_loss
 * left in the workspace.  Runs backward stages [stage_begin, stage_end); stage i completes gradient bucket i.  Gradients are
 * accumulated into the flat grad buffer (caller zeroes it once per step, e.g. via vk_unet_zero_grad).
 * Only the gradients of TRAINABLE tensors (vk_unet_set_trainable) are written; the element ranges of frozen tensors are left
 * untouched, so after a zeroing they stay exactly zero.  A launch runs only if something it writes is needed: a weight or
 * gamma / beta gradient iff its tensor is trainable, a data gradient or BatchNorm-backward pass iff a trainable tensor lies at or
 * behind it in the backward order (head, decoder blocks 4..0, encoder blocks layer4.2 .. layer1.0, stem, and last the input when
 * vk_unet_set_input_grad gave it a buffer).  Stages behind the last trainable tensor are no-ops that return VK_OK.  BatchNorm layers
 * run in the modes of the training forward before (vk_unet_set_bn_frozen): a frozen layer's gamma / beta gradient needs its
 * reduction only when gamma or beta is trainable; its dz = gamma / sqrt(running_var + eps) * g never does. */
int vk_unet_backward(vk_unet* h, const float* dlogits, int stage_begin, int stage_end, void* stream);
/* Fine-tuning: one flag per parameter tensor (kinds 0 and 1 of vk_unet_tensor_info, in table order; nonzero = trainable, i.e.
 * torch's requires_grad).  n must be the number of parameter tensors (140), else VK_ERR_ARG.  Host-only; takes effect at the next
 * vk_unet_backward.  A new plan starts with every tensor trainable, which is the unpruned schedule. */
int vk_unet_set_trainable(vk_unet* h, const uint8_t* flags, int n);
/* Per-layer BatchNorm modes: one flag per BatchNorm layer (46, in the order of the num_batches_tracked entries of the tensor table;
 * nonzero = frozen statistics, torch's eval() of that module), else VK_ERR_ARG.  Host-only; takes effect at the next TRAINING
 * forward, which normalises a frozen layer with its running statistics, leaves its running_mean / running_var /
 * num_batches_tracked untouched and records the modes for the backward that follows it.  Eval forwards (training = 0) are unchanged. */
int vk_unet_set_bn_frozen(vk_unet* h, const uint8_t* flags, int n);
/* Gradient of the input: dx fp32 NCHW [N][3][H][W] ([N][in_channels][H][W] for a plan of vk_unet_create_in; or NULL: none, the default).  When set, vk_unet_backward's last stage WRITES dx
 * (the input ranks behind the stem in the pruning order, so every data gradient down to the stem runs even with every parameter
 * frozen).  Host-only. */
int vk_unet_set_input_grad(vk_unet* h, float* dx);
int vk_unet_zero_grad(vk_unet* h, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Data-parallel collectives for a host that is not PyTorch (SURVEY.md 8(b) "DP", 8(e)): RCCL over xGMI behind plain C.  The reference
 * is single-process; this is the new capability's C boundary.  One process per GPU (call hipSetDevice first); rank 0 creates the id
 * and hands its VK_COMM_ID_BYTES to the other ranks by any out-of-band means (file, socket, MPI); vk_comm_init is collective.
 * A data-parallel step below the C boundary:
 *     vk_unet_zero_grad; vk_unet_forward; vk_unet_loss;
 *     for stage s in 0 .. num_buckets-1:  vk_unet_backward(h, NULL, s, s + 1, compute_stream)
 *     [event on compute_stream -> comm_stream waits]  vk_allreduce_bucket(comm, grads + b0, b1 - b0, comm_stream) for the finished
 *         buckets — per bucket, or (recommended, see parallel.py / DESIGN.md section 5) ONE call over buckets 0..8, which are contiguous,
 *         once stage 8 is done, then bucket 9 after the last stage;
 *     [compute_stream waits for comm_stream]  vk_adamw_step(..., inv_scale = 1 / world, ...)
 * librccl.so is opened on first use; VK_ERR_STATE when it is absent.
 * ---------------------------------------------------------------------------------------------- */
#define VK_COMM_ID_BYTES 128
typedef struct vk_comm vk_comm;
int vk_comm_unique_id(void* id_out /* VK_COMM_ID_BYTES */);
int vk_comm_init(int rank, int world, const void* id, vk_comm** out);
int vk_comm_world(const vk_comm* c);
/* in-place SUM over all ranks of `count` fp32 gradients, enqueued on `stream` (ncclAllReduce) */
int vk_allreduce_bucket(vk_comm* c, float* grads, size_t count, void* stream);
/* in-place broadcast of `bytes` bytes from rank `root` (parameters / BatchNorm buffers at start, ncclBroadcast) */
int vk_comm_broadcast(vk_comm* c, void* buf, size_t bytes, int root, void* stream);
int vk_comm_destroy(vk_comm* c);

/* debugging / parity: pointer + shape of a named intermediate ("z:encoder.layer1.0.conv1", "out:encoder.layer1.0", ...) */
int vk_unet_debug_tensor(const vk_unet* h, const char* name, void** ptr, int dims_nhwc[4]);

#ifdef __cplusplus
}
#endif
#endif /* VK_UNET_H */
