/* libmauv_hip — C-ABI of the MI355X (gfx950) hot path of sams-tom/Multimodal-AUV.
 *
 * The reference is pure Python: its hot path calls into third-party framework kernels
 * (bayesian-torch 0.5.0 reparameterisation layers -> F.conv2d / F.linear / normal_ /
 * log1p(exp) on cuDNN/cuBLAS/curand).  Each entry point below replaces one of those call
 * sites (file:line in /root/reference/src/Multimodal_AUV unless noted) and is bound from
 * Python with ctypes by multimodal-auv_amd/mauv/_lib.py.
 *
 * Conventions:
 *  - every pointer is a DEVICE pointer owned by the caller (PyTorch caching allocator);
 *    the library never allocates device memory — workspace sizes come from *_workspace_*;
 *  - every call takes the hipStream_t to launch on (torch.cuda.current_stream()) and is
 *    asynchronous (no host synchronisation);
 *  - return 0 on success, < 0 on error (-1 bad argument, -2 launch failure);
 *    mauv_last_error() returns a thread-local message;
 *  - stateless and re-entrant; one process per GPU.
 *  - MC groups: G = number of Monte-Carlo samples processed by ONE launch (the reference's
 *    `for _ in range(num_mc): model(...)` loop, train/multimodal.py:107-112,
 *    inference/predictors.py:54-61, collapsed onto blockIdx.z).
 *  - layouts: activations NHWC [G][B][H][W][C] fp32; sampled weights KRSC [G][Cout][R][S][Cin];
 *    parameters/gradients in the reference's OIHW layout (bayesian-torch state_dict shapes).
 */
#ifndef MAUV_H
#define MAUV_H

#include <hip/hip_runtime.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- housekeeping ---------------------------------------------------------------------- */
const char* mauv_last_error(void);
int mauv_abi_version(void);

/* Kernel routing: ONE process-wide record, the only state the library keeps besides the
 * thread-local error message.  Every launch reads it; change it only while no other thread of
 * the process launches (a test or an A/B run between launches, or once at start-up).  Each
 * field selects between kernels that compute the same operation (outputs bit-identical, or — for
 * f32_math and the reparam backward — the same fp32 maths in another summation order); none
 * replaces a reference call site, so the defaults need never change.
 *   f32_math        arithmetic of the fp32 convs (mauv_conv2d_*_f32, mauv_stem_fwd_f32):
 *                   6 split (default): every fp32 operand split exactly into three bf16 planes
 *                   x = h + m + l, the six plane products h*h, h*m, m*h, h*l, l*h, m*m on
 *                   v_mfma_f32_32x32x16_bf16 with fp32 accumulation — the dropped terms are
 *                   <= 2^-24 |a*b|: fp32-grade results at 2.67x the f32-MFMA rate;
 *                   5 split1 (one accumulator everywhere); 3 split3 (planes h, m; products
 *                   h*h, h*m, m*h: ~2^-16 |a*b|, opt-in); 0 exact (v_mfma_f32_32x32x2_f32).
 *                   Initial value from MAUV_F32_MATH=split|split1|split3|exact.
 *   halo3           16-bit 3x3 / stride-1 convs over 64 -> 64 channels through an LDS image of
 *                   the input rows (conv_halo16.hip): 1 (default) / 0 the implicit GEMM.
 *   big16, big16_min_k  16-bit forwards on 256-row LDS-DMA tiles (conv_big16.hip): 1 (default)
 *                   the shapes where they measured faster (1x1, no pending BN, K >= 512,
 *                   N >= 256, >= 512 tiles), 2 every covered forward with K >= big16_min_k
 *                   (default and minimum 512: the K range its tests cover), 0 none.
 *   haloc16         16-bit 3x3 / stride-1 forwards and data gradients over 128-512 channels
 *                   through the chunked LDS row image (conv_haloc16.hip): 1 (default) with
 *                   32 x 64 wave tiles, 2 with 64 x 64 wave tiles, 3 the forwards only, 0 none.
 *   expand16        16-bit 1x1 expansion forwards (K = 64 / 128 / 256) through the
 *                   weight-stationary kernel (conv_expand16.hip): 1 (default) where it measured
 *                   faster, 2 every covered shape, 3 as 2 with 32-column waves at K = 128, 0 none.
 *   reparam_kernels bit 0: sampling by (output channel, channel range) blocks with vector KRSC
 *                   stores (bit-identical to the per-element kernel); bit 1: the reparameterisation
 *                   backward with 16-byte slab loads (another fixed sum order).  Default 3.
 * mauv_set_route validates every field and changes nothing on an error (-1). */
typedef struct MauvRoute {
  int f32_math;
  int halo3;
  int big16;
  int big16_min_k;
  int haloc16;
  int expand16;
  int reparam_kernels;
  int reserved[9];
} MauvRoute;
int mauv_get_route(MauvRoute* out);
int mauv_set_route(const MauvRoute* in);

/* ---- conv geometry (every mauv_conv2d_* entry point and sizing helper, fp32 and 16-bit) ----
 * Accepted, and tested against float64 per kernel family (tests/test_conv_rect_gpu.py): filter
 * rows R and columns S independent (R != S), image height H and width W independent (H != W),
 * one stride >= 1 and one zero padding pad >= 0 for both axes (pad may exceed R / 2 or S / 2:
 * outputs over padding only are 0 + bias), Ho = (H + 2 pad - R) / stride + 1 and Wo likewise
 * from W and S.  Weights are [G][Cout][R][S][Cin], weight-gradient slabs
 * [splits][G][Cout][R*S*Cin] with columns in (r, s, c) order.
 * Refused with a negative code before anything is computed or launched, mauv_last_error() naming
 * the entry point and the quantity: G, B, H, W, Cin, Cout, R, S or stride < 1; pad < 0; a filter
 * taller or wider than the padded image (Ho < 1 or Wo < 1); splits < 1 (weight gradients).  The
 * sizing helpers return that code in place of a count.  Not expressible: per-axis stride or
 * padding, dilation, groups, padding modes other than zeros. */

/* ---- implicit-GEMM convolution on MFMA (conv_gemm.hip) ---------------------------------
 * Replaces F.conv2d inside bayesian-torch Conv2dReparameterization.forward for every conv of
 * the three torchvision ResNet-50 trunks (models/base_models.py:15-18,
 * models/model_utils.py:57-61) and F.linear in LinearReparameterization.forward (attention
 * q/k/v/score, fc, fc1, fc2: models/base_models.py:38-41,60-65) as the 1x1, H=W=1 case.
 * x_strides (host pointer, nullable): element strides {group, batch, h, w, c} of x; NULL =
 * dense NHWC.  Group stride 0 = one input shared by all G samples (the stems read the
 * caller's NCHW images this way). */
/* x_scale/x_shift (nullable, [G][Cin]) + x_relu: the producing layer's BatchNorm(+ReLU)
 * applied while loading x (its normalised activation is never stored).
 * st_mean/st_m2/st_cnt (nullable): per-m-tile BatchNorm statistics of y written by the
 * epilogue ([G][nblk][Cout], [G][nblk][Cout], [G][nblk]; nblk from
 * mauv_conv2d_fwd_stat_blocks) for mauv_bn_stats_finalize. */
int mauv_conv2d_fwd_f32(const float* x, const long long* x_strides, const float* x_scale,
                        const float* x_shift, int x_relu, const float* w, const float* bias,
                        float* y, int G, int B, int H, int W, int Cin, int Cout, int R, int S,
                        int stride, int pad, float* st_mean, float* st_m2, float* st_cnt,
                        hipStream_t stream);
int mauv_conv2d_fwd_stat_blocks(int G, int B, int H, int W, int Cin, int Cout, int R, int S,
                                int stride, int pad);
/* cuDNN dgrad in loss.backward() (train/multimodal.py:138): dx = conv^T(dy, W_g)
 * (+ addend) (+ dx if accumulate); one launch per output-parity class (stride^2).
 * bn_* (nullable): dx is the output gradient of a BatchNorm(+ReLU) whose backward partial
 * sums (sum dz, sum dz*xhat per channel; [G][nblk][Cin], nblk from
 * mauv_conv2d_bwd_data_stat_blocks) the epilogue writes for mauv_bn_bwd's pre_p1/pre_p2;
 * the ReLU mask comes from bn_mask bits (mauv_bn_apply_mask), else bn_out, else from
 * bn_y*bn_scale+bn_shift.  addend_mask
 * (nullable): the addend counts only where these ReLU-mask bits ([G][B*H*W][Cin] / 8,
 * mauv_bn_apply_mask) are set — a block output's residual gradient dres = dout * mask added
 * without being stored. */
int mauv_conv2d_bwd_data_f32(const float* dy, const float* w, float* dx, const float* addend,
                             const unsigned char* addend_mask,
                             int accumulate, int G, int B, int H, int W, int Cin, int Cout,
                             int R, int S, int stride, int pad, const float* bn_y,
                             const float* bn_out, const unsigned char* bn_mask,
                             const float* bn_scale, const float* bn_shift,
                             const float* bn_mean, const float* bn_invstd, int bn_relu,
                             float* bn_p1, float* bn_p2, hipStream_t stream);
int mauv_conv2d_bwd_data_stat_blocks(int G, int B, int H, int W, int Cin, int Cout, int R,
                                     int S, int stride, int pad);
/* cuDNN wgrad (train/multimodal.py:138): split-K partial slabs ws[splits][G][Cout][R*S*Cin],
 * reduced deterministically by mauv_reparam_bwd.  mauv_conv2d_wgrad_splits sizes them. */
int mauv_conv2d_wgrad_splits(int G, int B, int H, int W, int Cin, int Cout, int R, int S,
                             int stride, int pad);
int mauv_conv2d_bwd_weight_f32(const float* x, const long long* x_strides, const float* x_scale,
                               const float* x_shift, int x_relu, const float* dy, float* ws,
                               int splits, int G, int B, int H, int W, int Cin, int Cout, int R,
                               int S, int stride, int pad, hipStream_t stream);
/* Their arithmetic: MauvRoute.f32_math (housekeeping section). */

/* ---- 16-bit implicit-GEMM convs (conv_gemm16.hip) -----------------------------------------
 * Same three GEMM views on v_mfma_f32_32x32x16_{bf16,f16}: dtype 0 = bf16 (BASELINE configs[2]
 * training), 1 = f16 (the reference predictor's torch.amp.autocast on a GPU,
 * inference/predictors.py:55).  x / w / y / dy / dx / addend are 16-bit words, statistics
 * partials and weight-gradient slabs fp32.  Cin and Cout must be multiples of 8 (the stems
 * run as GEMMs over im2col rows, mauv_stem_*; their former 8-channel padded form remains
 * valid), dgrad needs Cout % 32 == 0; x strides
 * are channel-contiguous multiples of 8.  Statistics partials: mauv_conv2d_fwd_stat_blocks.
 * y_shift (nullable, [Cout] fp32): y is STORED centred, y[.., c] = round16(conv - y_shift[c]):
 * the fp32 accumulators start at -y_shift[c], so the statistics partials are those of the stored
 * values too; pass the consuming BatchNorm's centre (its running mean where that dominates the
 * channel's spread, else 0) here and to mauv_bn_stats_finalize — the 16-bit rounding error of the
 * stored tensor then scales with the batch spread |y - mean| instead of |y|, the error the BN's
 * 1/std amplifies when a channel's mean is large.  Every route (the
 * implicit GEMM, 3x3 row images, LDS-DMA tiles, weight-stationary expansion) gives the same bits
 * for the same y_shift; so does the implicit GEMM's register-staged form that takes the shapes
 * outside the pipelined kernels (Cin % 64 != 0): the pipelined kernel's bits on the same operands
 * zero-padded to Cin % 64 == 0, outputs and statistics partials (it shares their epilogue). */
int mauv_conv2d_fwd_h16(int dtype, const void* x, const long long* x_strides,
                        const float* x_scale, const float* x_shift, int x_relu, const void* w,
                        void* y, int G, int B, int H, int W, int Cin, int Cout, int R, int S,
                        int stride, int pad, float* st_mean, float* st_m2, float* st_cnt,
                        const float* y_shift, hipStream_t stream);
/* A bottleneck's conv1 (1x1, stride 1, no padding) whose input is the previous bottleneck's
 * output, formed while conv1's tiles are loaded (replaces bn3 + residual add + ReLU, the
 * `out += identity; out = relu(out)` of torchvision's Bottleneck.forward under
 * models/base_models.py:74-90, followed by the next block's conv1):
 *   out = relu(y*scale + shift + r),  r = res, or res*res_scale + res_shift (the downsample
 *   branch's BN, res_scale / res_shift both non-NULL), per (group, channel) [G][Cin] parameters;
 * `out` ([G][B][H][W][Cin], written once) gets exactly mauv_bn_apply's values (out_mask,
 * nullable: mauv_bn_apply_mask's ReLU bits of it, for a training step) and y1 / the
 * statistics partials exactly mauv_conv2d_fwd_h16's on that `out`.  y, res: contiguous
 * [G][B][H][W][Cin]; Cin % 64 == 0, Cin <= 2048.  Returns 0 when launched, 1 when the shape is
 * outside the kernel (nothing launched: run mauv_bn_apply, then mauv_conv2d_fwd_h16), < 0 on an
 * argument error.  y1_shift: mauv_conv2d_fwd_h16's y_shift for y1. */
int mauv_conv2d_fwd_fold_h16(int dtype, const void* y, const float* scale, const float* shift,
                             const void* res, const float* res_scale, const float* res_shift,
                             void* out, unsigned char* out_mask, const void* w, void* y1, int G,
                             int B, int H, int W, int Cin, int Cout, float* st_mean,
                             float* st_m2, float* st_cnt, const float* y1_shift,
                             hipStream_t stream);
int mauv_conv2d_bwd_data_h16(int dtype, const void* dy, const void* w, void* dx,
                             const void* addend, int accumulate, int G, int B, int H, int W,
                             int Cin, int Cout, int R, int S, int stride, int pad,
                             hipStream_t stream);
/* mauv_conv2d_bwd_data_h16 whose epilogue also writes the BatchNorm-backward partial sums of
 * the BN whose output gradient dx is (bn_p1 = sum dz, bn_p2 = sum dz*xhat, [G][nblk][Cin], nblk
 * = mauv_conv2d_bwd_data_stat_blocks), for mauv_bn_bwd_ex's pre_p1/pre_p2: the standalone
 * partial pass over (y, dout) of models/resnet50_variational.py's BN backward disappears.
 * ReLU mask: bn_mask bits (mauv_bn_apply_mask) else bn_out > 0 else bn_y*bn_scale+bn_shift > 0.
 * addend_mask as in mauv_conv2d_bwd_data_f32.  bn_p1 and addend_mask NULL =
 * mauv_conv2d_bwd_data_h16.  Cout % 64 == 0 with partials or addend_mask. */
int mauv_conv2d_bwd_data_bn_h16(int dtype, const void* dy, const void* w, void* dx,
                                const void* addend, int accumulate, int G, int B, int H, int W,
                                int Cin, int Cout, int R, int S, int stride, int pad,
                                const unsigned char* addend_mask, const void* bn_y, const void* bn_out,
                                const unsigned char* bn_mask, const float* bn_scale,
                                const float* bn_shift, const float* bn_mean,
                                const float* bn_invstd, int bn_relu, float* bn_p1, float* bn_p2,
                                hipStream_t stream);
int mauv_conv2d_bwd_weight_h16(int dtype, const void* x, const long long* x_strides,
                               const float* x_scale, const float* x_shift, int x_relu,
                               const void* dy, float* ws, int splits, int G, int B, int H, int W,
                               int Cin, int Cout, int R, int S, int stride, int pad,
                               hipStream_t stream);

/* ---- variational sampling / KL (reparam.hip) --------------------------------------------
 * bayesian-torch Conv2dReparameterization/LinearReparameterization.forward:
 *   sigma = log1p(exp(rho)); eps.normal_(); w = mu + sigma*eps      (per MC sample g)
 * eps from Philox4x32-10(seed, sample0+g, layer, quad) — or the explicit eps [G][numel]
 * (parameter order) when non-NULL (parity tests).  out_gstride 0 = numel. */
int mauv_reparam_sample(const float* mu, const float* rho, const float* eps,
                        unsigned long long seed, unsigned long long sample0, unsigned int layer,
                        int G, int Cout, int Cin, int RS, float* out, long long out_gstride,
                        hipStream_t stream);
/* Backward of the above: dmu += sum_g dW_g; drho += sum_g dW_g * eps_g' * sigmoid(rho),
 * g' = g (fixed_sample < 0) or the sample `fixed_sample` for every g (bayesian-torch 0.5.0
 * semantics: its eps buffer is overwritten in place by later MC forwards while autograd
 * still references it; 0 <= fixed_sample < sample0 is an argument error).  dw element (s, g, i) at dw[s*dw_sstride + g*dw_gstride + i], i in
 * KRSC order with dw_cin (>= Cin; the 16-bit stems' padded channel count) channels. */
int mauv_reparam_bwd(const float* dw, int splits, long long dw_gstride, long long dw_sstride,
                     const float* mu, const float* rho, const float* eps,
                     unsigned long long seed, unsigned long long sample0, unsigned int layer,
                     int G, int Cout, int Cin, int RS, int dw_cin, float* dmu, float* drho,
                     long long fixed_sample, hipStream_t stream);
/* Their kernel forms: MauvRoute.reparam_kernels (housekeeping section). */
/* 16-bit sampled weights (dtype 0 = bf16, 1 = f16) for the 16-bit convs: KRSC with cin_pad
 * (>= Cin) input channels; pad channels are not written (zero-fill them once).  The sampling
 * arithmetic is fp32, only the stored weight is rounded.  out_gstride 0 = Cout*RS*cin_pad. */
int mauv_reparam_sample_h16(int dtype, const float* mu, const float* rho, const float* eps,
                            unsigned long long seed, unsigned long long sample0,
                            unsigned int layer, int G, int Cout, int Cin, int RS, int cin_pad,
                            void* out, long long out_gstride, hipStream_t stream);
/* The three sampling forms in one entry (dtype -1 = fp32, 0 = bf16, 1 = f16; KRSC with cin_pad
 * >= Cin channels, pad untouched) whose MC sample index is sample0 + *sample_base + g when
 * sample_base (nullable device counter) is given: a HIP graph captured around a forward
 * replays with fresh samples after the caller updates the counter. */
int mauv_reparam_sample_ex(int dtype, const float* mu, const float* rho, const float* eps,
                           unsigned long long seed, unsigned long long sample0,
                           const unsigned long long* sample_base, unsigned int layer, int G,
                           int Cout, int Cin, int RS, int cin_pad, void* out,
                           long long out_gstride, hipStream_t stream);
/* fp32 counterpart of mauv_reparam_sample_h16's padded layout (the fp32 stems' 4-channel KRSC
 * weights); same sampling as mauv_reparam_sample, pad channels not written. */
int mauv_reparam_sample_padded(const float* mu, const float* rho, const float* eps,
                               unsigned long long seed, unsigned long long sample0,
                               unsigned int layer, int G, int Cout, int Cin, int RS, int cin_pad,
                               float* out, long long out_gstride, hipStream_t stream);

/* get_kl_loss (bayesian-torch 0.5.0; called at train/multimodal.py:114,284 and
 * train/unimodal.py:130,262): sum over entries of mean(log s_p - log s + (s^2 + (mu-m_p)^2)
 * / (2 s_p^2) - 1/2), s = softplus(rho).  `table` is a device array of MauvKlEntry. */
typedef struct MauvKlEntry {
  const float* mu;
  const float* rho;
  float* dmu;
  float* drho;
  long long numel;
  float prior_mu;
  float prior_sigma;
} MauvKlEntry;
int mauv_kl_workspace_bytes(int n_entries);
int mauv_kl_fwd(const MauvKlEntry* table, int n, double* workspace, float scale, float* out,
                hipStream_t stream);
/* dmu/drho += (coef_dev ? *coef_dev : 1) * scale * dKL/d(mu, rho) (coef_dev: device scalar,
 * the upstream gradient — no host sync).  An entry's dmu and drho may each be NULL (a frozen
 * tensor has no gradient): that half of the entry is skipped, the other is still added. */
int mauv_kl_bwd(const MauvKlEntry* table, int n, const float* coef_dev, float scale,
                hipStream_t stream);
/* test hook: raw Philox words [nq][4] and the derived normals [nq][4] */
int mauv_philox_raw(unsigned long long seed, unsigned long long sample, unsigned int layer,
                    int nq, unsigned int* out_u32x4, float* out_normal4, hipStream_t stream);

/* ---- fused Adam (adam.hip) ------------------------------------------------------------------
 * torch.optim.Adam as the reference builds it (train/loop_utils.py:45-61: amsgrad=False,
 * maximize=False, L2 weight_decay) stepped for a whole table of fp32 tensors in one launch;
 * step = the (shared) 1-based step count used for bias correction.  amsgrad, maximize,
 * decoupled weight decay and several parameter groups: mauv_adam_step_ex below. */
typedef struct MauvAdamEntry {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  long long numel;
} MauvAdamEntry;
int mauv_adam_step(const MauvAdamEntry* table, int n, float lr, float beta1, float beta2,
                   float eps, float weight_decay, long long step, hipStream_t stream);
/* The step decision of train/multimodal.py:133-145 (skip on a non-finite loss; skip the step
 * AND the zero_grad on non-finite gradients; otherwise step + zero_grad) taken on the device, so
 * a training step has no host round trip.  64-byte device struct; the caller zero-initialises
 * it, writes ok_loss (1 = the loss is finite on every rank) before the backward and counts
 * the gradient arena's non-finite elements into `nonfinite` after it.  mode / step_size /
 * bc2_sqrt are written by mauv_adam_step_gated; step is the Adam step count (bias correction);
 * poisoned = the arena still holds a skipped step's non-finite gradients.
 * Global-norm gradient clipping: the caller writes max_norm (> 0 turns it on; 0, as in a
 * zero-initialised gate, is off and the step is what it was without these words) and norm_kind
 * (0 = L2, 1 = max-abs), and scans the gradients with mauv_grad_norm(..., &gate->grad_norm,
 * &gate->nonfinite, ...) in place of mauv_nonfinite_count.  The library reads max_norm and
 * grad_norm and writes clip_coef on every decision: min(1, max_norm / (grad_norm + 1e-6)) when
 * max_norm > 0, else 1.  A gated Adam step multiplies every gradient element by clip_coef as it
 * loads it (before maximize's negation and the weight-decay term, rounded on its own: the result
 * of clipping in place and then stepping); the clipped gradient is never written back. */
typedef struct MauvStepGate {
  int ok_loss, nonfinite, poisoned, mode;
  int step, stepped, skipped_loss, skipped_grad;
  float step_size, bc2_sqrt;
  float max_norm, grad_norm, clip_coef;
  int norm_kind;
  int reserved[2];   /* untouched by the library (mauv.train counts non-finite inputs in [1]) */
} MauvStepGate;
int mauv_adam_step_gated(const MauvAdamEntry* table, int n, float lr, float beta1, float beta2,
                         float eps, float weight_decay, MauvStepGate* gate, hipStream_t stream);
/* Every option of torch.optim.Adam's update and several parameter groups in one launch.  A row
 * names its group (0-based index into `groups`); max_exp_avg_sq is NULL unless that group has
 * MAUV_ADAM_AMSGRAD.  `groups` is a HOST array of n_groups (1..MAUV_ADAM_MAX_GROUPS) records,
 * copied into the kernel arguments, so a changed lr needs no device copy.  Element update, in
 * torch's order: g = -g (MAXIMIZE); p *= 1 - lr wd (DECOUPLED) or g += wd p, when wd != 0;
 * m += (1 - b1)(g - m); v = b2 v + (1 - b2) g^2; vmax = max(vmax, v) (AMSGRAD);
 * p -= lr / (1 - b1^t) * m / (sqrt(v or vmax) / sqrt(1 - b2^t) + eps).
 * gate == NULL: the ungated step at count `step` >= 1.  Otherwise `step` is ignored, the
 * decision of mauv_adam_step_gated runs first (same modes and counters) and every group steps
 * at the gate's count with its own lr and betas.  Rows whose group is out of range, or whose
 * group has AMSGRAD and no max_exp_avg_sq, are left untouched. */
#define MAUV_ADAM_MAX_GROUPS 8
#define MAUV_ADAM_AMSGRAD 1u
#define MAUV_ADAM_MAXIMIZE 2u
#define MAUV_ADAM_DECOUPLED 4u
typedef struct MauvAdamEntryEx {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  float* max_exp_avg_sq;
  long long numel;
  long long group;
} MauvAdamEntryEx;
typedef struct MauvAdamGroup {   /* 32 bytes */
  float lr, beta1, beta2, eps, weight_decay;
  unsigned int flags;
  int reserved[2];
} MauvAdamGroup;
int mauv_adam_step_ex(const MauvAdamEntryEx* table, int n, const MauvAdamGroup* groups,
                      int n_groups, long long step, MauvStepGate* gate, hipStream_t stream);
/* Dynamic loss scaling (torch.amp.GradScaler's algorithm) decided and applied on the device.
 * 32-byte device struct beside the gate; the caller initialises it (scale > 0, growth_factor,
 * backoff_factor, growth_interval; the rest 0) and runs the backward on loss * scale, so the
 * gradients the scan and the step see are `scale` times the true ones.  growth_interval == 0 is
 * a static scale: the library never changes `scale`.  The library writes unscale, the counters
 * and, when dynamic, scale and growth_tracker.  overflows counts the steps skipped on non-finite
 * scaled gradients, growths the times growth_tracker reached growth_interval.  The factors are
 * fp32: a scale update is (float)((double)scale * (double)factor), torch's rounding. */
typedef struct MauvLossScale {
  float scale, unscale, growth_factor, backoff_factor;
  int growth_interval, growth_tracker, overflows, growths;
} MauvLossScale;
/* The gated mauv_adam_step_ex with a loss scaler.  scaler == NULL: exactly
 * mauv_adam_step_ex(table, n, groups, n_groups, 0, gate, stream).  Otherwise one thread decides,
 * unscale = (float)(1.0 / (double)scale) being formed first, from the scale the backward used:
 *   ok_loss == 0   -> as without a scaler (mode 2, or 0 on a poisoned arena); scaler untouched
 *   nonfinite != 0 -> no step and the gradients are ZEROED (mode 2; poisoned = 0, stepped = 0,
 *                     skipped_grad += 1), overflows += 1; dynamic: scale *= backoff_factor,
 *                     growth_tracker = 0
 *   otherwise      -> Adam at step + 1, gradients zeroed (mode 3); dynamic: growth_tracker += 1,
 *                     and on reaching growth_interval scale *= growth_factor if the product is
 *                     finite, growth_tracker = 0, growths += 1
 * With max_norm > 0 the scanned grad_norm (of the scaled gradients) is rewritten as
 * grad_norm * unscale, the true norm (NaN stays NaN), and clip_coef is formed from that.  The
 * Adam kernel loads each gradient as fl32(fl32(g * unscale) * clip_coef): two roundings in
 * torch's order (GradScaler.unscale_, then clip_grad_norm_), never contracted into the
 * weight-decay term and never written back.  Argument errors (a null table / groups / gate,
 * n outside 1..65535, n_groups outside 1..8) return a negative code before any launch. */
int mauv_adam_step_ex_scaled(const MauvAdamEntryEx* table, int n, const MauvAdamGroup* groups,
                             int n_groups, MauvStepGate* gate, MauvLossScale* scaler,
                             hipStream_t stream);
/* Gradient accumulation decided on the device: a window of micro-batches whose gradients sum in
 * the arena and take ONE decision and one Adam step.  32-byte device struct beside the gate, as
 * MauvLossScale; the caller zero-initialises it and, per micro-batch, writes gate->ok_loss and
 * runs the backward (on loss * scale with a scaler: the scale cannot change inside a window).
 * mauv_accum_note is a micro-batch that does not close its window, on one thread: micro += 1;
 * if ok_loss == 0, bad_loss += 1 and gate->skipped_loss += 1; gate->stepped = 0, gate->mode = 0.
 * It touches nothing else (not nonfinite, poisoned, the step count or a scaler); the caller runs
 * no scan and no Adam launch for such a micro-batch. */
typedef struct MauvAccum {      /* caller zero-initialises */
  int micro;      /* micro-batches folded into the open window            (library) */
  int bad_loss;   /* of those, how many had ok_loss == 0                  (library) */
  float avg;      /* (float)(1.0 / micro) of the window just closed       (library) */
  int windows, dropped;         /* windows closed; closed without a step on a bad loss */
  int reserved[3];
} MauvAccum;
int mauv_accum_note(MauvStepGate* gate, MauvAccum* acc, hipStream_t stream);
/* mauv_adam_step_ex_scaled closing a window (the caller has scanned the arena into the gate, as
 * for every gated step).  acc == NULL: exactly mauv_adam_step_ex_scaled(table, n, groups,
 * n_groups, gate, scaler, stream); scaler may be NULL either way.  Otherwise one thread folds this
 * micro-batch in as mauv_accum_note does, forms avg = (float)(1.0 / (double)micro) and takes the
 * decision of mauv_adam_step_ex_scaled (of mauv_adam_step_ex without a scaler) with "ok_loss" read
 * as bad_loss == 0; then windows += 1, dropped += (bad_loss != 0), micro = bad_loss = 0.  So
 *   any non-finite loss in the window -> the window is dropped whole: no step, the arena zeroed
 *                     (mode 2) or left alone when poisoned (mode 0); the scaler is untouched
 *   nonfinite != 0 -> as without a window: poisoned and kept without a scaler; zeroed and one
 *                     backoff with one
 *   otherwise      -> one Adam step; the growth tracker moves once per window
 * With max_norm > 0 grad_norm becomes fl32(fl32(grad_norm * unscale) * avg), the norm of the
 * averaged, unscaled gradient, and clip_coef is formed from it.  The Adam kernel loads each
 * gradient as fl32(fl32(fl32(g * unscale) * avg) * clip_coef), each product rounded on its own,
 * never contracted into the weight-decay term and never written back.  A window of one (a fresh
 * MauvAccum) gives mauv_adam_step_ex_scaled's bits.  Argument errors (a null table / groups /
 * gate, n outside 1..65535, n_groups outside 1..8; a null gate or acc for mauv_accum_note) return
 * a negative code before any launch. */
int mauv_adam_step_ex_accum(const MauvAdamEntryEx* table, int n, const MauvAdamGroup* groups,
                            int n_groups, MauvStepGate* gate, MauvLossScale* scaler,
                            MauvAccum* acc, hipStream_t stream);
/* An exponential moving average (EMA) of the weights decided on the device: every parameter has a
 * shadow tensor that moves towards it after each Adam step that happened, and only then.  32-byte
 * device struct beside the gate, as MauvLossScale and MauvAccum; the caller zero-initialises it
 * and sets decay and warmup (and may set updates when it resumes a run). */
typedef struct MauvEma {
  float decay;     /* 0 < decay < 1                                            (caller)  */
  int   warmup;    /* 0: w = 1 - decay; 1: timm's warm-up, below                (caller)  */
  int   updates;   /* EMA updates taken so far                                  (library) */
  float weight;    /* the w of the last update; 1 = "copy"                      (library) */
  int   reserved[4];
} MauvEma;
/* mauv_adam_step_ex_accum with a weight EMA.  ema_rows is a DEVICE array of n float pointers, the
 * shadow tensor of each table row (row[i].numel floats), NULL for a row without one; ema is the
 * device MauvEma.  ema == NULL or ema_rows == NULL: exactly mauv_adam_step_ex_accum(table, n,
 * groups, n_groups, gate, scaler, acc, stream).  Otherwise one thread takes that entry's decision
 * (scaler and acc may each be NULL, as there) and then, if and only if the decision is "Adam step"
 * (mode bit 1), with n = updates and d = decay:
 *   n == 0    -> w = 1 (the first update copies, as torch.optim.swa_utils.AveragedModel)
 *   otherwise -> with warmup, d = min((double)decay, (1.0 + n) / (10.0 + n)); w = (float)(1.0 - d)
 * and weight = w, updates = n + 1.  Every other decision (a skip on the loss, non-finite gradients,
 * a poisoned arena, an overflow, a dropped window) leaves the MauvEma untouched, as does
 * mauv_accum_note.  The Adam kernel, having formed the new p of a row with a shadow, stores
 * e = p when w == 1, else e = fmaf(w, p - e, e) (torch's lerp for weights below 0.5) beside it:
 * one more read and write per element, no extra pass.  A step that does not update never touches
 * a shadow.  A row takes the loop (16-byte vectors or scalars) it takes without a shadow; a
 * shadow that is not 16-byte aligned is read and written float by float inside the vector loop,
 * so p, m, v and the zeroed gradients are mauv_adam_step_ex_accum's bits whatever its address.  Argument errors (a null table / groups
 * / gate, n outside 1..65535, n_groups outside 1..8) return a negative code before any launch. */
int mauv_adam_step_ex_ema(const MauvAdamEntryEx* table, int n, const MauvAdamGroup* groups,
                          int n_groups, MauvStepGate* gate, MauvLossScale* scaler, MauvAccum* acc,
                          float* const* ema_rows, MauvEma* ema, hipStream_t stream);
/* The same element update at a host-given weight w (0 < w <= 1; 1 copies), for steps the host
 * decided, and the element-wise exchange of parameters and shadows in place (no pointer changes:
 * cached tables stay valid), both over a DEVICE table of n rows in one launch with the Adam
 * kernels' grid; a row takes 16-byte vectors when both its pointers are 16-byte aligned.  Argument
 * errors (a null table, n outside 1..65535, w outside (0, 1]) return a negative code before any
 * launch. */
typedef struct MauvEmaRow {
  float* ema;
  const float* param;   /* written by mauv_ema_swap only */
  long long numel;
} MauvEmaRow;
int mauv_ema_update(const MauvEmaRow* rows, int n, float w, hipStream_t stream);
int mauv_ema_swap(const MauvEmaRow* rows, int n, hipStream_t stream);

/* ---- global gradient norm + non-finite scan, in-place clip (gradnorm.hip) -------------------
 * torch.nn.utils.clip_grad_norm_ over a DEVICE table of fp32 spans: the flat gradient arena is
 * one span, a plain parameter list one span per tensor; numel may be 0.  A span whose pointer is
 * not 16-byte aligned takes scalar loads up to the first boundary.
 * mauv_grad_norm: kind 0 = L2 (every square and the sum in double: no overflow or underflow for
 * finite fp32 input), kind 1 = max-abs.  Blocks write double partials into `workspace`
 * (mauv_grad_norm_workspace_bytes(n_spans) bytes, 8-byte aligned, no initialisation needed) and a
 * one-block kernel joins them in a fixed order: no floating-point atomics, the same data gives
 * the same bits.  *norm_out = the norm rounded once to fp32.  If any element was non-finite,
 * *norm_out = NaN (both kinds) and a positive number is added to *nonfinite (may be NULL), which
 * accumulates as with mauv_nonfinite_count.
 * mauv_grad_clip: g *= (float)min(1.0, (double)max_norm / ((double)*norm + 1e-6)) over the same
 * table, the coefficient formed on the device; nothing is written when it is 1 (also for a NaN
 * norm: non-finite gradients are left as they are).
 * Argument errors (n_spans outside 1..65535, a null table / workspace / norm, kind not 0 / 1,
 * max_norm not finite or <= 0) return a negative code before any launch. */
typedef struct MauvSpan {
  const float* p;
  long long numel;
} MauvSpan;
long long mauv_grad_norm_workspace_bytes(int n_spans);
int mauv_grad_norm(const MauvSpan* spans, int n_spans, int kind, void* workspace, float* norm_out,
                   int* nonfinite, hipStream_t stream);
int mauv_grad_clip(const MauvSpan* spans, int n_spans, const float* norm, float max_norm,
                   hipStream_t stream);

/* ---- BatchNorm2d (training mode, per MC group) + residual + ReLU (bn.hip) ---------------
 * torchvision Bottleneck bn1..3 / downsample.1 / stem bn1 in .train() for every MC pass
 * (train/multimodal.py:60,232; inference/predictors.py:27).  y/out [G][M][C], M = B*H*W. */
long long mauv_bn_workspace_floats(int G, long long M, int C);
int mauv_bn_fwd_train(const float* y, int G, long long M, int C, const float* gamma,
                      const float* beta, float* run_mean, float* run_var, float momentum,
                      float eps, float* workspace, float* mean, float* invstd, float* scale,
                      float* shift, const float* res, int relu, float* out,
                      hipStream_t stream);
/* statistics from per-m-tile partials written by mauv_conv2d_fwd_f32's epilogue: Chan merge,
 * mean/invstd/scale/shift [G][C], sequential running-stat update (run_* nullable);
 * workspace: mauv_bn_stats_workspace_floats(G, nblk, C) floats (2*G*C when nblk <= 128*64;
 * larger partial counts are merged in segments).  y_shift (nullable, [C]): the centre the 16-bit
 * forward stored y with (mauv_conv2d_fwd_h16); the partials are then those of the stored values
 * and mean / shift describe them (mean = mu_stored, shift = beta - mean*scale) for every
 * consumer of that tensor, while the running mean is updated with the true mean
 * mu_stored + y_shift; y_shift may alias run_mean (it is read before the update). */
long long mauv_bn_stats_workspace_floats(int G, int nblk, int C);
int mauv_bn_stats_finalize(int G, int nblk, int C, const float* pmean, const float* pm2,
                           const float* pcnt, const float* gamma, const float* beta,
                           float* run_mean, float* run_var, float momentum, float eps,
                           float* workspace, float* mean, float* invstd, float* scale,
                           float* shift, const float* y_shift, hipStream_t stream);
/* The forward apply, one implementation behind three entries:
 *   out = [relu](y*scale + shift (+ res')); res' = res*res_scale + res_shift when res_scale is
 *   non-NULL — the bottleneck's downsample BatchNorm applied inside the residual add (its output
 *   is never materialised); C % 8 == 0.
 * mauv_bn_apply_mask is the full form (dtype -1 = fp32, 0 = bf16, 1 = f16: the type of
 * y/res/out; scale/shift always fp32) with relu fixed to 1: it also writes the ReLU mask bits of
 * the stored output, mask[G][M][C/8] (bit e of byte j: out[8j+e] > 0, non-NULL), which the
 * backward reads instead of the 2-4 B output; C <= 2048.  It replaces the torchvision Bottleneck
 * bn3 -> += identity -> relu.  mauv_bn_apply is that form with dtype -1, relu free and no mask
 * (any C % 8 == 0), mauv_bn_apply_h16 the same with dtype 0 or 1: the same `out` bits. */
int mauv_bn_apply(const float* y, const float* scale, const float* shift, const float* res,
                  const float* res_scale, const float* res_shift, int relu, float* out, int G,
                  long long M, int C, hipStream_t stream);
int mauv_bn_apply_h16(int dtype, const void* y, const float* scale, const float* shift,
                      const void* res, const float* res_scale, const float* res_shift, int relu,
                      void* out, int G, long long M, int C, hipStream_t stream);
int mauv_bn_apply_mask(int dtype, const void* y, const float* scale, const float* shift,
                       const void* res, const float* res_scale, const float* res_shift, void* out,
                       unsigned char* mask, int G, long long M, int C, hipStream_t stream);
int mauv_bn_eval_params(int G, int C, const float* gamma, const float* beta,
                        const float* run_mean, const float* run_var, float eps, float* scale,
                        float* shift, hipStream_t stream);
/* The backward, defined by mauv_bn_bwd_ex (dtype -1 = fp32, 0 = bf16, 1 = f16: the type of
 * y/out/dout/dy/dres; statistics, scale/shift, workspace and dgamma/dbeta always fp32):
 *   dz = dout where the ReLU passed: by the mask bits of mauv_bn_apply_mask when mask is
 *        non-NULL (relu and out are then ignored), else all of dout when relu is 0, else where
 *        out > 0, else (out NULL: lazily-applied BN) where y*scale + shift > 0,
 *   dy = gamma*invstd*(dz - mean(dz) - xhat*mean(dz*xhat)),  dres = dz (nullable),
 *   dgamma += sum dz*xhat, dbeta += sum dz (over all groups; nullable).
 * pre_p1/pre_p2 (nullable, [G][pre_nblk][C]): the partial sums of dz and dz*xhat a data-gradient
 * epilogue already wrote (mauv_conv2d_bwd_data_bn_h16 / _f32): the partial pass over dout is
 * skipped, only the finalize and the apply pass run.  dy and dres both NULL: partials /
 * parameter gradients only.  C % 8 == 0, C <= 2048; workspace: mauv_bn_workspace_floats. */
int mauv_bn_bwd_ex(int dtype, const void* y, const void* out, const unsigned char* mask,
                   const void* dout, int relu, const float* mean, const float* invstd,
                   const float* scale, const float* shift, int G, long long M, int C,
                   float* workspace, void* dy, void* dres, float* dgamma, float* dbeta,
                   const float* pre_p1, const float* pre_p2, int pre_nblk, hipStream_t stream);
/* mauv_bn_bwd_ex with dtype = -1 and mask = NULL. */
int mauv_bn_bwd(const float* y, const float* out, const float* dout, int relu,
                const float* mean, const float* invstd, const float* scale, const float* shift,
                int G, long long M, int C, float* workspace, float* dy, float* dres,
                float* dgamma, float* dbeta, const float* pre_p1, const float* pre_p2,
                int pre_nblk, hipStream_t stream);
/* mauv_bn_bwd_ex with dtype 0 or 1, mask = NULL and no pre_p1/pre_p2. */
int mauv_bn_bwd_h16(int dtype, const void* y, const void* out, const void* dout, int relu,
                    const float* mean, const float* invstd, const float* scale,
                    const float* shift, int G, long long M, int C, float* workspace, void* dy,
                    void* dres, float* dgamma, float* dbeta, hipStream_t stream);
/* mauv_bn_bwd_ex with a non-NULL mask, out = shift = NULL and no pre_p1/pre_p2. */
int mauv_bn_bwd_mask(int dtype, const void* y, const unsigned char* mask, const void* dout,
                     const float* mean, const float* invstd, const float* scale, int G,
                     long long M, int C, float* workspace, void* dy, void* dres, float* dgamma,
                     float* dbeta, hipStream_t stream);
/* Frozen BatchNorm: normalisation with the running statistics (module.eval()).
 * mauv_bn_eval_stats is mauv_bn_eval_params (the same scale / shift bits) plus the two rows the
 * backward's xhat needs, copied per group: mean[g][c] = run_mean[c],
 * invstd[g][c] = 1 / sqrtf(run_var[c] + eps). */
int mauv_bn_eval_stats(int G, int C, const float* gamma, const float* beta,
                       const float* run_mean, const float* run_var, float eps, float* mean,
                       float* invstd, float* scale, float* shift, hipStream_t stream);
/* The backward of a BatchNorm whose statistics are constants of the step; the arguments are
 * mauv_bn_bwd_ex's without pre_p1/pre_p2, dz and the ReLU source rules are its own:
 *   dy = scale * dz (one fp32 product, one rounding to the storage type),  dres = dz (exact),
 *   dgamma += sum dz * (y - mean) * invstd,  dbeta += sum dz  (over all groups);
 * dy, dres, dgamma, dbeta each nullable.  dgamma and dbeta both NULL: one row-walk launch that
 * reads dout once and, beside it, only the ReLU source (y only for y*scale + shift; mean, invstd
 * and workspace may be NULL).  Otherwise one kernel sums mauv_bn_bwd_ex's partials (its geometry
 * and order) while it stores dy / dres, and mauv_bn_bwd_ex's finalize and parameter kernels
 * reduce them: no atomics, and dgamma / dbeta are the bits mauv_bn_bwd_ex accumulates for the
 * same operands.  C % 8 == 0, C <= 2048; workspace: mauv_bn_workspace_floats. */
int mauv_bn_bwd_frozen(int dtype, const void* y, const void* out, const unsigned char* mask,
                       const void* dout, int relu, const float* mean, const float* invstd,
                       const float* scale, const float* shift, int G, long long M, int C,
                       float* workspace, void* dy, void* dres, float* dgamma, float* dbeta,
                       hipStream_t stream);

/* ---- pooling (pool.hip): torchvision stem maxpool 3x3/2 pad 1 and adaptive avgpool ------ */
/* max-pool forward: C % 8 == 0 (the stem: 64); backward: C % 4 == 0. */
int mauv_maxpool_fwd(const float* x, int N, int H, int W, int C, float* y, unsigned char* idx,
                     hipStream_t stream);
int mauv_maxpool_bwd(const float* dy, const unsigned char* idx, int N, int H, int W, int C,
                     float* dx, hipStream_t stream);
/* The stem's pending BatchNorm + ReLU applied on load (out = maxpool(relu(y*scale[g] +
 * shift[g])), group g = image / (N/G)): the 112x112 BN output is never materialised.
 * Replaces the bn1 -> relu -> maxpool sequence of torchvision's ResNet stem
 * (models/base_models.py:15-16 builds it).  idx nullable (inference) in every maxpool entry. */
int mauv_maxpool_bn_fwd(const float* y, const float* scale, const float* shift, int G, int N,
                        int H, int W, int C, float* out, unsigned char* idx, hipStream_t stream);
int mauv_avgpool_fwd(const float* x, int N, int HW, int C, float* y, hipStream_t stream);
int mauv_avgpool_bwd(const float* dy, int N, int HW, int C, float* dx, hipStream_t stream);
/* 16-bit activations; the pooled features / their gradient stay fp32 (the head is fp32). */
int mauv_maxpool_fwd_h16(int dtype, const void* x, int N, int H, int W, int C, void* y,
                         unsigned char* idx, hipStream_t stream);
int mauv_maxpool_bwd_h16(int dtype, const void* dy, const unsigned char* idx, int N, int H,
                         int W, int C, void* dx, hipStream_t stream);
int mauv_maxpool_bn_fwd_h16(int dtype, const void* y, const float* scale, const float* shift,
                            int G, int N, int H, int W, int C, void* out, unsigned char* idx,
                            hipStream_t stream);
int mauv_avgpool_fwd_h16(int dtype, const void* x, int N, int HW, int C, float* y,
                         hipStream_t stream);
int mauv_avgpool_bwd_h16(int dtype, const float* dy, int N, int HW, int C, void* dx,
                         hipStream_t stream);
/* Stem input of the 16-bit path: fp32 NCHW [B][C][H][W] -> 16-bit NHWC [B][H][W][Cp], channels
 * C..Cp-1 zero (the caller's images are read once per trunk, shared by all MC samples). */
int mauv_pack_nchw_h16(int dtype, const float* x, int B, int C, int H, int W, int Cp, void* y,
                       hipStream_t stream);
/* Stem input of the fp32 path: NCHW -> NHWC [B][H][W][Cp] fp32, channels C..Cp-1 zero (Cp = 4:
 * the stem conv then runs the pipelined split kernel on 16-byte pixel quads). */
int mauv_pack_nchw_f32(const float* x, int B, int C, int H, int W, int Cp, float* y,
                       hipStream_t stream);

/* ---- stems over shared im2col rows (stem.hip) --------------------------------------------
 * conv1 of each trunk (7x7 / 2, models/base_models.py:18, model_utils.py:58-59) sees the same
 * images in every MC sample.  mauv_stem_im2col unrolls fp32 NCHW images once into rows
 * cols[m][k] (m = (b, oh, ow), k = c*R*S + r*S + s: the OIHW parameter order), zero for
 * k >= C*R*S up to Kp (Kp % 8 == 0); dtype -1 = fp32, 0 = bf16, 1 = f16 rows (RNE).
 * mauv_stem_fwd_{f32,h16}: y[g][m][c] = sum_k cols[m][k] w[g][c][k] as ONE GEMM with the G
 * weight sets stacked along N (w: [G][Cout][Kp], k >= C*R*S zero); per-m-tile BatchNorm
 * partials as mauv_conv2d_fwd_f32 with nblk = mauv_conv2d_fwd_stat_blocks of the stem.
 * fp32 needs Kp % 4 == 0, 16-bit Kp % 64 == 0 and Cout % 8 == 0.  The weight gradient is
 * mauv_conv2d_bwd_weight_* of a 1x1 conv over the rows (group stride 0). */
int mauv_stem_im2col(int dtype, const float* x, int B, int C, int H, int W, int R, int S,
                     int stride, int pad, int Kp, void* out, hipStream_t stream);
int mauv_stem_fwd_f32(const float* cols, const float* w, float* y, int G, int M, int Kp,
                      int Cout, float* st_mean, float* st_m2, float* st_cnt, hipStream_t stream);
int mauv_stem_fwd_h16(int dtype, const void* cols, const void* w, void* y, int G, int M, int Kp,
                      int Cout, float* st_mean, float* st_m2, float* st_cnt, const float* y_shift,
                      hipStream_t stream);

/* ---- the stems' data gradient (stem_dgrad.hip) --------------------------------------------
 * d loss / d images through conv1, SUMMED over the G MC samples (they share the images), in two
 * deterministic stages without atomics:
 *   mauv_stem_bwd_rows_{f32,h16}: drows[m][k] = sum_g sum_co dy[g][m][co] w[g][co][k], one GEMM
 *     M x Kp x (G*Cout) whose K loop runs over (g, co): the samples are summed in the fp32
 *     accumulators.  dy [G][M][Cout] and w [G][Cout][Kp] (the forward's sampled weights, k >=
 *     C*R*S zero) in fp32 (v_mfma_f32_32x32x2_f32) or dtype 0 = bf16 / 1 = f16
 *     (v_mfma_f32_32x32x16_*); drows [M][Kp] is always fp32, its padded columns come out 0.
 *     Kp % 8 == 0, Kp <= 2048, Cout % 8 == 0, M * Kp / 8 < 2^31; buffers 16-byte aligned.
 *   mauv_stem_col2im: dx[b][c][ih][iw] (fp32 NCHW, the images' layout) = the sum, in a fixed
 *     order, of drows[(b, oh, ow)][c*R*S + r*S + s] over the taps that reach the pixel — the
 *     adjoint of mauv_stem_im2col's fp32 rows; columns k >= C*R*S are never read.
 *     Kp >= C*R*S, B*C*H*W < 2^31. */
int mauv_stem_bwd_rows_f32(const float* dy, const float* w, float* drows, int G, int M, int Kp,
                           int Cout, hipStream_t stream);
int mauv_stem_bwd_rows_h16(int dtype, const void* dy, const void* w, float* drows, int G, int M,
                           int Kp, int Cout, hipStream_t stream);
int mauv_stem_col2im(const float* drows, int B, int C, int H, int W, int R, int S, int stride,
                     int pad, int Kp, float* dx, hipStream_t stream);

/* ---- fusion head + MC head (head.hip) ----------------------------------------------------
 * AdditiveAttention.forward (models/base_models.py:43-52) epilogues around the q|k|v and
 * score GEMMs (qkv rows [q | k | v], each hid wide; the reference's model: hid = 128):
 * t = tanh(q + k); o = v * softmax(s, dim=1) into the concat slot (:86) of ld comb_ld. */
int mauv_attn_t(const float* qkv, int rows, int hid, float* t, hipStream_t stream);
int mauv_attn_t_bwd(const float* dt, const float* t, int rows, int hid, float* dqkv,
                    hipStream_t stream);
int mauv_attn_out(const float* qkv, const float* s, int rows, int hid, float* comb, int comb_ld,
                  int comb_off, hipStream_t stream);
int mauv_attn_out_bwd(const float* dcomb, int comb_ld, int comb_off, const float* qkv,
                      const float* s, int rows, int hid, float* dqkv, float* ds,
                      hipStream_t stream);
/* bias gradients of the linear layers */
int mauv_colsum(const float* dy, int G, int rows, int N, float* out, int accumulate,
                hipStream_t stream);
/* The MC head: logits [G][B][C] fp32 (G MC samples), 1 <= C <= 4096 classes (the bound of
 * mauv_confusion_update); more is -1 with the bound in mauv_last_error().  B == 0 or G == 0
 * launches nothing and returns 0.  C <= 32 runs one thread per item (the reference's C = 7);
 * 33 <= C <= 4096 runs the many-class kernels: lanes along the class axis (coalesced rows), a
 * wave or a block per item, cross-lane max / sum / argmax, no scratch memory and no atomics, so
 * every output is bit-reproducible from run to run.  Rules both families share: argmax is the
 * first strict maximum (ties -> the lowest class index), a NaN never wins and an all-NaN row
 * gives class 0; non-finite logits propagate into the loss and the sums; eps_h is added inside
 * the log per sample, eps_pred in mauv_mc_finalize.
 * Labels (int64 [B]), many-class kernels: -100 (torch's ignore_index) leaves the item out of the
 * loss sum and of its divisor and zeroes the item's dlogits rows (no counted item: NaN loss, as
 * torch); any other label outside [0, C) makes the loss and the item's dlogits NaN (the step
 * gate then skips the batch, as the reference skips a non-finite loss); no label indexes memory
 * unchecked.  The C <= 32 kernels index mean[b][label] directly: labels must be in [0, C).
 * Sum order: the mean is the sum over g = 0..G-1 (fp32 for C <= 32; float64, rounded once, for
 * C > 32) over G; the many-class loss is a float64 sum over the items in a fixed order by one
 * block; sums[b][*] add the samples g = 0..G-1 in float64 in that order — with accumulate != 0
 * the C > 32 kernels continue from the stored value, so a call sequence over chunks of the
 * samples gives the bits of one call (C <= 32: the chunk's own sum is added to the stored one).
 * train/multimodal.py:121 (mean over MC), :127 (CrossEntropyLoss), :151 (argmax); labels, loss
 * and pred nullable */
int mauv_mc_mean_ce(const float* logits, const long long* labels, int G, int B, int C,
                    float* mean, float* loss, long long* pred, hipStream_t stream);
int mauv_mc_mean_bwd(const float* dmean, const float* gloss, const float* mean,
                     const long long* labels, int G, int B, int C, float* dlogits,
                     hipStream_t stream);
/* The same head under the criterion a training loop is handed (`criterion` of
 * train_multimodal_model / train_unimodal_model): what
 *   F.cross_entropy(logits.mean(0), labels, weight=class_weight, ignore_index=ignore_index,
 *                   reduction=("mean", "sum")[reduction], label_smoothing=label_smoothing)
 * and its autograd compute.  class_weight fp32 [C], null = all ones; reduction 0 = mean, 1 = sum.
 * With lp = log_softmax(mean[b]), p = exp(lp), y = labels[b], w the weights, W = sum_c w[c] and
 * an item counted iff y != ignore_index:
 *   nll_b = -w[y] lp[y];  smooth_b = -sum_c w[c] lp[c];  D = sum over counted items of w[y]
 *   (mean) or 1 (sum);  loss = (1 - eps) sum_b nll_b / D + (eps / C) sum_b smooth_b / D
 *   dlogits[g][b][c] = gloss / D ((1 - eps) w[y] (p[c] - [c == y]) + (eps / C) (p[c] W - w[c])) / G
 * mean and pred follow mauv_mc_mean_ce's rules (float64 sum over g rounded once, at every C).
 * Every C in 1..4096 runs the many-class kernels, so the label rules hold at C <= 32 too: a
 * label equal to ignore_index is ignored even when it is a valid class (its dlogits rows are
 * zero); any other label outside [0, C) makes the loss and that item's dlogits rows NaN and
 * adds nothing to D; no label indexes memory unchecked.  Sum order: per-item terms, their sums
 * and D in float64 in a fixed order by one block, rounded to float once, no atomics: the same
 * bits from run to run.  Mean reduction with no counted weight: D = 0 and the loss is NaN
 * (0 / 0, as torch); sum reduction with no counted item: 0.  denom [1] receives D; the backward
 * reads it as written and does not recompute it.  Non-finite logits or weights propagate into
 * the loss.  With class_weight null, label_smoothing 0, ignore_index -100 and reduction 0 the
 * forward gives mauv_mc_mean_ce's mean, loss and pred bit for bit at C > 32.
 * label_smoothing outside [0, 1], a reduction other than 0 / 1 and C > 4096 are -1; B == 0 or
 * G == 0 launches nothing and returns 0.  labels (then loss, denom are untouched) and pred
 * nullable in the forward. */
int mauv_mc_mean_ce_ex(const float* logits, const long long* labels, const float* class_weight,
                       float label_smoothing, long long ignore_index, int reduction, int G, int B,
                       int C, float* mean, float* loss, float* denom, long long* pred,
                       hipStream_t stream);
int mauv_mc_mean_bwd_ex(const float* gloss, const float* mean, const long long* labels,
                        const float* class_weight, float label_smoothing, long long ignore_index,
                        int reduction, const float* denom, int G, int B, int C, float* dlogits,
                        hipStream_t stream);
/* inference/predictors.py:65-84, train/multimodal.py:305-310, train/unimodal.py:298-308:
 * sufficient statistics sums[b] = {sum_g p (C), sum_g p^2 (C), sum_g H[p_g]} (float64,
 * all-reducible across MC-sharded ranks), then mean prob, unbiased variance (mean over
 * classes), aleatoric entropy, predictive entropy, argmax. */
int mauv_mc_stats(const float* logits, int G, int B, int C, float eps_h, double* sums,
                  int accumulate, hipStream_t stream);
int mauv_mc_finalize(const double* sums, int N, int B, int C, float eps_pred, float* mean_prob,
                     float* var_unc, float* alea, float* pred_entropy, long long* pred,
                     hipStream_t stream);
/* train/multimodal.py:133,141 NaN/Inf guards as one fused scan (*out += blocks with a
 * non-finite value) */
int mauv_nonfinite_count(const float* p, long long n, int* out, hipStream_t stream);

/* ---- input staging (staging.hip) ---------------------------------------------------------
 * data/datasets.py:239-250 per-tile transforms on the device: uint8 HWC tiles [B][H][W][C] as
 * PIL decodes them -> fp32 NCHW out = x / 255 (ToTensor), then (out - mean[c]) / std[c]
 * (Normalize; mean/std nullable = ToTensor only), bit-exact with torchvision's fp32 ops.
 * uifm_bt (nullable): also apply the underwater image formation model of
 * Examples/"Example training with image noise.py":55-93 to the result:
 *   t = exp(-bt[c] * (d * depth)); out = clamp(out * t + binf[c] * (1 - t), 0, 1)
 * with bt[c] = beta_c * turbidity computed in fp32 as the reference does and d the
 * [B][1][H][W] distance map (nullable = uniform 1, what the reference passes).
 * mauv_uifm: the same degradation on fp32 NCHW tiles [B][C][H][W]. */
int mauv_stage_u8(const unsigned char* x, int B, int H, int W, int C, const float* mean,
                  const float* stdv, const float* uifm_bt, const float* uifm_binf,
                  const float* dist, float depth, float* out, hipStream_t stream);
int mauv_uifm(const float* x, int B, int C, int H, int W, const float* bt, const float* binf,
              const float* dist, float depth, float* out, hipStream_t stream);
/* data/datasets.py:240-246 transforms.Resize((256, 256)) of the decoded tiles = PIL's
 * Image.resize(size, BILINEAR) (antialiased when downscaling), bit-exact with Pillow's 8-bit
 * separable resampler (libImaging/Resample.c; the reference pins pillow 11.0.0): uint8
 * [B][H][W][C] (1 <= C <= 4) -> uint8 [B][Ho][Wo][C] (out_u8), or — out_f32 instead — the
 * resized tile through mauv_stage_u8's ToTensor / Normalize / UIFM maths into fp32 NCHW
 * [B][C][Ho][Wo] in the same pass (mean/std, uifm_bt/binf, dist [B][1][Ho][Wo] nullable as
 * there).  workspace: mauv_resize_workspace_bytes(...) device bytes (coefficient tables and
 * the 8-bit horizontal-pass image), caller-owned; -1 = bad shape. */
long long mauv_resize_workspace_bytes(int B, int H, int W, int C, int Ho, int Wo);
int mauv_resize_u8(const unsigned char* x, int B, int H, int W, int C, int Ho, int Wo,
                   void* workspace, unsigned char* out_u8, const float* mean, const float* stdv,
                   const float* uifm_bt, const float* uifm_binf, const float* dist, float depth,
                   float* out_f32, hipStream_t stream);

/* ---- on-device augmentation of co-registered tiles (staging.hip) ---------
 * A move code is one byte per item, low 3 bits: bit0 = flip W, bit1 = flip H, bit2 = transpose
 * H <-> W applied last (the dihedral group of the square).  As a gather on fp32 NCHW:
 *   out[b][c][h][w] = v[b][c][h'][w'],  (p, q) = bit2 ? (w, h) : (h, w),
 *   h' = bit1 ? H - 1 - p : p,  w' = bit0 ? W - 1 - q : q
 * where v is what the un-augmented entry computes (Resize, ToTensor, Normalize and UIFM are
 * evaluated at the source pixel, the distance map dist[b][h'][w'] included).  The inverse of
 * code k is k when bit2 is clear, else k with bit0 and bit1 swapped.
 *
 * mauv_augment_draw: for item i = item0 + b,
 *   r = philox4x32_10(ctr = (i, step lo32, 0x41554721, step hi32), key = seed)
 * ops_out[b] = 0 (mode 0), r.x >> 30 (mode 1, flips) or r.x >> 29 (mode 2, dihedral);
 * turb_out[b] (nullable) = turb_lo + (turb_hi - turb_lo) * u, u = ((float)r.y + 0.5f) * 2^-32,
 * every operation rounded separately in fp32 (u can round to 1: turb lies in [lo, hi]).
 * Refused: mode outside 0..2, turb_hi < turb_lo, B < 0, item0 < 0 or item0 + B > 2^32.
 *
 * The *_aug staging entries take the arguments of their plain entry plus ops (u8 [B],
 * nullable = no move), turb (f32 [B], nullable) and allow_transpose.  With turb given the
 * uifm_bt / beta argument holds the plain beta[c] and the kernel forms beta[c] * turb[b] as one
 * fp32 product (the product the host forms for the plain entries: equal turbidities give the
 * plain entry's bits); turb goes with an fp32 output only.  allow_transpose != 0 needs a square
 * output tile (H == W; Ho == Wo for the resize) and is refused otherwise; with
 * allow_transpose == 0 only bits 0 and 1 of a code are read, so no code indexes outside a
 * non-square tile.  ops == NULL and turb == NULL run the plain entry's kernel.  The resize
 * entry applies the move where its last pass stores (8-bit or fused fp32 output).
 * mauv_stage_f32_aug: fp32 NCHW in and out, beta == NULL = a pure move.  A move is a gather, so
 * an x that overlaps the output in any byte is refused: always by mauv_stage_f32_aug, and by the
 * other two entries when ops are given.  Extents are refused by name (B < 0, C < 1, H or W < 1, an element
 * count of 2^62 or more). */
int mauv_augment_draw(unsigned long long seed, unsigned long long step, long long item0, int B,
                      int mode, float turb_lo, float turb_hi, unsigned char* ops_out,
                      float* turb_out, hipStream_t stream);
int mauv_stage_u8_aug(const unsigned char* x, int B, int H, int W, int C, const float* mean,
                      const float* stdv, const float* uifm_bt, const float* uifm_binf,
                      const float* dist, float depth, const unsigned char* ops,
                      const float* turb, int allow_transpose, float* out, hipStream_t stream);
int mauv_resize_u8_aug(const unsigned char* x, int B, int H, int W, int C, int Ho, int Wo,
                       void* workspace, unsigned char* out_u8, const float* mean,
                       const float* stdv, const float* uifm_bt, const float* uifm_binf,
                       const float* dist, float depth, const unsigned char* ops,
                       const float* turb, int allow_transpose, float* out_f32,
                       hipStream_t stream);
int mauv_stage_f32_aug(const float* x, int B, int C, int H, int W, const float* beta,
                       const float* binf, const float* dist, float depth,
                       const unsigned char* ops, const float* turb, int allow_transpose,
                       float* out, hipStream_t stream);

/* ---- evaluation metrics (metrics.hip) ----------------------------------------------------
 * train/multimodal.py:312-347 (confusion matrix) and Examples/"Example training with image
 * noise.py":530-634 (uncertainty-error AUROC, macro F1, 15-bin ECE / Emax), accumulated on the
 * device across an epoch instead of per-batch .cpu() copies:
 * mauv_confusion_update: counts[y * C + p] += 1 (int32 [C*C + 1]; out-of-range labels or
 *   predictions counted in counts[C*C]);
 * mauv_calibration_update: per MC-mean probability row, conf = max, pred = argmax (first
 *   maximum); the bin b with edges[b] < conf <= edges[b+1] (float64 edges, nbins + 1 of them)
 *   gets bins[3b] += 1, bins[3b+1] += conf, bins[3b+2] += (pred == label);
 * mauv_auroc_pairs: count2 += sum over (positive i, negative j) of 2 [s_i > s_j] + [s_i == s_j]
 *   (AUROC = count2 / (2 n_pos n_neg)). */
int mauv_confusion_update(const long long* labels, const long long* pred, int n, int C,
                          int* counts, hipStream_t stream);
int mauv_calibration_update(const float* probs, const long long* labels, int n, int C,
                            int nbins, const double* edges, double* bins, hipStream_t stream);
int mauv_auroc_pairs(const float* score, const unsigned char* positive, int n,
                     unsigned long long* count2, hipStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MAUV_H */
