// Host-side launch API of the fluxmpi_amd native library (no ATen dependency:
// raw device pointers + a hipStream_t, so callers can launch on any PyTorch
// stream, inside or outside HIP-graph capture).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include <vector>

namespace fluxmpi {

// ---- multi-tensor copy / cast / scale (pack, unpack, scale) -----------------
// dst[i][k] = (Tout)(src[i][k] * scale) for k < numel[i]. src[i] may equal dst[i]
// (in-place scale / cast is not allowed when the element sizes differ). The product is formed in
// fp64 with the caller's double when the source or the destination is fp64, else in fp32 with the
// scale rounded once to fp32; it is then rounded once to Tout.
void mt_copy(const std::vector<uintptr_t>& src, const std::vector<uintptr_t>& dst,
             const std::vector<int64_t>& numel, int in_dtype, int out_dtype, double scale,
             hipStream_t stream);

// Fill every tensor with `value` (zeroing flat grad buckets): fp64 leaves take the double, the
// others the value rounded once to fp32 and then to the leaf's dtype.
void mt_fill(const std::vector<uintptr_t>& dst, const std::vector<int64_t>& numel, int dtype,
             double value, hipStream_t stream);

// Sum of squares of all tensors into out[0] (fp32, atomically accumulated; out must be
// zeroed by the caller). Used by ClipNorm and by debug checksums.
void mt_sumsq(const std::vector<uintptr_t>& src, const std::vector<int64_t>& numel, int dtype,
              float* out, hipStream_t stream);

// ---- fused optimisers ---------------------------------------------------------
// Stochastic rounding of the bf16 stores of an update (optim_sr.h): given to mt_adam / mt_sgd /
// mt_rule as a trailing pointer (null: round to nearest, the kernels without it). Only the
// (bf16, bf16, bf16, no master) and (bf16, bf16, fp32, no master) layouts take it; LARS / LAMB do not.
struct SrHyper {
  uint64_t seed;                      // the Philox key
  uint32_t stream;                    // caller-chosen id below 2^30 (the engine: the bucket index)
  uint32_t step;                      // host step, read when dev_step is null
  const uint32_t* dev_step;           // optional device block {uint32 step, 7 unused} (sr_advance)
  const int64_t* offsets = nullptr;   // per leaf of the call: its first element's index in the stream; null: 0
  size_t n_offsets = 0;
};

struct AdamHyper {
  // doubles, as RuleHyper's: fp64 leaves compute with the caller's values; the fp32 kernels round
  // them once, to what the caller's fp32 value was
  double lr, beta1, beta2, eps;
  double bc1, bc2;     // 1 - beta1^t, 1 - beta2^t (host mode)
  double weight_decay;  // Optimisers.jl WeightDecay after Adam (AdamW = chain)
  float grad_scale;    // multiplies the incoming gradient (e.g. 1/world for mean)
  const float* dev;    // optional device hyper block {lr, beta1^t, beta2^t} (graph mode)
  const float* dev_gscale;  // optional device gradient scale (e.g. 1/loss_scale, the global-norm clip)
  const void* tscale = nullptr;  // optional device scale per leaf of the call (ClipNorm), fp32 (fp64 params: fp64)
  float clip_delta = 0.f;        // ClipGrad: clamp the scaled gradient to [-delta, delta]; 0: off
  // optional device int32 (loss scaling's non-finite flag): when *dev_skip != 0 every workgroup
  // returns before its first load of tensor data and nothing is stored; null: no predicate
  const int32_t* dev_skip = nullptr;
};

// master: optional fp32 master weights (mixed precision); when given, param is
// the low-precision copy that is re-written from the master after the update.
void mt_adam(const std::vector<uintptr_t>& param, const std::vector<uintptr_t>& grad,
             const std::vector<uintptr_t>& m, const std::vector<uintptr_t>& v,
             const std::vector<uintptr_t>& master, const std::vector<int64_t>& numel,
             int p_dtype, int g_dtype, int s_dtype, const AdamHyper& h, hipStream_t stream,
             const SrHyper* sr = nullptr);

// dev[1] *= beta1, dev[2] *= beta2 (advance the bias-correction powers on device); not when
// dev_skip is given and *dev_skip != 0 (a skipped step does not count).
void adam_advance(float* dev, float beta1, float beta2, hipStream_t stream, const int32_t* dev_skip = nullptr);

struct SgdHyper {
  double lr, momentum, weight_decay;  // doubles: as in AdamHyper
  float grad_scale;
  int nesterov;  // 0: heavy ball (Optimisers.Momentum), 1: Optimisers.Nesterov
  const float* dev_lr;
  const float* dev_gscale = nullptr;  // as in AdamHyper
  const void* tscale = nullptr;
  float clip_delta = 0.f;
  const int32_t* dev_skip = nullptr;  // as in AdamHyper
};
// buf: momentum buffers (ignored when momentum == 0 -> Optimisers.Descent).
void mt_sgd(const std::vector<uintptr_t>& param, const std::vector<uintptr_t>& grad,
            const std::vector<uintptr_t>& buf, const std::vector<uintptr_t>& master,
            const std::vector<int64_t>& numel, int p_dtype, int g_dtype, int s_dtype,
            const SgdHyper& h, hipStream_t stream, const SrHyper* sr = nullptr);

// The rest of the rule set (optim_rules.hip), one generic kernel with a per-element functor.
// kLars / kLamb: the layer-wise rules (optim_layerwise.hip), two phases (norm partials, then the
// update scaled by the leaf's trust ratio) behind the same entry.
enum RuleKind : int { kRmsProp = 0, kAdaGrad = 1, kLion = 2, kAdaMax = 3, kAmsGrad = 4, kNAdam = 5,
                      kAdaBelief = 6, kAdaDelta = 7, kLars = 8, kLamb = 9 };
struct RuleHyper {
  int kind;                  // RuleKind
  // doubles: fp64 leaves compute with the caller's values (1 - beta2 of a float 0.999 is off by
  // 1e-5); the fp32 kernels round them once, to what the caller's fp32 value was
  double lr, beta1, beta2, eps;  // beta1 is rho for RMSProp / AdaDelta / LARS; beta2 is LARS' trust coefficient
  double bt1, bt2;           // beta1^t, beta2^t (host mode; AdaMax, NAdam, AdaBelief)
  double weight_decay;       // WeightDecay after the rule: dx += wd * x (LARS / LAMB: the rule's own decay)
  float grad_scale;
  const float* dev;          // optional device block {lr, beta1^t, beta2^t}; {lr} for rules without beta^t
  const float* dev_gscale;   // as in AdamHyper
  const void* tscale;        // LARS / LAMB: written, the trust ratio of each leaf of the call (no input scale)
  float clip_delta;          // LARS / LAMB: must be 0
  // as in AdamHyper; a skipped LARS / LAMB step also leaves the moments, the partials and the ratio
  // table as the previous step wrote them
  const int32_t* dev_skip = nullptr;
};
// s1 / s2 / s3: the rule's state tensors in its Optimisers.jl order (as many lists as the rule
// keeps states: 1 RMSProp, AdaGrad, Lion; 2 AdaMax, NAdam, AdaBelief, AdaDelta; 3 AMSGrad; the
// others empty). master as in mt_adam. adam_advance advances a device block with beta^t entries.
// LARS (s1: velocity) and LAMB (s1, s2: m, v; device block as Adam's) take in s3 each leaf's address
// in a workspace of 2 * sumsq_partials(numel) entries of fp32 (fp64 leaves: fp64), no zero fill.
void mt_rule(const std::vector<uintptr_t>& param, const std::vector<uintptr_t>& grad,
             const std::vector<uintptr_t>& s1, const std::vector<uintptr_t>& s2,
             const std::vector<uintptr_t>& s3, const std::vector<uintptr_t>& master,
             const std::vector<int64_t>& numel, int p_dtype, int g_dtype, int s_dtype, const RuleHyper& h,
             hipStream_t stream, const SrHyper* sr = nullptr);

// ---- stochastic rounding (optim_sr.hip) ------------------------------------------------
// dst[i] (bf16) = sr(src[i] (fp32), bits of element offsets[leaf] + i of slot 0 of the stream): the
// update kernels' rounding as a stand-alone multi-tensor cast in their job layout. dev_skip (or
// null): non-zero calls the launch off before it loads tensor data.
void mt_stochastic_round(const std::vector<uintptr_t>& dst, const std::vector<uintptr_t>& src,
                         const std::vector<int64_t>& numel, const SrHyper& sr, const int32_t* dev_skip,
                         hipStream_t stream);
// The step block, 8 words: {uint32 step, 7 unused}. One thread: step += 1, unless *dev_skip != 0.
void sr_advance(void* block, const int32_t* dev_skip, hipStream_t stream);

// ---- gradient clipping: deterministic multi-tensor sum of squares ------------------
// Two launches per group of leaves, no float atomics (bit-identical from run to run):
// sumsq[i] = sum(grad[i]^2) and, when scale != nullptr,
// scale[i] = min(1, omega / (grad_scale * sqrt(sumsq[i]))) with torch.clamp's edge values
// (norm 0 -> 1, NaN -> NaN, inf -> 0). sumsq / scale / partials hold fp32 (fp64 gradients:
// fp64); partials needs sumsq_partials(numel) entries. A leaf without elements gets 0 / 1.
// nonfinite_flag: the same pass also runs mt_check_finite's test on every element it reads (the
// sums are the bits of the call without it). dev_pre: a device scalar multiplied into the norm
// (loss scaling's inverse scale: the scales then refer to the unscaled gradient); sumsq stays raw.
int64_t sumsq_partials(const std::vector<int64_t>& numel);
void mt_leaf_sumsq(const std::vector<uintptr_t>& grad, const std::vector<int64_t>& numel, int g_dtype,
                   void* partials, void* sumsq, void* scale, float omega, float grad_scale, hipStream_t stream,
                   int32_t* nonfinite_flag = nullptr, const float* dev_pre = nullptr);
// slot[0] = (accumulate ? slot[0] : 0) + sum_i sumsq[i] (fixed order); slot[1] = grad_scale *
// [*dev_pre *] sqrt(slot[0]) (the global gradient norm); slot[2] = [*dev_pre *] (omega > 0 ?
// min(1, omega / slot[1]) : 1): the one dev_gscale of an update behind a loss scale and a global clip.
void clip_total(const void* sumsq, int64_t n, int acc_dtype, float* slot, int accumulate, float omega,
                float grad_scale, hipStream_t stream, const float* dev_pre = nullptr);

// ---- loss scaling: exact non-finite check, scaler update -------------------------------
// flag[0] = 1 if any element of any gradient is inf or NaN (exponent field all ones: per element,
// so a finite value whose square overflows does not count); left alone otherwise. One int32,
// sticky: the checks of a step's buckets and dtypes accumulate into it and loss_scale_update
// clears it. The update kernels' job layout (one workgroup per 4096-element chunk); a workgroup
// that found one stores the 1 from one lane after a block-wide OR: no atomics, no zero fill.
void mt_check_finite(const std::vector<uintptr_t>& grad, const std::vector<int64_t>& numel, int g_dtype,
                     int32_t* flag, hipStream_t stream);
// The scaler's device block, 8 words: {float scale, float 1/scale, int32 growth tracker, int32 steps
// skipped so far, int32 last step skipped, int32 non-finite flag, 2 unused}. One thread applies
// GradScaler's rule: flag set -> scale *= backoff, tracker = 0, skipped += 1; clear -> tracker += 1
// and at tracker == interval scale *= growth, tracker = 0. Then scale is clamped to [min_scale,
// max_scale], its inverse stored, the flag copied to "last step skipped" and cleared.
void loss_scale_update(void* block, float growth, float backoff, int interval, float min_scale, float max_scale,
                       hipStream_t stream);

// ---- exponential moving average of the weights (optim_ema.hip) -------------------------
// ema[i] <- ema[i] + omd * (src[i] - ema[i]) per element, in this form (src == ema keeps the bits), in
// the update kernels' job layout. src: the fp32 master of a leaf, or its parameter (src_dtype: fp32,
// bf16, fp16, fp64); ema: fp32 (fp64 sources: fp64). dev_block (the block below, or null) overrides
// omd with its first word and calls the launch off while its `hold` word is set; dev_skip (or null)
// calls it off as it does the update kernels. A launch that is called off loads no tensor data.
void mt_ema(const std::vector<uintptr_t>& ema, const std::vector<uintptr_t>& src, const std::vector<int64_t>& numel,
            int src_dtype, double omd, const int32_t* dev_block, const int32_t* dev_skip, hipStream_t stream);
// The EMA device block, 8 words: {float omd = 1 - d_t, float d_t, int32 n (EMA updates done), int32 k
// (optimiser steps since the last EMA update), int32 hold (the coming step is not an EMA step), 3
// unused}. One thread, after a step's mt_ema launches; nothing changes when *dev_skip != 0. The step
// was an EMA step (hold == 0): n += 1, k = 0; else k += 1. Then hold = (k + 1 < every), d_t = warmup ?
// min(decay, (1 + n) / (10 + n)) : decay, omd = 1 - d_t.
void ema_advance(void* block, float decay, int warmup, int every, const int32_t* dev_skip, hipStream_t stream);

// ---- device input pipeline (augment.hip): crop, flip, normalise, mixup / cutmix in one pass ----
// out [B][h][w][C] (bf16 / fp16, C in {3, 4}, channel 3 = +0, 16-byte-aligned base) from the dense
// u8 batch in [B][H][W][3] (any byte alignment). Sample b draws one Philox4x32-10 call, key (seed lo,
// seed hi), counter (s lo, s hi, stream, step), s = sample_offset + b: ox = (w0 * rx) >> 32, oy =
// (w1 * ry) >> 32, flip = w2 & 1, rx = W + 2 pad - w + 1, ry likewise (crop_center: ox = (rx - 1) / 2,
// oy = (ry - 1) / 2, no draw; flip == 0: never flipped). Output pixel (i, j) reads source row
// i + oy - pad, column (flip ? w - 1 - j : j) + ox - pad; outside the image the byte is `fill`.
// y = float(u) * a[c] + b[c], the product and the sum rounded separately. The partner of sample b is
// B - 1 - b, its pixel its own crop and flip at the same (i, j): mode 0 z = y; mode 1 (mixup)
// z = y_p + lam * (y - y_p), each operation rounded; mode 2 (cutmix) z = y_p for y0 <= i < y1,
// x0 <= j < x1, else y. The store is the round-to-nearest cast of z.
struct AugHyper {
  uint64_t seed;           // the Philox key
  uint32_t stream;         // caller-chosen id below 2^30
  uint32_t step;           // read when dev_block is null
  int64_t sample_offset;   // index of sample 0 of this batch in the random stream (>= 0)
  int mode;                // 0 none, 1 mixup, 2 cutmix (dev_block null)
  int y0, x0, y1, x1;      // the cutmix box in the output (dev_block null)
  float lam;               // mixup weight of the sample itself (dev_block null)
  int pad, fill;           // zero-extension of the image on every side; the byte it is made of
  int crop_center, flip;   // centre crop (no draw); flips enabled
  float a[3], b[3];        // fp32(1 / (255 std_c)), fp32(-mean_c / std_c)
  // optional device block, 8 words {step, mode, y0, x0, y1, x1, lam bits, 0} (aug_block_set): read
  // wave-uniformly in place of those six, so that a captured launch follows the block
  const uint32_t* dev_block = nullptr;
};
void augment_batch(const void* in, void* out, int64_t B, int H, int W, int h, int w, int C, int dtype,
                   const AugHyper& a, hipStream_t stream);
// One thread fills the block with plain stores.
void aug_block_set(void* block, uint32_t step, int mode, int y0, int x0, int y1, int x1, float lam,
                   hipStream_t stream);

// ---- device input pipeline, resampling form (resize_crop.hip): per-sample box -> bilinear resize ----
// As augment_batch, with the crop given per sample: boxes int32 [B][5] = (top, left, bh, bw, flip) on
// the device, a box inside the image (it is clamped to it before use: top into [0, H - 1], bh into
// [1, H - top], columns likewise, flip & 1). Sides H, W, h, w <= 16384. Output column j, j' = w - 1 - j
// under a flip: num = (2 j' + 1) bw - w, den = 2 w; num < 0: x0 = 0, fx = 0; else x0 = num / den, fx =
// ((num % den) * 2048 + w) / den; x1 = min(x0 + 1, bw - 1). Rows likewise with (i, bh, h), no flip.
// Per channel, from the four bytes at rows top + y0 / y1, columns left + x0 / x1: t0 = p00 (2048 - fx)
// + p01 fx, t1 likewise, v = (t0 (2048 - fy) + t1 fy + 2^21) >> 22 (half-pixel centres, no antialias,
// 11-bit weights). From the byte v on: augment_batch's arithmetic, the partner B - 1 - b with its own
// box. Of AugHyper the mixing fields, a, b and dev_block apply; pad and fill must be 0.
void resized_crop_batch(const void* in, void* out, const int32_t* boxes, int64_t B, int H, int W, int h, int w, int C,
                        int dtype, const AugHyper& a, hipStream_t stream);

// ---- BatchNorm (NHWC, channels innermost) + ReLU / residual-add fusions ----------
// Training forward: per-channel batch statistics over rows = N*H*W, then
//   y = act(x * scale_c + shift_c [+ residual]).
// Writes mean/invstd (fp32 [C]) for the backward and updates running stats.
void bn_fwd_train(const void* x, void* y, const void* residual, const float* weight,
                  const float* bias, float* running_mean, float* running_var, float* save_mean,
                  float* save_invstd, float* workspace, int64_t rows, int64_t C, float momentum,
                  float eps, int relu, uint8_t* relu_mask, int dtype, hipStream_t stream, int64_t* num_batches_tracked = nullptr);
// Backward: given dy (and y when relu, to mask), computes dx, dweight, dbias and
// (when residual was fused) d_residual = masked dy.
// y == nullptr with relu: the ReLU mask is recomputed from x (bit-identical to forward).
// relu_mask (optional): the 1-bit-per-element mask written by bn_fwd_train.
// dx == nullptr: reduce and finalize only. dweight / dbias (the finished sums of dy_eff * xhat and of
// dy_eff) are written and no pass forms dx; the consumer forms it itself from them (gemm_bf16 mode 4).
// dres must then be null too (it is written by the dx pass): the combination is an error.
void bn_bwd(const void* dy, const void* x, const void* y, const uint8_t* relu_mask, const float* weight,
            const float* bias,
            const float* save_mean, const float* save_invstd, void* dx, void* dres,
            float* dweight, float* dbias, float* workspace, int64_t rows, int64_t C, int relu,
            int dtype, hipStream_t stream, int stats_ready = 0);
size_t bn_workspace_floats(int64_t rows, int64_t C);
// Split forward for producer/consumer fusion with the GEMM:
// bn_stats_finalize: [stats pass over x unless stats_ready (a GEMM epilogue already
// accumulated them into ws)] + finalize (mean/invstd, running stats, and optionally the
// per-channel scale/shift a consumer GEMM applies on load). bn_apply: the normalise pass.
void bn_stats_finalize(const void* x, const float* w, const float* b, float* running_mean,
                       float* running_var, float* save_mean, float* save_invstd, float* scale,
                       float* shift, float* workspace, int64_t rows, int64_t C, float momentum,
                       float eps, int stats_ready, int dtype, hipStream_t stream, int64_t* num_batches_tracked = nullptr);
void bn_apply(const void* x, void* y, const void* residual, const float* w, const float* b,
              const float* save_mean, const float* save_invstd, int64_t rows, int64_t C, int relu,
              uint8_t* relu_mask, int dtype, hipStream_t stream);
// Synchronised (cross-rank) BatchNorm on the same kernels, stopped at the seams where a collective
// belongs, with deterministic reductions (per-workgroup partials in `part`, folded in a fixed order:
// no float atomics, bit-identical run to run). `part`: bn_sync_workspace_floats(rows, C) floats, no
// zero fill needed. rows >= 1 (an empty shard sends a zero message and launches nothing).
//   bn_sync_stats: msg[2C + 2] = (sum x [C], sum x^2 [C], n_hi, n_lo), rows = 4096 n_hi + n_lo.
//     With save_mean != nullptr the finalize from the LOCAL sums runs in the same launch (world size 1).
//   bn_sync_finalize_fwd: mean / invstd / running statistics / num_batches_tracked from a (summed)
//     message; the count is read on the device. Follow with bn_apply.
//   bn_sync_bwd_reduce: msg[2C] = (sum g [C], sum g xhat [C]) of this shard, also written to dbias / dweight.
//   bn_sync_bwd_dx: dx (and dres) from a (summed) backward message. count = the (n_hi, n_lo) pair of the
//     summed forward message and coef = 2C floats of scratch; count == nullptr: msg holds the sums of
//     these `rows` rows alone (world size 1).
size_t bn_sync_workspace_floats(int64_t rows, int64_t C);
void bn_sync_stats(const void* x, float* part, float* msg, int64_t rows, int64_t C, int dtype, hipStream_t stream,
                   float* save_mean = nullptr, float* save_invstd = nullptr, float* running_mean = nullptr,
                   float* running_var = nullptr, float momentum = 0.f, float eps = 0.f,
                   int64_t* num_batches_tracked = nullptr);
void bn_sync_finalize_fwd(const float* msg, float* running_mean, float* running_var, float* save_mean,
                          float* save_invstd, int64_t C, float momentum, float eps, hipStream_t stream,
                          int64_t* num_batches_tracked = nullptr);
void bn_sync_bwd_reduce(const void* dy, const void* x, const void* y, const uint8_t* relu_mask, const float* weight,
                        const float* bias, const float* save_mean, const float* save_invstd, float* part, float* msg,
                        float* dweight, float* dbias, int64_t rows, int64_t C, int relu, int dtype,
                        hipStream_t stream);
void bn_sync_bwd_dx(const void* dy, const void* x, const void* y, const uint8_t* relu_mask, const float* weight,
                    const float* bias, const float* save_mean, const float* save_invstd, const float* msg,
                    const float* count, float* coef, void* dx, void* dres, int64_t rows, int64_t C, int relu,
                    int dtype, hipStream_t stream);
// Dual BatchNorm of a downsample block: y = relu(BN(x) + BN2(x2)) (+ 1-bit ReLU mask), and its
// backward: dx, dx2 and both BatchNorms' dweight/dbias from one reduce + one dx pass over
// (dy, mask, x, x2). ws/ws2: two zeroed statistics workspaces. C/8 must divide 256.
// bn_bwd_dual with dx == dx2 == null stops after the reduce and the finalize (the four finished sums
// in dweight / dbias / dweight2 / dbias2), as bn_bwd does for a null dx; exactly one null is an error.
void bn_apply_dual(const void* x, const void* x2, void* y, const float* w, const float* b, const float* save_mean,
                   const float* save_invstd, const float* w2, const float* b2, const float* save_mean2,
                   const float* save_invstd2, int64_t rows, int64_t C, uint8_t* relu_mask, int dtype,
                   hipStream_t stream);
void bn_bwd_dual(const void* dy, const uint8_t* relu_mask, const void* x, const void* x2, const float* w,
                 const float* save_mean, const float* save_invstd, const float* w2, const float* save_mean2,
                 const float* save_invstd2, void* dx, void* dx2, float* dweight, float* dbias, float* dweight2,
                 float* dbias2, float* ws, float* ws2, int64_t rows, int64_t C, int dtype, hipStream_t stream);
// Inference: y = act(x * scale + shift [+ residual]) from running statistics.
void bn_fwd_infer(const void* x, void* y, const void* residual, const float* weight,
                  const float* bias, const float* running_mean, const float* running_var,
                  int64_t rows, int64_t C, float eps, int relu, int dtype, hipStream_t stream);

// ---- fused stem: BN affine + ReLU + max-pool (NHWC) ---------------------------------
// y = relu(max over KxK/S window (pad P) of x*scale+shift), idx = window index (0xFF: max <= 0)
void bn_relu_maxpool_fwd(const void* x, const float* scale, const float* shift, void* y, uint8_t* idx, int64_t N,
                         int64_t H, int64_t W, int64_t C, int K, int S, int P, int dtype, hipStream_t stream);
// y[p][0..3] = (x[p][0], x[p][1], x[p][2], 0) for npix 16-bit NHWC pixels (stem channel pad)
void pad_c3_to_c4(const void* x, void* y, int64_t npix, int dtype, hipStream_t stream);

// ---- ResNet stem on MFMA (stem.hip): 7x7/2 conv of NHWC4 224x224 images + BN statistics;
// the fused backward (pool gather + BN backward + filter gradient)
// (stem_fwd's max_blocks caps the persistent grid, 0 = the resident workgroups: fewer workgroups walk more
// row groups each, which is how the tests run the double-buffered halo loop at small batches)
void stem_fwd(const void* x, const void* wp, void* y, float* stats, int64_t n, hipStream_t stream,
              int max_blocks = 0);
int stem_bwd_blocks(int64_t n);
int64_t stem_part_floats();
void stem_bwd(const void* x, const void* c, const void* dp, const uint8_t* idx, const float* w, const float* mean,
              const float* inv, float* part, int blocks, float* stats, float* dw_bn, float* db_bn, float* dwp,
              int64_t n, hipStream_t stream);
// Softmax attention, head dim 64, bf16 (csrc/kernels/attention.hip). q/k/v and dq/dk/dv share
// strides (sq_b, sq_t; head stride 64), o has (so_b, so_t, so_h), dout (sg_b, sg_t; head stride
// 64); stats is fp32 [B][H][T][2]: attn_fwd writes [..][0] = base-2 log-sum-exp of the scaled
// scores, attn_bwd reads it and writes [..][1] = rowsum(dO*O).
void attn_fwd(const void* q, const void* k, const void* v, void* o, float* stats, int64_t sq_b, int64_t sq_t,
              int64_t so_b, int64_t so_t, int64_t so_h, int B, int T, int H, int Dh, float scale, hipStream_t stream);
void attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* dout, void* dq, void* dk,
              void* dv, float* stats, int64_t sq_b, int64_t sq_t, int64_t so_b, int64_t so_t, int64_t so_h,
              int64_t sg_b, int64_t sg_t, int B, int T, int H, int Dh, float scale, hipStream_t stream,
              float* colpart = nullptr);
// rows of attn_bwd's optional column-sum partials ([rows][3*H*64] fp32: per-wave sums of the dQ /
// dK / dV rows it writes; their reduce is the packed QKV bias gradient), 0 if this call's variant
// does not write them
int attn_bwd_colpart_rows(int B, int T, int H, int64_t sq_t, int64_t sg_t);
// the kernels attn_fwd / attn_bwd launch for this shape in this process (the FLUXMPI_ATTN_*
// switches are read once): their names ("a+b" for a two-kernel backward) and the workgroups per
// (batch, head); the launchers take their choice from the same function
struct AttnDispatch {
  const char* fwd;
  const char* bwd;
  int fwd_parts, bwd_parts;
};
AttnDispatch attn_dispatch(int B, int T, int H);
// dx[n,h,w,c] = sum of dy over the windows whose idx points at (h,w) (gather; dx fully written)
void maxpool_bwd(const void* dy, const uint8_t* idx, void* dx, int64_t N, int64_t H, int64_t W, int64_t C, int K,
                 int S, int P, int dtype, hipStream_t stream);

// ---- fused LayerNorm (+ residual add), rows of D (D % 8 == 0, D <= 8192) ----------------
// forward: [h = x + residual] (h written when residual != nullptr); y = LN(h) * w + b;
// mean / rstd per row (fp32) saved. w/b: fp32 or the activation dtype (wdtype), 16-byte aligned.
void layernorm_fwd(const void* x, const void* residual, void* h, void* y, const void* w, const void* b, float* mean,
                   float* rstd, int64_t rows, int64_t D, float eps, int dtype, int wdtype, hipStream_t stream);
// backward: dx = LN backward of dy [+ dh_ext]; per-workgroup [2][D] fp32 partials of (dw, db)
// stored into `partials` (capacity max_blocks x 2D); returns the number of partial rows written
// (sum them with gemm_splitk_reduce). colsum (dh_ext required): [3][D] rows, the third the
// column sums of dx.
int layernorm_bwd(const void* dy, const void* x, const void* dh_ext, const float* mean, const float* rstd,
                  const void* w, void* dx, float* partials, int max_blocks, int64_t rows, int64_t D, int dtype,
                  int wdtype, hipStream_t stream, bool colsum);

// ---- MFMA bf16 GEMM with BatchNorm fusions (1x1 convolutions) --------------------
// C[M,N] = A[M,K] * B[N,K]^T. a_kmajor: A stored [M][lda] (K contiguous), else [K][lda]
// (M contiguous); b_kmajor likewise for B. mode 0: C bf16; mode 1: C bf16 + per-column
// sum/sumsq into stats[64][2][N] (sharded, caller-zeroed); mode 2: C fp32 += (atomics,
// allows split-K over `splits`); mode 3: split s stores its fp32 partial to C + s*M*ldc. a_scale/a_shift: relu(A*s+t) per k applied on load
// (K-major A); b_scale/b_shift: per n on load (N-major B).
struct GemmProblem {
  const void* a;
  const void* b;
  void* c;
  int64_t lda, ldb, ldc, M, N, K;
  bool a_kmajor, b_kmajor;
  int mode, splits;
  const float* a_scale;
  const float* a_shift;
  const float* b_scale;
  const float* b_shift;
  float* stats;
  int tile_m, tile_n;  // 0 = auto, 64 forces the 64 tile
  int nbuf;            // LDS buffers: 0 = auto (2), 1, 2
  const void* res;     // optional bf16 residual [M][ldr] added in the epilogue (modes 0/1)
  int64_t ldr;
  // mode 1 + bnb_x: stats = BatchNorm-backward reductions (sum dy_eff, sum dy_eff*xhat) of a BN
  // whose input is bnb_x ([M][N] dense) and whose output gradient is C (see gemm.hip)
  const void* bnb_x;
  const float* bnb_w;
  const float* bnb_b;
  const float* bnb_mean;
  const float* bnb_inv;
  const uint8_t* bnb_mask;
  int bnb_rm;
  // conv_h > 0: A is implicit — the 3x3 / stride 1 / pad 1 im2col of an NHWC image batch
  // [M/(H*W)][H][W][conv_c] (K = 9*conv_c, K-major B = [N][3][3][conv_c] filter)
  int conv_h = 0, conv_w = 0, conv_c = 0;
  int engine = 0;  // 0 auto, 1 register-staged kernel (gemm.hip), 2 LDS-DMA pipelined kernel (gemm_glds.hip)
  // LDS-DMA kernel: residual element (m, n) counts only if bit n%8 of res_mask[(m*N + n)/8] is set
  // (the 1-bit ReLU mask of the BatchNorm whose output gradient the residual is)
  const uint8_t* res_mask = nullptr;
  // LDS-DMA kernel: res_sub_h > 0 — the residual is the compact stride-2 subsample of an
  // [M/(H*W)][H][W] row grid (H = res_sub_h, W = res_sub_w): output row (n, h, w) adds residual row
  // (n, h/2, w/2) when h and w are even and nothing otherwise (a stride-2 1x1 convolution's input
  // gradient, without the zero-filled full-resolution tensor). No res_mask with it.
  int res_sub_h = 0, res_sub_w = 0;
  // LDS-DMA kernel: a_sub_h > 0 — A row (n, ho, wo) of an [M/(Ho*Wo)][Ho][Wo] output grid is row
  // (n, 2*ho, 2*wo) of the NHWC image [M/(Ho*Wo)][a_sub_h][a_sub_w][lda] (Ho = ceil(H/2)): a
  // stride-2 1x1 convolution without the strided copy of its input. Plain K-major A only.
  int a_sub_h = 0, a_sub_w = 0;
  // LDS-DMA kernel, implicit conv: conv_s == 2 — a 3x3 / stride 2 / pad 1 convolution over the
  // NHWC image [M/(Ho*Wo)][conv_h][conv_w][conv_c] (conv_h / conv_w the INPUT size, Ho = ceil(H/2));
  // conv_s == 16 + (2 py + px) — parity class (py, px) of that convolution's INPUT gradient: A = dY
  // [M/(Ho*Wo)][conv_h = Ho][conv_w = Wo][conv_c = Cout], B = the flipped transposed filter
  // [N = Cin][3][3][Cout] (ldb >= 9 Cout), K = taps * Cout (1, 2, 2, 4 taps), C row (img, a, b) =
  // dX pixel (img, 2a + py, 2b + px) of [.][2 Ho][2 Wo] (even input sizes)
  int conv_s = 1;
};
void gemm_bf16(const GemmProblem& g, hipStream_t stream);
// mode 4 (conv3bn3_bwd.hip): the one-pass backward of conv3 (1x1, 64 -> 256) -> bn3 (+ residual,
// ReLU) of a stage-1 identity block. dx3, bn3's input gradient, is formed in registers (the dx
// pass's arithmetic, bit for bit) and never stored; c = d_a2 [M][64] = dx3 . W and the filter
// gradient's fp32 partials stats[s][256][64], s < splits, of dx3^T . a2 (sum them with
// gemm_splitk_reduce). Fields: M = pixels, N = 64, K = 256; a = dy [M][256] (K-major, lda = 256);
// bnb_x = x3 [M][256]; bnb_mask = the 1-bit ReLU mask (bnb_rm = 3); bnb_w / bnb_mean / bnb_inv =
// bn3's weight (nullable) / saved mean / saved invstd; a_scale = sum dy_eff, a_shift = sum dy_eff
// xhat ([256] fp32, bn_bwd's dbias / dweight); b = W [256][64] as stored (N-major, ldb = 64);
// res = a2 [M][64] (ldr = 64); ldc = 64. splits = the slab count = the workgroups launched, the
// caller's choice: min(ceil(M / 64), 2 x compute units) fills the device with one round.
// The same with N = 128, K = 512 (a stage-2 identity block's 128 -> 512; every 64 / 256 above doubled)
// runs conv3bn3_s2_bwd.hip: one workgroup per compute unit, so splits = min(ceil(M / 32), compute units).
// Any other (N, K) throws.
void conv3bn3_bwd(const GemmProblem& g, hipStream_t stream);
// conv3ds_bwd.hip: the same around the dual BatchNorm of a stage-1 downsample block,
// out = relu(bn3(conv3(a2)) + bn_ds(conv_ds(x))), both convolutions 1x1, 64 -> 256, stride 1. One pass
// over (dy [P][256], the 1-bit ReLU mask, c3, c_ds [P][256], a2, x [P][64]) forms dx3 and dx_ds in
// registers (bit for bit what bn_bwd_dual's dx pass stores from the same finished sums) and writes
// d_a2 = dx3 . W3, d_xside = dx_ds . W_ds ([P][64] bf16) and the fp32 partials ws3 / wsds
// [slabs][256][64] of dx3^T . a2 / dx_ds^T . x (sum each with gemm_splitk_reduce). w / w2: the
// BatchNorm weights (nullable: 1); sum_dy* / sum_dy_xhat*: [256] fp32, bn_bwd_dual's dbias* / dweight*
// (call it with dx = dx2 = null). wt3 / wtds: the filters [256][64] as stored. Every pointer 16-byte
// aligned. slabs = the workgroups launched, the caller's choice: min(ceil(P / 32), compute units)
// fills the device with one round (one workgroup of 512 lanes and 112 KiB of LDS per compute unit).
void conv3ds_bwd(const void* dy, const uint8_t* relu_mask, const void* c3, const void* cds, const float* w,
                 const float* save_mean, const float* save_invstd, const float* sum_dy, const float* sum_dy_xhat,
                 const float* w2, const float* save_mean2, const float* save_invstd2, const float* sum_dy2,
                 const float* sum_dy_xhat2, const void* a2, const void* x, const void* wt3, const void* wtds,
                 void* d_a2, void* d_xside, float* ws3, float* wsds, int64_t P, int slabs, hipStream_t stream);
// bn_relu_conv1x1_fwd.hip: bn2 apply + ReLU + the 1x1 expansion convolution of a bottleneck in one
// streaming kernel, (Cin, Cout) = (64, 256) or (128, 512), bf16 NHWC. Reads c2 [P][Cin] once, writes
// a2 = relu(fmaf(c2, scale, shift)) [P][Cin] (bit for bit what bn_apply stores from the same
// statistics; scale / shift [Cin] fp32 as bn_stats_finalize produces them) and c3 = a2 . W^T
// [P][Cout] (wt = the filter [Cout][Cin] as stored), and adds the per-channel sum and sum of squares
// of the rounded c3 into stats [64][2][Cout] (one atomic per column, moment and workgroup). Every
// pointer 16-byte aligned; the grid is one resident round, at most one workgroup per 32-pixel tile.
bool bn_relu_conv1x1_fwd_supported(int Cin, int Cout);
void bn_relu_conv1x1_fwd(const void* c2, const float* scale, const float* shift, const void* wt, void* a2, void* c3,
                         float* stats, int64_t P, int Cin, int Cout, hipStream_t stream);
// the LDS-DMA pipelined kernel: K-major A (or implicit conv) and B, modes 0/1, optional residual,
// no prologue affine / split-K / BN-backward epilogue
bool gemm_glds_supported(const GemmProblem& g);
void gemm_glds(const GemmProblem& g, hipStream_t stream);
// weight gradient, fp32 split-K partials ws[s][M][N] = sum over split s of A[k][m] * B[k][n]
// (A: [K][lda], B: [K][ldb] or, conv_h > 0, the implicit 3x3/s1/p1 im2col of an NHWC image
// [K/(H*W)][H][W][conv_c] with N = 9*conv_c; b_sub: row k of B = pixel (n, 2ho, 2wo) of the NHWC image
// [.][conv_h][conv_w][ldb] for output pixel k = (n, ho, wo) of a stride-2 1x1 convolution, or with
// conv_c > 0 the implicit im2col of a 3x3 / stride 2 / pad 1 convolution over that grid);
// returns nothing, reduce with gemm_splitk_reduce. variant: 0/1 32-deep K-steps / 3 stages, 2 64-deep /
// 2 stages; bit 2: plain dispatch order; bit 3: two K-groups per 8-wave workgroup (gemm_glds.hip)
void gemm_wgrad(const void* a, const void* b, float* ws, int64_t lda, int64_t ldb, int64_t M, int64_t N, int64_t K,
                int splits, int conv_h, int conv_w, int conv_c, hipStream_t stream, int variant = 0, int b_sub = 0);
// out_i[ci][t][co] = in_i[co][taps-1-t][ci] (bf16) for every filter i, one launch per 40 filters:
// the K-major B operand of the input-gradient GEMMs (1x1: W^T; 3x3: transposed + flipped)
void transpose_filters(const std::vector<uintptr_t>& src, const std::vector<uintptr_t>& dst,
                       const std::vector<int>& co, const std::vector<int>& ci, const std::vector<int>& taps,
                       hipStream_t stream);
// out[e] = sum over s < splits of ws[s*n + e] (mode-3 split-K partials; ws is clobbered); out fp32 or bf16
void gemm_splitk_reduce(const float* ws, int splits, int64_t n, void* out, int out_dtype, hipStream_t stream);
// the same with the reduced row split into <= 3 segments of `seg` columns, each to its own output
// (e.g. a LayerNorm's dw / db straight into two DDP bucket slices)
void gemm_splitk_reduce_seg(const float* ws, int splits, int64_t n, int64_t seg, void* out0, void* out1, void* out2,
                            int out_dtype, hipStream_t stream);
// Weight gradient on 256 x 256 tiles (wgrad256.hip): ws[split][M][N] = sum over the split's k of
// A[k][m] * B[k][n] (bf16 A [K][lda], B [K][ldb], M and N multiples of 256), fp32 partials.
bool wgrad256_supported(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb);
int wgrad256_actual_splits(int64_t K, int splits);
void wgrad256_set_variant(int v);  // main-loop variant (A/B runs; 3 hoisted addressing, 4 ping-pong)
void gemm_wgrad256(const void* a, const void* b, float* ws, int64_t lda, int64_t ldb, int64_t M, int64_t N, int64_t K,
                   int splits, hipStream_t stream);
// Token-major Linear GEMM, both operands k-contiguous (gemm_nt.hip): C[M][N] = A[M][K] B[N][K]^T,
// 256 x 256 tiles, ping-pong 8-wave schedule; epi 0 (+ bias), 1 (+ bias: C = gelu'(h), C2 = gelu(h)),
// 2 (C = bf16(acc) * D, D = gelu'(h) as epi 1 stored it; colpart[2 * M / 256][N] = per-half-tile column sums of C),
// 3 (C, and its per-column sum / sum of squares added into the BatchNorm shards stats[64][2][N]).
bool gemm_nt_supported(int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc);
bool gemm_nt_conv_supported(int64_t pixels, int64_t C, int64_t Cout);
int gemm_nt_colpart_rows(int64_t M);
// split-K tail: the fewest k-tiles of a workgroup's share of the last round (0: off, the default;
// FLUXMPI_GEMM_NT_SPLIT overrides it). Test/diagnostic knob, not public API.
void gemm_nt_set_split(int min_ktiles);
int gemm_nt_get_split();
void gemm_nt(const void* a, const void* b, void* c, void* c2, const void* bias, int bias_f32, const void* h,
             float* colpart, float* stats, int64_t lda, int64_t ldb, int64_t ldc, int64_t M, int64_t N, int64_t K,
             int epi, hipStream_t stream);
// 3x3 / stride 1 / pad 1 convolution on the same kernel: A = the implicit im2col of the NHWC image
// x [nimg][H][W][C] (C % 64 == 0), B = w [Cout][3][3][C]; y [nimg*H*W][Cout]; epi 0, 3 (statistics)
// or 4 (y = bf16(bf16(conv) + residual), residual laid out as y)
void gemm_nt_conv(const void* x, const void* w, void* y, float* stats, int64_t nimg, int H, int W, int C,
                  int64_t Cout, int epi, hipStream_t stream, const void* residual = nullptr);
// A token-major Linear's input and weight gradients in one launch (linbwd.hip): dx [M][K] =
// dy [M][N] W [N][K] (bf16, nullptr: skip) and the weight gradient's fp32 split-K partials
// ws [s][N][K] of dy^T x (nullptr: skip; s = linear_bwd_splits(M, N, K, splits), sum them with
// gemm_splitk_reduce). M, N, K multiples of 256.
bool linear_bwd_supported(int64_t M, int64_t N, int64_t K, int64_t ldy, int64_t ldx, int64_t ldw, int64_t lddx);
int linear_bwd_splits(int64_t M, int64_t N, int64_t K, int splits);
void linear_bwd(const void* dy, const void* x, const void* w, void* dx, float* ws, int64_t M, int64_t N, int64_t K,
                int64_t ldy, int64_t ldx, int64_t ldw, int64_t lddx, int splits, int dg_first, hipStream_t stream);
// 3x3 / pad 1 / stride 1-2 convolution over a 3-channel NHWC bf16 image (conv_c3.hip), Cout % 128 == 0:
// forward y [pixels][Cout] from w_pairs [Cout][14] (the channels_last filter's 27 taps x channels as
// packed bf16 pairs, the 28th element 0); filter gradient as fp32 partials [blocks][Cout][27]
// (reduce with gemm_splitk_reduce into the [Cout][3][3][3] channels_last filter order)
bool conv_c3_supported(int64_t N, int H, int W, int stride, int Cout);
int64_t conv_c3_wgrad_blocks(int64_t N, int H, int W, int stride);
void conv_c3_fwd(const void* x, const void* w_pairs, void* y, int64_t N, int H, int W, int stride, int Cout,
                 hipStream_t stream);
void conv_c3_wgrad(const void* x, const void* dy, float* part, int64_t N, int H, int W, int stride, int Cout,
                   hipStream_t stream);
// Narrow-channel 3x3 / stride 1 / pad 1 convolution (conv3x3n.hip): C = Cout in {64, 128}, the
// input halo staged once per 256-pixel workgroup; x [pixels][C] NHWC, w [Cout][9][C], y [pixels][Cout];
// epi 0 or 3 (BatchNorm statistics into stats[64][2][Cout])
// resident workgroups of the 128-channel kernel on the current device (its tail split's round size)
int conv3x3n_slots128();
bool conv3x3n_supported(int64_t pixels, int C, int Cout, int H, int W);
void conv3x3n(const void* x, const void* w, void* y, float* stats, int64_t pixels, int H, int W, int C, int Cout,
              int epi, hipStream_t stream);
// Weight gradient of the narrow-channel 3x3 / stride 1 / pad 1 convolution (wgrad3x3n.hip): dy
// [N][H][W][Cout], x [N][H][W][C] (C in {64, 128}); ws[split][Cout][9 C] fp32 partials (reduce with
// gemm_splitk_reduce; the actual split count is wgrad3x3n_splits). variant bit 0: 8 waves (else 4),
// bit 1: two register sets of prefetched rows (4 waves), bit 2 (C = 128): 128 Cout per workgroup.
// A workgroup owns 64 / 128 Cout x all nine taps (C = 64) or x one filter row of three taps (C = 128).
bool wgrad3x3n_supported(int64_t N, int H, int W, int C, int Cout);
int wgrad3x3n_splits(int64_t N, int H, int splits);
int wgrad3x3n_groups(int C, int Cout, int variant);
void wgrad3x3n(const void* dy, const void* x, float* ws, int64_t N, int H, int W, int C, int Cout, int splits,
               int variant, hipStream_t stream);
// dst[c][r] = src[r][c], bf16 (rows, cols, leading dims multiples of 8)
void transpose_bf16(const void* src, void* dst, int64_t rows, int64_t cols, int64_t lds, int64_t ldd,
                    hipStream_t stream);

// ---- Anderson-acceleration solver (DEQ) --------------------------------------------
// X: fp32 history, F: fp32 or bf16 history, [bsz][m rows of row_stride][d] (batch_stride between batches).
// anderson_gram: partials[b][chunk][37]: the upper-triangle pair sums of G G^T (G = F - X over
// rows < n; pair (i, j>=i) at index i*n - i*(i-1)/2 + (j-i)) and |F[last]|^2 at [36];
// sum over chunks on the host side. anderson_gram_chunks: the chunk count to allocate for.
int anderson_gram_chunks(int64_t bsz, int64_t d);
// G (nullable): stored G = F - X rows (same layout); rows with their bit set in `fresh` are
// recomputed from F - X and written to G, the others are read from G.
// F: fp32 or bf16 (f_dtype), same element layout as X; X and G: h_dtype (fp32 or bf16).
void anderson_gram(const void* X, const void* F, int f_dtype, void* G, unsigned fresh, float* partials, int64_t bsz,
                   int64_t d, int64_t row_stride, int64_t batch_stride, int n, int last, int chunks, hipStream_t stream,
                   int h_dtype = 7);
// X[b, slot] = beta * sum_i alpha[b][i] F[b, i] + (1 - beta) * sum_i alpha[b][i] X[b, i] (i < n);
// z (nullable, [bsz][d], dtype z_dtype): the new iterate cast to the model dtype.
void anderson_mix(void* X, const void* F, int f_dtype, const float* alpha, void* z, int z_dtype, int64_t bsz,
                  int64_t d, int64_t row_stride, int64_t batch_stride, int n, int slot, float beta, hipStream_t stream,
                  int h_dtype = 7);
// anderson_solve: from anderson_gram's partials, alpha[b][0..n) of the regularised Anderson system
// [[0, 1^T], [1, G G^T + lam I]] a = e_0 (a[1..n]) per batch element (bsz <= 1024, one launch),
// and (res nullable) the relative residual of row `last` into res[0].
void anderson_solve(const float* partials, int chunks, int64_t bsz, int n, int last, float lam, float* alpha,
                    float* res, hipStream_t stream);
// adjoint_step: u_new = vjp + grad (dtype), partials[blocks] = per-workgroup sums of (u_new - u)^2
// (fp32; n % 8 == 0, 16-byte aligned, same memory layout); adjoint_step_blocks: the grid size.
int adjoint_step_blocks(int64_t n);
void adjoint_step(const void* vjp, const void* grad, const void* u, void* u_new, float* partials, int blocks,
                  int64_t n, int dtype, hipStream_t stream);

// ---- fused NHWC GroupNorm (+ add, + ReLU on its input); one workgroup per sample ---------
// forward: h = [relu](x [+ add]) (stored when h != nullptr); y = GN(h) * w + b (w/b fp32, nullable);
// mean / rstd [N][G] fp32 saved. backward: dh = d(GN)/dh [* (h > 0) when relu], the gradient of
// both x and add; partials[N][2][C] = per-sample (dw, db).
// y_stride: y's sample stride in elements (0: HW * C, dense) — y can be an Anderson history slot.
void groupnorm_nhwc_fwd(const void* x, const void* add, void* h, void* y, const float* w, const float* b, float* mean,
                        float* rstd, int64_t N, int64_t HW, int64_t C, int64_t G, bool relu, float eps, int dtype,
                        hipStream_t stream, int64_t y_stride = 0);
void groupnorm_nhwc_bwd(const void* dy, const void* h, const float* mean, const float* rstd, const float* w, void* dh,
                        float* partials, int64_t N, int64_t HW, int64_t C, int64_t G, bool relu, int dtype,
                        hipStream_t stream);

// ---- the DEQ cell in one kernel per evaluation (kernels/deq_cell.hip) ----------------------
// f(z, x) = GN3(relu(z + GN2(x + conv2(GN1(relu(conv1 z)))))) on NHWC bf16 [N][H*W][48]; one
// workgroup per sample, everything LDS-resident. w1 / w2: [C][9C] bf16 with k = tap * C + ci.
// gn_w / gn_b: 3 fp32 vectors each (nullable). out (bf16, sample stride out_stride elements, 0 =
// dense) and/or out32 (fp32, sample stride out32_stride elements); h[3] (the GroupNorm inputs) and mean / rstd[3] ([N][G]) nullable.
// vjp: J_f(z)^T u from that state; w2t / w1t are the transposed tap-flipped filters (k = tap * C + co).
bool deq_cell_supported(int64_t H, int64_t W, int64_t C, int64_t G);
void deq_cell_fwd(const void* z, const void* x, const void* w1, const void* w2, const float* const* gn_w,
                  const float* const* gn_b, void* out, float* out32, int64_t out32_stride, void* const* h,
                  float* const* mean, float* const* rstd, int64_t N, int64_t H, int64_t W, int64_t C, int64_t G,
                  float eps, hipStream_t stream, int64_t out_stride = 0);
// grad / ss_part (nullable together): the adjoint update fused in, out = bf16(J^T u + grad) and
// ss_part[N] the per-sample sum of (out - u)^2; deq_adjoint_check sums them (ss_out) and tests
// flag = (sum <= *thresh2) in one tiny launch.
void deq_cell_vjp(const void* u, const void* const* h, const void* w2t, const void* w1t, const float* const* gn_w,
                  const float* const* mean, const float* const* rstd, void* out, const void* grad, float* ss_part,
                  int64_t N, int64_t H, int64_t W, int64_t C, int64_t G, hipStream_t stream);
void deq_adjoint_check(const float* part, int64_t n, const float* thresh2, float* ss_out, float* flag,
                       hipStream_t stream);

// ---- GELU backward + bias gradient (transformer MLP fc1) ---------------------------------
// dh = dy * gelu'(h) (exact erf form); partials[blocks][N] = per-workgroup column sums of dh
// (sum with gemm_splitk_reduce). N/8 must be a multiple of 64, <= 1024.
int gelu_bwd_bias_blocks(int64_t rows);
// Column sums of a row-major [rows][N] matrix (N % 8 == 0, N <= 8192) into per-workgroup fp32
// partial rows [blocks][N] (sum them with gemm_splitk_reduce): the bias gradient of a Linear.
int colsum_blocks(int64_t rows);
// Measurement tool: `blocks` workgroups holding their CU slots for `microseconds` of wall time
// on `stream` (stands in for RCCL's kernels at world size 1, where RCCL launches none).
void emulate_comm(int blocks, double microseconds, hipStream_t stream, int threads, int lds_bytes);
void colsum(const void* x, float* partials, int blocks, int64_t rows, int64_t N, int dtype, hipStream_t stream);
void gelu_bwd_bias(const void* dy, const void* h, void* dh, float* partials, int blocks, int64_t rows, int64_t N,
                   int dtype, hipStream_t stream);
// GELU form of the fused GELU kernels (gelu_bwd_bias, gemm_nt EPI 1 / 2): 1 tanh (NNlib's `gelu`,
// the default), 0 exact erf. Host-side switch read at launch.
void gelu_set_form(int tanh_form);
// g = gelu(h) (the selected form) over n bf16 / fp16 elements, n % 8 == 0, 16-B aligned
void gelu_fwd(const void* h, void* g, int64_t n, int dtype, hipStream_t stream);
int gelu_form();

// ---- fused softmax cross-entropy (csrc/kernels/xent.hip) --------------------------------------
// Logits x [B, C] contiguous (dtype bf16 / fp16 / fp32), arithmetic fp32. mode 0 hard labels, 1 mixed
// labels (partner row B - 1 - b; lam by value, or read from dev_lam when not null), 2 dense targets
// [B, C] (target_dtype fp32 / bf16 / fp16). labels: int32 / int64 (label_dtype), compared and never
// used as an address; in mode 2 they are optional and serve the rank only. eps: label smoothing in
// [0, 1). None of the three allocates, copies or synchronises.
// forward: loss_row, m (row max), s (sum of exp(x - m)) per row in fp32; rank (optional, needs
// labels): the number of classes that beat the row's label, ties broken towards the lower index.
void xent_fwd(const void* x, const void* labels, const void* target, float* loss_row, float* m, float* s,
              int32_t* rank, int64_t B, int64_t C, int dtype, int label_dtype, int target_dtype, int mode, float eps,
              float lam, const float* dev_lam, hipStream_t stream);
// One workgroup: loss[0] = sum_b loss_row[b] in a fixed order (reduction 1), times fl32(1/B)
// (reduction 0); loss may be null. meter (optional, needs rank): 8 words {fp64 sum of the row
// losses, int64 rows, int64 #(rank < k0), int64 #(rank < k1)}, the batch added by one thread.
void xent_finish(const float* loss_row, const int32_t* rank, float* loss, void* meter, int64_t B, int reduction,
                 int k0, int k1, hipStream_t stream);
// backward: dx = (softmax(x) W - t) gs in x's dtype, one rounding; gs = g[0] fl32(1/B) (reduction 0),
// g[0] (1) or g[row] (2), g read on the device.
void xent_bwd(const void* x, const void* labels, const void* target, const float* m, const float* s, const float* g,
              void* dx, int64_t B, int64_t C, int dtype, int label_dtype, int target_dtype, int mode, int reduction,
              float eps, float lam, const float* dev_lam, hipStream_t stream);

}  // namespace fluxmpi
