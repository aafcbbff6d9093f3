// pybind11 bindings of the fluxmpi_amd native library -> module `fluxmpi_amd._C`.
//
// Pointers and streams cross the boundary as integers (tensor.data_ptr(),
// torch.cuda.Stream.cuda_stream), which keeps this module independent of the
// ATen C++ ABI and lets it launch on any stream, including during HIP-graph
// capture.
#include <array>
#include <optional>
#include <tuple>
#include <type_traits>
#include <pybind11/pybind11.h>
#include <pybind11/stl.h>

#include "api.h"
#include "comm/rccl_comm.h"

namespace py = pybind11;
using namespace fluxmpi;

// The one place an integer becomes a pointer again. Py<T> is how Python passes a parameter of C type
// T: uintptr_t for every pointer (hipStream_t is one), T itself otherwise; ptr<T> converts back.
// raw(&fn) is fn with that applied to every parameter, in fn's own parameter order.
template <typename T> using Py = std::conditional_t<std::is_pointer_v<T>, uintptr_t, T>;

template <typename T> T ptr(Py<T> v) {
  if constexpr (std::is_pointer_v<T>) return reinterpret_cast<T>(v);
  else return v;
}

template <typename T> std::array<T, 3> ptr3(const std::array<uintptr_t, 3>& v) {
  return {ptr<T>(v[0]), ptr<T>(v[1]), ptr<T>(v[2])};
}

template <typename R, typename... A> auto raw(R (*fn)(A...)) {
  return [fn](Py<A>... a) -> R { return fn(ptr<A>(a)...); };
}

using Ptrs = const std::vector<uintptr_t>&;
using Ptrs3 = std::array<uintptr_t, 3>;

// ---- the fused optimisers' entries ----------------------------------------------------------------
// Behind the parameters `_C` has always had, the update entries take two trailing keywords, both off
// by default: `dev_skip` (loss scaling: the device predicate that calls the launch off) and `sr`
// (stochastic rounding). `sr` is ONE optional keyword, None or the tuple (seed, sr_stream, step,
// dev_step, offsets), because seed = 0, step = 0 is a valid generator state: "on" cannot be read off
// the values. A call that passes neither reaches the kernels with SrHyper* null and dev_skip null.
static SrHyper sr_hyper(uint64_t seed, uint32_t sr_stream, uint32_t step, uintptr_t dev_step,
                        const std::vector<int64_t>& offsets) {
  return SrHyper{seed, sr_stream, step, ptr<const uint32_t*>(dev_step), offsets.empty() ? nullptr : offsets.data(),
                 offsets.size()};
}
using SrArg = const std::optional<std::tuple<uint64_t, uint32_t, uint32_t, uintptr_t, std::vector<int64_t>>>&;
// *sr as an SrHyper in `h` (which points into sr's offsets), or null
static const SrHyper* sr_or_null(SrArg sr, SrHyper& h) {
  if (!sr) return nullptr;
  h = std::apply(sr_hyper, *sr);
  return &h;
}

static void py_mt_adam(Ptrs p, Ptrs g, Ptrs mm, Ptrs vv, Ptrs master,
                       const std::vector<int64_t>& numel, int p_dtype, int g_dtype, int s_dtype, double lr, double beta1,
                       double beta2, double eps, double bc1, double bc2, double weight_decay, float grad_scale,
                       uintptr_t dev_hyper, uintptr_t dev_gscale, uintptr_t stream, uintptr_t tscale, float clip_delta,
                       uintptr_t dev_skip, SrArg sr) {
  SrHyper s;
  AdamHyper h{lr, beta1, beta2, eps, bc1, bc2, weight_decay, grad_scale, ptr<const float*>(dev_hyper),
              ptr<const float*>(dev_gscale)};
  h.tscale = ptr<const void*>(tscale);
  h.clip_delta = clip_delta;
  h.dev_skip = ptr<const int32_t*>(dev_skip);
  mt_adam(p, g, mm, vv, master, numel, p_dtype, g_dtype, s_dtype, h, ptr<hipStream_t>(stream), sr_or_null(sr, s));
}

static void py_mt_sgd(Ptrs p, Ptrs g, Ptrs buf, Ptrs master, const std::vector<int64_t>& numel, int p_dtype,
                      int g_dtype, int s_dtype, double lr, double momentum, double weight_decay,
                      float grad_scale, int nesterov, uintptr_t dev_lr, uintptr_t stream, uintptr_t dev_gscale,
                      uintptr_t tscale, float clip_delta, uintptr_t dev_skip, SrArg sr) {
  SrHyper s;
  SgdHyper h{lr, momentum, weight_decay, grad_scale, nesterov, ptr<const float*>(dev_lr)};
  h.dev_gscale = ptr<const float*>(dev_gscale);
  h.tscale = ptr<const void*>(tscale);
  h.clip_delta = clip_delta;
  h.dev_skip = ptr<const int32_t*>(dev_skip);
  mt_sgd(p, g, buf, master, numel, p_dtype, g_dtype, s_dtype, h, ptr<hipStream_t>(stream), sr_or_null(sr, s));
}

static void py_mt_rule(int kind, Ptrs p, Ptrs g, Ptrs s1, Ptrs s2, Ptrs s3, Ptrs master,
                       const std::vector<int64_t>& numel, int p_dtype, int g_dtype, int s_dtype, double lr, double beta1,
                       double beta2, double eps, double bt1, double bt2, double weight_decay, float grad_scale,
                       uintptr_t dev_hyper, uintptr_t dev_gscale, uintptr_t tscale, float clip_delta, uintptr_t stream,
                       uintptr_t dev_skip, SrArg sr) {
  SrHyper s;
  RuleHyper h{kind, lr, beta1, beta2, eps, bt1, bt2, weight_decay, grad_scale, ptr<const float*>(dev_hyper),
              ptr<const float*>(dev_gscale), ptr<const void*>(tscale), clip_delta, ptr<const int32_t*>(dev_skip)};
  mt_rule(p, g, s1, s2, s3, master, numel, p_dtype, g_dtype, s_dtype, h, ptr<hipStream_t>(stream), sr_or_null(sr, s));
}

// the two trailing keywords of the update entries (above)
#define SKIP_SR_ARGS py::arg("dev_skip") = uintptr_t(0), py::arg("sr") = py::none()

PYBIND11_MODULE(_C, m) {
  m.doc() = "fluxmpi_amd native library: gfx950 HIP kernels + RCCL communicator";

  m.def("mt_copy", raw(&mt_copy), py::arg("src"), py::arg("dst"), py::arg("numel"), py::arg("in_dtype"),
        py::arg("out_dtype"), py::arg("scale"), py::arg("stream"));
  m.def("mt_fill", raw(&mt_fill));
  m.def("mt_sumsq", raw(&mt_sumsq));

  m.def("mt_adam", &py_mt_adam, py::arg("param"), py::arg("grad"), py::arg("m"), py::arg("v"), py::arg("master"),
        py::arg("numel"), py::arg("p_dtype"), py::arg("g_dtype"), py::arg("s_dtype"), py::arg("lr"), py::arg("beta1"),
        py::arg("beta2"), py::arg("eps"), py::arg("bc1"), py::arg("bc2"), py::arg("weight_decay"),
        py::arg("grad_scale"), py::arg("dev_hyper"), py::arg("dev_gscale"), py::arg("stream"),
        py::arg("tscale") = uintptr_t(0), py::arg("clip_delta") = 0.f, SKIP_SR_ARGS);
  m.def("adam_advance", raw(&adam_advance), py::arg("dev"), py::arg("beta1"), py::arg("beta2"), py::arg("stream"),
        py::arg("dev_skip") = uintptr_t(0));
  m.def("mt_sgd", &py_mt_sgd, py::arg("param"), py::arg("grad"), py::arg("buf"), py::arg("master"), py::arg("numel"),
        py::arg("p_dtype"), py::arg("g_dtype"), py::arg("s_dtype"), py::arg("lr"), py::arg("momentum"),
        py::arg("weight_decay"), py::arg("grad_scale"), py::arg("nesterov"), py::arg("dev_lr"), py::arg("stream"),
        py::arg("dev_gscale") = uintptr_t(0), py::arg("tscale") = uintptr_t(0), py::arg("clip_delta") = 0.f,
        SKIP_SR_ARGS);
  m.def("mt_rule", &py_mt_rule, py::arg("kind"), py::arg("param"), py::arg("grad"), py::arg("s1"), py::arg("s2"),
        py::arg("s3"), py::arg("master"), py::arg("numel"), py::arg("p_dtype"), py::arg("g_dtype"), py::arg("s_dtype"),
        py::arg("lr"), py::arg("beta1"), py::arg("beta2"), py::arg("eps"), py::arg("bt1"), py::arg("bt2"),
        py::arg("weight_decay"), py::arg("grad_scale"), py::arg("dev_hyper"), py::arg("dev_gscale"),
        py::arg("tscale"), py::arg("clip_delta"), py::arg("stream"), SKIP_SR_ARGS);
  // stochastic rounding as a stand-alone cast; sr_advance steps the device block `dev_step` points at
  m.def(
      "mt_stochastic_round",
      [](Ptrs dst, Ptrs src, const std::vector<int64_t>& numel, uintptr_t dev_skip, uintptr_t stream, uint64_t seed,
         uint32_t sr_stream, uint32_t step, uintptr_t dev_step, const std::vector<int64_t>& offsets) {
        mt_stochastic_round(dst, src, numel, sr_hyper(seed, sr_stream, step, dev_step, offsets),
                            ptr<const int32_t*>(dev_skip), ptr<hipStream_t>(stream));
      },
      py::arg("dst"), py::arg("src"), py::arg("numel"), py::arg("dev_skip"), py::arg("stream"), py::arg("seed"),
      py::arg("sr_stream"), py::arg("step"), py::arg("dev_step"), py::arg("offsets"));
  m.def("sr_advance", raw(&sr_advance), py::arg("block"), py::arg("dev_skip"), py::arg("stream"));

  // ---- gradient clipping, loss scaling (nonfinite_flag, dev_pre: the scaler's, null without) ----
  m.def("sumsq_partials", &sumsq_partials, py::arg("numel"));
  m.def("mt_leaf_sumsq", raw(&mt_leaf_sumsq), py::arg("grad"), py::arg("numel"), py::arg("g_dtype"),
        py::arg("partials"), py::arg("sumsq"), py::arg("scale"), py::arg("omega"), py::arg("grad_scale"),
        py::arg("stream"), py::arg("nonfinite_flag") = uintptr_t(0), py::arg("dev_pre") = uintptr_t(0));
  m.def("clip_total", raw(&clip_total), py::arg("sumsq"), py::arg("n"), py::arg("acc_dtype"), py::arg("slot"),
        py::arg("accumulate"), py::arg("omega"), py::arg("grad_scale"), py::arg("stream"),
        py::arg("dev_pre") = uintptr_t(0));
  m.def("mt_check_finite", raw(&mt_check_finite), py::arg("grad"), py::arg("numel"), py::arg("g_dtype"),
        py::arg("flag"), py::arg("stream"));
  m.def("loss_scale_update", raw(&loss_scale_update), py::arg("block"), py::arg("growth"), py::arg("backoff"),
        py::arg("interval"), py::arg("min_scale"), py::arg("max_scale"), py::arg("stream"));

  // ---- exponential moving average of the weights ------------------------------------
  m.def("mt_ema", raw(&mt_ema), py::arg("ema"), py::arg("src"), py::arg("numel"), py::arg("src_dtype"),
        py::arg("omd"), py::arg("dev_block"), py::arg("dev_skip"), py::arg("stream"));
  m.def("ema_advance", raw(&ema_advance), py::arg("block"), py::arg("decay"), py::arg("warmup"), py::arg("every"),
        py::arg("dev_skip"), py::arg("stream"));

  // ---- the device input pipeline (augment.hip): AugHyper's arguments travel as keywords; `dev_block`
  // (or 0) is the device block of aug_block_set ----
  m.def(
      "augment_batch",
      [](uintptr_t in, uintptr_t out, int64_t B, int H, int W, int h, int w, int C, int dtype, uint64_t seed,
         uint32_t aug_stream, uint32_t step, int64_t sample_offset, int mode, std::array<int, 4> box, float lam, int pad,
         int fill, int crop_center, int flip, std::array<float, 3> a, std::array<float, 3> b, uintptr_t dev_block,
         uintptr_t stream) {
        AugHyper hy{seed, aug_stream, step, sample_offset, mode, box[0], box[1], box[2], box[3], lam, pad, fill,
                    crop_center, flip, {a[0], a[1], a[2]}, {b[0], b[1], b[2]}, ptr<const uint32_t*>(dev_block)};
        augment_batch(ptr<const void*>(in), ptr<void*>(out), B, H, W, h, w, C, dtype, hy, ptr<hipStream_t>(stream));
      },
      py::arg("input"), py::arg("out"), py::arg("B"), py::arg("H"), py::arg("W"), py::arg("h"), py::arg("w"),
      py::arg("C"), py::arg("dtype"), py::arg("seed"), py::arg("aug_stream"), py::arg("step"),
      py::arg("sample_offset"), py::arg("mode"), py::arg("box"), py::arg("lam"), py::arg("pad"), py::arg("fill"),
      py::arg("crop_center"), py::arg("flip"), py::arg("a"), py::arg("b"), py::arg("dev_block"), py::arg("stream"));
  m.def(
      "aug_block_set",
      [](uintptr_t block, uint32_t step, int mode, std::array<int, 4> box, float lam, uintptr_t stream) {
        aug_block_set(ptr<void*>(block), step, mode, box[0], box[1], box[2], box[3], lam, ptr<hipStream_t>(stream));
      },
      py::arg("block"), py::arg("step"), py::arg("mode"), py::arg("box"), py::arg("lam"), py::arg("stream"));

  // ---- ResNet one-pass nodes: the backward around the dual BatchNorm of a stage-1 downsample block
  // (conv3ds_bwd.hip); bn2 apply + ReLU + conv3 forward (bn_relu_conv1x1_fwd.hip) ----
  m.def("conv3ds_bwd", raw(&conv3ds_bwd), py::arg("dy"), py::arg("mask"), py::arg("c3"), py::arg("cds"), py::arg("w"),
        py::arg("mean"), py::arg("inv"), py::arg("sum_dy"), py::arg("sum_dy_xhat"), py::arg("w2"), py::arg("mean2"),
        py::arg("inv2"), py::arg("sum_dy2"), py::arg("sum_dy_xhat2"), py::arg("a2"), py::arg("x"), py::arg("wt3"),
        py::arg("wtds"), py::arg("d_a2"), py::arg("d_xside"), py::arg("ws3"), py::arg("wsds"), py::arg("P"),
        py::arg("slabs"), py::arg("stream"));
  m.def("bn_relu_conv1x1_fwd_supported", &bn_relu_conv1x1_fwd_supported, py::arg("Cin"), py::arg("Cout"));
  m.def("bn_relu_conv1x1_fwd", raw(&bn_relu_conv1x1_fwd), py::arg("c2"), py::arg("scale"), py::arg("shift"),
        py::arg("wt"), py::arg("a2"), py::arg("c3"), py::arg("stats"), py::arg("P"), py::arg("Cin"), py::arg("Cout"),
        py::arg("stream"));

  // ---- fused NHWC BatchNorm ------------------------------------------------
  m.def("bn_fwd_train", raw(&bn_fwd_train));
  m.def("bn_fwd_infer", raw(&bn_fwd_infer));
  m.def("bn_bwd", raw(&bn_bwd));
  m.def("bn_stats_finalize", raw(&bn_stats_finalize));
  m.def("bn_apply", raw(&bn_apply));

  // ---- synchronised BatchNorm (deterministic reductions, split at the collectives) ----
  m.def("bn_sync_workspace_floats", &bn_sync_workspace_floats);
  m.def("bn_sync_stats", raw(&bn_sync_stats));
  m.def("bn_sync_finalize_fwd", raw(&bn_sync_finalize_fwd));
  m.def("bn_sync_bwd_reduce", raw(&bn_sync_bwd_reduce));
  m.def("bn_sync_bwd_dx", raw(&bn_sync_bwd_dx));

  m.def("bn_apply_dual", raw(&bn_apply_dual));
  m.def("bn_bwd_dual", raw(&bn_bwd_dual));

  // ---- fused stem pool -------------------------------------------------------
  m.def("bn_relu_maxpool_fwd", raw(&bn_relu_maxpool_fwd));
  m.def("attn_fwd", raw(&attn_fwd));
  m.def("attn_bwd", raw(&attn_bwd), py::arg("q"), py::arg("k"), py::arg("v"), py::arg("o"), py::arg("dout"),
        py::arg("dq"), py::arg("dk"), py::arg("dv"), py::arg("stats"), py::arg("sq_b"), py::arg("sq_t"),
        py::arg("so_b"), py::arg("so_t"), py::arg("so_h"), py::arg("sg_b"), py::arg("sg_t"), py::arg("B"),
        py::arg("T"), py::arg("H"), py::arg("Dh"), py::arg("scale"), py::arg("stream"), py::arg("colpart") = 0);
  m.def("attn_bwd_colpart_rows", &attn_bwd_colpart_rows);
  m.def("attn_dispatch", [](int B, int T, int H) {
    const AttnDispatch d = attn_dispatch(B, T, H);
    return py::make_tuple(std::string(d.fwd), std::string(d.bwd), d.fwd_parts, d.bwd_parts);
  });
  m.def("pad_c3_to_c4", raw(&pad_c3_to_c4));
  m.def("stem_fwd", raw(&stem_fwd), py::arg("x"), py::arg("wp"), py::arg("y"), py::arg("stats"), py::arg("n"),
        py::arg("stream"), py::arg("max_blocks") = 0);
  m.def("stem_bwd_blocks", &stem_bwd_blocks);
  m.def("stem_part_floats", &stem_part_floats);
  m.def("stem_bwd", raw(&stem_bwd));
  m.def("maxpool_bwd", raw(&maxpool_bwd));

  // ---- Anderson solver (DEQ) ---------------------------------------------------
  m.def("anderson_gram_chunks", &anderson_gram_chunks);
  m.def("anderson_gram", raw(&anderson_gram), py::arg("X"), py::arg("F"), py::arg("fdt"), py::arg("G"),
        py::arg("fresh"), py::arg("part"), py::arg("bsz"), py::arg("d"), py::arg("rs"), py::arg("bs"), py::arg("n"),
        py::arg("last"), py::arg("chunks"), py::arg("stream"), py::arg("hdt") = 7);
  m.def("adjoint_step_blocks", &adjoint_step_blocks);
  m.def("adjoint_step", raw(&adjoint_step));
  m.def("anderson_solve", raw(&anderson_solve));
  m.def("anderson_mix", raw(&anderson_mix), py::arg("X"), py::arg("F"), py::arg("fdt"), py::arg("alpha"),
        py::arg("z"), py::arg("zdt"), py::arg("bsz"), py::arg("d"), py::arg("rs"), py::arg("bs"), py::arg("n"),
        py::arg("slot"), py::arg("beta"), py::arg("stream"), py::arg("hdt") = 7);

  // ---- fused NHWC GroupNorm ------------------------------------------------------
  m.def("groupnorm_nhwc_fwd", raw(&groupnorm_nhwc_fwd));
  m.def("groupnorm_nhwc_bwd", raw(&groupnorm_nhwc_bwd));

  // ---- the DEQ cell in one kernel ------------------------------------------------------
  m.def("deq_cell_supported", &deq_cell_supported);
  m.def("deq_cell_fwd", [](uintptr_t z, uintptr_t x, uintptr_t w1, uintptr_t w2, Ptrs3 gw, Ptrs3 gb, uintptr_t out,
                           uintptr_t out32, int64_t out32_stride, Ptrs3 h, Ptrs3 mean, Ptrs3 rstd, int64_t N,
                           int64_t H, int64_t W, int64_t C, int64_t G, float eps, uintptr_t stream,
                           int64_t out_stride) {
    deq_cell_fwd(ptr<const void*>(z), ptr<const void*>(x), ptr<const void*>(w1), ptr<const void*>(w2),
                 ptr3<const float*>(gw).data(), ptr3<const float*>(gb).data(), ptr<void*>(out), ptr<float*>(out32),
                 out32_stride, ptr3<void*>(h).data(), ptr3<float*>(mean).data(), ptr3<float*>(rstd).data(), N, H, W,
                 C, G, eps, ptr<hipStream_t>(stream), out_stride);
  });
  m.def("deq_cell_vjp", [](uintptr_t u, Ptrs3 h, uintptr_t w2t, uintptr_t w1t, Ptrs3 gw, Ptrs3 mean, Ptrs3 rstd,
                           uintptr_t out, uintptr_t grad, uintptr_t ss_part, int64_t N, int64_t H, int64_t W,
                           int64_t C, int64_t G, uintptr_t stream) {
    deq_cell_vjp(ptr<const void*>(u), ptr3<const void*>(h).data(), ptr<const void*>(w2t), ptr<const void*>(w1t),
                 ptr3<const float*>(gw).data(), ptr3<const float*>(mean).data(), ptr3<const float*>(rstd).data(),
                 ptr<void*>(out), ptr<const void*>(grad), ptr<float*>(ss_part), N, H, W, C, G,
                 ptr<hipStream_t>(stream));
  });
  m.def("deq_adjoint_check", raw(&deq_adjoint_check));

  // ---- GELU backward + bias gradient -------------------------------------------------
  m.def("gelu_bwd_bias_blocks", &gelu_bwd_bias_blocks);
  m.def("colsum_blocks", &colsum_blocks);
  m.def("emulate_comm", raw(&emulate_comm));
  m.def("wgrad256_supported", &wgrad256_supported);
  m.def("wgrad256_actual_splits", &wgrad256_actual_splits);
  m.def("wgrad256_set_variant", &wgrad256_set_variant);
  m.def("gemm_wgrad256", raw(&gemm_wgrad256));
  m.def("gemm_nt_supported", &gemm_nt_supported);
  m.def("gemm_nt_colpart_rows", &gemm_nt_colpart_rows);
  m.def("gemm_nt_set_split", &gemm_nt_set_split);
  m.def("gemm_nt_get_split", &gemm_nt_get_split);
  m.def("gemm_nt", [](uintptr_t a, uintptr_t b, uintptr_t c, uintptr_t c2, uintptr_t bias, int bias_f32, uintptr_t h,
                      uintptr_t colpart, int64_t lda, int64_t ldb, int64_t ldc, int64_t M, int64_t N, int64_t K,
                      int epi, uintptr_t stream) {
    raw(&gemm_nt)(a, b, c, c2, bias, bias_f32, h, colpart, 0, lda, ldb, ldc, M, N, K, epi, stream);
  });
  m.def("gemm_nt_stats", [](uintptr_t a, uintptr_t b, uintptr_t c, uintptr_t stats, int64_t lda, int64_t ldb,
                            int64_t ldc, int64_t M, int64_t N, int64_t K, uintptr_t stream) {
    raw(&gemm_nt)(a, b, c, 0, 0, 0, 0, 0, stats, lda, ldb, ldc, M, N, K, 3, stream);
  });
  m.def("linear_bwd_supported", &linear_bwd_supported);
  m.def("linear_bwd_splits", &linear_bwd_splits);
  m.def("linear_bwd", raw(&linear_bwd));
  m.def("conv_c3_supported", &conv_c3_supported);
  m.def("conv_c3_wgrad_blocks", &conv_c3_wgrad_blocks);
  m.def("conv_c3_fwd", raw(&conv_c3_fwd));
  m.def("conv_c3_wgrad", raw(&conv_c3_wgrad));
  m.def("conv3x3n_supported", &conv3x3n_supported);
  m.def("conv3x3n_slots128", &conv3x3n_slots128);
  m.def("conv3x3n", raw(&conv3x3n));
  m.def("wgrad3x3n_supported", &wgrad3x3n_supported);
  m.def("wgrad3x3n_splits", &wgrad3x3n_splits);
  m.def("wgrad3x3n_groups", &wgrad3x3n_groups);
  m.def("wgrad3x3n", raw(&wgrad3x3n));
  m.def("gemm_nt_conv_supported", &gemm_nt_conv_supported);
  m.def("gemm_nt_conv", raw(&gemm_nt_conv));
  m.def("transpose_bf16", raw(&transpose_bf16));
  m.def("colsum", raw(&colsum));
  m.def("gelu_bwd_bias", raw(&gelu_bwd_bias));

  m.def("gelu_set_form", &gelu_set_form);
  m.def("gelu_fwd", raw(&gelu_fwd));
  m.def("gelu_form", &gelu_form);

  // ---- fused LayerNorm ------------------------------------------------------
  m.def("layernorm_fwd", raw(&layernorm_fwd));
  m.def("layernorm_bwd", raw(&layernorm_bwd));

  // ---- MFMA GEMM (1x1 conv) -------------------------------------------------
  m.def("gemm_bf16",
        [](uintptr_t a, uintptr_t b, uintptr_t c, int64_t lda, int64_t ldb, int64_t ldc, int64_t M, int64_t N,
           int64_t K, bool a_kmajor, bool b_kmajor, int mode, int splits, uintptr_t a_scale, uintptr_t a_shift,
           uintptr_t b_scale, uintptr_t b_shift, uintptr_t stats, int tile_m, int tile_n, uintptr_t stream, int nbuf,
           uintptr_t res, int64_t ldr, uintptr_t bnb_x, uintptr_t bnb_w, uintptr_t bnb_b, uintptr_t bnb_mean,
           uintptr_t bnb_inv, uintptr_t bnb_mask, int bnb_rm, int conv_h, int conv_w, int conv_c, int engine,
           uintptr_t res_mask, int res_sub_h, int res_sub_w, int a_sub_h, int a_sub_w, int conv_s) {
          using F = const float*;
          using V = const void*;
          using M8 = const uint8_t*;
          GemmProblem g{ptr<V>(a), ptr<V>(b), ptr<void*>(c), lda, ldb, ldc, M, N, K, a_kmajor, b_kmajor, mode, splits,
                        ptr<F>(a_scale), ptr<F>(a_shift), ptr<F>(b_scale), ptr<F>(b_shift), ptr<float*>(stats), tile_m,
                        tile_n, nbuf, ptr<V>(res), ldr, ptr<V>(bnb_x), ptr<F>(bnb_w), ptr<F>(bnb_b), ptr<F>(bnb_mean),
                        ptr<F>(bnb_inv), ptr<M8>(bnb_mask), bnb_rm, conv_h, conv_w, conv_c, engine, ptr<M8>(res_mask),
                        res_sub_h, res_sub_w, a_sub_h, a_sub_w, conv_s};
          gemm_bf16(g, ptr<hipStream_t>(stream));
        },
        py::arg("a"), py::arg("b"), py::arg("c"), py::arg("lda"), py::arg("ldb"), py::arg("ldc"), py::arg("M"),
        py::arg("N"), py::arg("K"), py::arg("a_kmajor"), py::arg("b_kmajor"), py::arg("mode"), py::arg("splits"),
        py::arg("a_scale"), py::arg("a_shift"), py::arg("b_scale"), py::arg("b_shift"), py::arg("stats"),
        py::arg("tile_m"), py::arg("tile_n"), py::arg("stream"), py::arg("nbuf") = 0, py::arg("res") = 0,
        py::arg("ldr") = 0, py::arg("bnb_x") = 0, py::arg("bnb_w") = 0, py::arg("bnb_b") = 0,
        py::arg("bnb_mean") = 0, py::arg("bnb_inv") = 0, py::arg("bnb_mask") = 0, py::arg("bnb_rm") = 0,
        py::arg("conv_h") = 0, py::arg("conv_w") = 0, py::arg("conv_c") = 0, py::arg("engine") = 0,
        py::arg("res_mask") = 0, py::arg("res_sub_h") = 0, py::arg("res_sub_w") = 0, py::arg("a_sub_h") = 0,
        py::arg("a_sub_w") = 0, py::arg("conv_s") = 1);

  m.def("gemm_wgrad", raw(&gemm_wgrad), py::arg("a"), py::arg("b"), py::arg("ws"), py::arg("lda"), py::arg("ldb"),
        py::arg("M"), py::arg("N"), py::arg("K"), py::arg("splits"), py::arg("conv_h") = 0, py::arg("conv_w") = 0,
        py::arg("conv_c") = 0, py::arg("stream") = 0, py::arg("variant") = 0, py::arg("b_sub") = 0);

  m.def("transpose_filters", raw(&transpose_filters), py::arg("src"), py::arg("dst"), py::arg("co"), py::arg("ci"),
        py::arg("taps"), py::arg("stream"));

  m.def("gemm_splitk_reduce_seg", raw(&gemm_splitk_reduce_seg));
  m.def("gemm_splitk_reduce", raw(&gemm_splitk_reduce), py::arg("ws"), py::arg("splits"), py::arg("n"),
        py::arg("out"), py::arg("out_dtype"), py::arg("stream"));

  // ---- RCCL ----------------------------------------------------------------
  m.def("rccl_unique_id", []() { return py::bytes(rccl_unique_id()); });
  m.def("rccl_version", &rccl_version);
  py::class_<RcclComm>(m, "RcclComm")
      .def(py::init<const std::string&, int, int, int>(), py::call_guard<py::gil_scoped_release>())
      .def("allreduce", &RcclComm::allreduce, py::call_guard<py::gil_scoped_release>())
      .def("allreduce_many", &RcclComm::allreduce_many, py::call_guard<py::gil_scoped_release>())
      .def("broadcast", &RcclComm::broadcast, py::call_guard<py::gil_scoped_release>())
      .def("reduce", &RcclComm::reduce, py::call_guard<py::gil_scoped_release>())
      .def("allgather", &RcclComm::allgather, py::call_guard<py::gil_scoped_release>())
      .def("reduce_scatter", &RcclComm::reduce_scatter, py::call_guard<py::gil_scoped_release>())
      .def("alltoall", &RcclComm::alltoall, py::call_guard<py::gil_scoped_release>())
      .def("comm_count", &RcclComm::comm_count, py::call_guard<py::gil_scoped_release>())
      .def("comm_user_rank", &RcclComm::comm_user_rank, py::call_guard<py::gil_scoped_release>())
      .def("comm_device", &RcclComm::comm_device, py::call_guard<py::gil_scoped_release>())
      .def("async_error", &RcclComm::async_error, py::call_guard<py::gil_scoped_release>())
      .def_static("error_string", &RcclComm::error_string)
      .def("abort", &RcclComm::abort, py::arg("abort_wait_ms") = 2000, py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("aborted", &RcclComm::aborted)
      .def_property_readonly("is_open", &RcclComm::is_open)
      .def("destroy", &RcclComm::destroy, py::call_guard<py::gil_scoped_release>())
      .def_property_readonly("rank", &RcclComm::rank)
      .def_property_readonly("size", &RcclComm::size)
      .def_property_readonly("device", &RcclComm::device);
}

// A second module of the same shared object (loaded from _C.__file__ by ops/_ext.py: xent()): the
// fused softmax cross-entropy entries, beside `_C` so that its recorded surface stays as it is.
PYBIND11_MODULE(_C_xent, m) {
  m.doc() = "fluxmpi_amd native library: the fused softmax cross-entropy entries (csrc/kernels/xent.hip)";
  m.def("xent_fwd", raw(&xent_fwd), py::arg("x"), py::arg("labels"), py::arg("target"), py::arg("loss_row"),
        py::arg("m"), py::arg("s"), py::arg("rank"), py::arg("B"), py::arg("C"), py::arg("dtype"),
        py::arg("label_dtype"), py::arg("target_dtype"), py::arg("mode"), py::arg("eps"), py::arg("lam"),
        py::arg("dev_lam"), py::arg("stream"));
  m.def("xent_finish", raw(&xent_finish), py::arg("loss_row"), py::arg("rank"), py::arg("loss"), py::arg("meter"),
        py::arg("B"), py::arg("reduction"), py::arg("k0"), py::arg("k1"), py::arg("stream"));
  m.def("xent_bwd", raw(&xent_bwd), py::arg("x"), py::arg("labels"), py::arg("target"), py::arg("m"), py::arg("s"),
        py::arg("g"), py::arg("dx"), py::arg("B"), py::arg("C"), py::arg("dtype"), py::arg("label_dtype"),
        py::arg("target_dtype"), py::arg("mode"), py::arg("reduction"), py::arg("eps"), py::arg("lam"),
        py::arg("dev_lam"), py::arg("stream"));
}

// A third module of the same shared object, loaded the same way: the resampling form of the device
// input pipeline (csrc/kernels/resize_crop.hip). `mode`, `box`, `lam`, `a`, `b` and `dev_block` are
// AugHyper's; `boxes` is the device table int32 [B][5].
PYBIND11_MODULE(_C_rrc, m) {
  m.doc() = "fluxmpi_amd native library: the resized-crop entry (csrc/kernels/resize_crop.hip)";
  m.def(
      "resized_crop_batch",
      [](uintptr_t in, uintptr_t out, uintptr_t boxes, int64_t B, int H, int W, int h, int w, int C, int dtype,
         uint32_t step, int mode, std::array<int, 4> box, float lam, std::array<float, 3> a, std::array<float, 3> b,
         uintptr_t dev_block, uintptr_t stream) {
        AugHyper hy{};
        hy.step = step, hy.mode = mode, hy.y0 = box[0], hy.x0 = box[1], hy.y1 = box[2], hy.x1 = box[3], hy.lam = lam;
        for (int c = 0; c < 3; ++c) hy.a[c] = a[c], hy.b[c] = b[c];
        hy.dev_block = ptr<const uint32_t*>(dev_block);
        resized_crop_batch(ptr<const void*>(in), ptr<void*>(out), ptr<const int32_t*>(boxes), B, H, W, h, w, C, dtype,
                           hy, ptr<hipStream_t>(stream));
      },
      py::arg("input"), py::arg("out"), py::arg("boxes"), py::arg("B"), py::arg("H"), py::arg("W"), py::arg("h"),
      py::arg("w"), py::arg("C"), py::arg("dtype"), py::arg("step"), py::arg("mode"), py::arg("box"), py::arg("lam"),
      py::arg("a"), py::arg("b"), py::arg("dev_block"), py::arg("stream"));
}
