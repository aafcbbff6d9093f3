// Shared by the fused multi-tensor optimiser kernels (optim.hip: Adam, SGD, sums of squares;
// optim_rules.hip: the rest of the rule set; optim_layerwise.hip: LARS, LAMB): the job layout — 4096-element chunks of up to 24
// leaves per launch, the chunk -> leaf map a prefix table in the kernel arguments — and the one
// copy of what the kernels have in common: chunk_of (which chunk a workgroup owns), block_sum /
// block_sum2, the compute type, the gradient clamp and dispatch_opt_combo (the dtype combinations
// every update kernel is built for).
#pragma once
#include <stdexcept>
#include <string>
#include <vector>

#include "../api.h"
#include "common.h"

namespace fluxmpi {

constexpr int kThreads = 256;
constexpr int kVec = 8;
constexpr int kIters = 2;
constexpr int kChunk = kThreads * kVec * kIters;  // 4096 elements per workgroup
constexpr int kMaxT = 24;

struct OptArgs {
  uintptr_t p[kMaxT];
  uintptr_t g[kMaxT];
  uintptr_t s1[kMaxT];
  uintptr_t s2[kMaxT];
  uintptr_t s3[kMaxT];  // third state tensor (AMSGrad), else 0
  uintptr_t w[kMaxT];   // fp32 master (or 0)
  int64_t numel[kMaxT];
  int32_t start[kMaxT + 1];
  int32_t tidx[kMaxT];  // position of the leaf in the CALL's lists (per-leaf scales, sums)
  int64_t pbase;        // workgroups of the call's earlier launches (index of this one's first partial)
  int n;
};

template <typename P> struct Comp { using type = float; };
template <> struct Comp<double> { using type = double; };

// clamp(g, -delta, delta) with torch.clamp's NaN behaviour (a NaN stays a NaN); delta == 0: off
template <typename C>
__device__ __forceinline__ C clip_grad(C g, C delta) {
  if (delta > C(0)) g = g < -delta ? -delta : (g > delta ? delta : g);
  return g;
}

// load8 / store8 for a pointer that may miss 16-byte alignment (`vec` false): element by element then, in
// the same thread -> element layout, so a reduction over a thread's elements adds in the same order
template <typename T>
__device__ __forceinline__ void load8_any(bool vec, const T* __restrict__ p, T (&out)[kVec]) {
  if (vec) {
    load8(p, out);
  } else {
#pragma unroll
    for (int j = 0; j < kVec; ++j) out[j] = p[j];
  }
}
template <typename T>
__device__ __forceinline__ void store8_any(bool vec, T* __restrict__ p, const T (&in)[kVec]) {
  if (vec) {
    store8(p, in);
  } else {
#pragma unroll
    for (int j = 0; j < kVec; ++j) p[j] = in[j];
  }
}

// This workgroup's job: chunk c of the nb chunks of leaf t, elements [base, end) of the leaf.
struct Chunk {
  int t, c, nb;
  int64_t base, end;
};

__device__ __forceinline__ Chunk chunk_of(const OptArgs& a) {
  const int b = blockIdx.x;
  const int t = find_tensor(a.start, a.n, b);
  const int c = b - a.start[t];
  const int64_t base = static_cast<int64_t>(c) * kChunk;
  const int64_t n = a.numel[t];
  return {t, c, a.start[t + 1] - a.start[t], base, base + kChunk < n ? base + kChunk : n};
}

// The step's skip predicate (loss scaling: a non-finite gradient calls the whole step off): one
// wave-uniform load of *dev_skip; a kernel leaves on `true` before its first load of tensor data.
// SKIP == false (dev_skip == nullptr, the launchers' choice) compiles to nothing.
template <bool SKIP>
__device__ __forceinline__ bool step_skipped(const int32_t* dev_skip) {
  if constexpr (SKIP) return *dev_skip != 0;
  else return false;
}

// inf or NaN: the exponent field all ones, read off the bits (exact, no arithmetic)
__device__ __forceinline__ bool nonfinite(f16 x) { return (__builtin_bit_cast(uint16_t, x) & 0x7c00u) == 0x7c00u; }
__device__ __forceinline__ bool nonfinite(bf16 x) { return (__builtin_bit_cast(uint16_t, x) & 0x7f80u) == 0x7f80u; }
__device__ __forceinline__ bool nonfinite(float x) {
  return (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) == 0x7f800000u;
}
__device__ __forceinline__ bool nonfinite(double x) {
  return (__builtin_bit_cast(uint64_t, x) & 0x7ff0000000000000ull) == 0x7ff0000000000000ull;
}

// Block-wide OR of `found` in two halves around ONE barrier: note_found leaves each wave's OR (a
// ballot: no LDS traffic inside the wave) in LDS, raise_noted — after a __syncthreads() — has one
// lane of a workgroup that found something store the sticky flag. A kernel that reduces anyway
// (block_sum has a barrier inside) puts its reduction between the two and pays no second barrier.
__device__ __forceinline__ int* found_slots() {
  __shared__ int wave_found[kThreads / 64];
  return wave_found;
}
__device__ __forceinline__ void note_found(bool found) {
  const bool any = __ballot(found) != 0;  // wave-uniform
  if ((threadIdx.x & 63) == 0) found_slots()[threadIdx.x >> 6] = any;
}
__device__ __forceinline__ void raise_noted(int32_t* __restrict__ flag) {
  if (threadIdx.x == 0) {
    const int* w = found_slots();
    int any = 0;
#pragma unroll
    for (int i = 0; i < kThreads / 64; ++i) any |= w[i];
    if (any) flag[0] = 1;
  }
}

// sum over the workgroup, valid in every thread. Wave level: DPP (fp32) / xor shuffles (fp64), every
// lane takes part (EXEC full); then the four wave totals through LDS, added in wave order. A second
// call in one kernel needs a __syncthreads() in front: it writes the same LDS slots.
template <typename A>
__device__ __forceinline__ A block_sum(A v) {
  __shared__ A wave_tot[kThreads / 64];
  if constexpr (sizeof(A) == 4) {
    v = wave_sum_dpp(v);
  } else {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  }
  if ((threadIdx.x & 63) == 0) wave_tot[threadIdx.x >> 6] = v;
  __syncthreads();
  A s = wave_tot[0];
#pragma unroll
  for (int w = 1; w < kThreads / 64; ++w) s += wave_tot[w];
  return s;
}

// two sums over the workgroup, each valid in every thread
template <typename A>
__device__ __forceinline__ void block_sum2(A ax, A ay, A& sx, A& sy) {
  sx = block_sum(ax);
  __syncthreads();  // block_sum's LDS slots are about to be written again
  sy = block_sum(ay);
}

template <typename F>
void for_each_group(const std::vector<uintptr_t>& p, const std::vector<uintptr_t>& g,
                    const std::vector<uintptr_t>& s1, const std::vector<uintptr_t>& s2,
                    const std::vector<uintptr_t>& s3, const std::vector<uintptr_t>& w,
                    const std::vector<int64_t>& numel, F&& launch) {
  const size_t N = numel.size();
  if (p.size() != N || g.size() != N) throw std::runtime_error("optimizer kernel: list length mismatch");
  if ((!s1.empty() && s1.size() != N) || (!s2.empty() && s2.size() != N) || (!s3.empty() && s3.size() != N) ||
      (!w.empty() && w.size() != N))
    throw std::runtime_error("optimizer kernel: state list length mismatch");
  OptArgs a{};
  int n = 0;
  int32_t blocks = 0;
  int64_t pbase = 0;
  auto flush = [&]() {
    if (n == 0) return;
    a.n = n;
    a.start[n] = blocks;
    a.pbase = pbase;
    launch(a, blocks);
    pbase += blocks;
    a = OptArgs{};
    n = 0;
    blocks = 0;
  };
  for (size_t i = 0; i < N; ++i) {
    if (numel[i] <= 0) continue;
    const int64_t nb = (numel[i] + kChunk - 1) / kChunk;
    if (n == kMaxT || int64_t(blocks) + nb > (int64_t(1) << 30)) flush();
    a.p[n] = p[i];
    a.g[n] = g[i];
    a.s1[n] = s1.empty() ? 0 : s1[i];
    a.s2[n] = s2.empty() ? 0 : s2[i];
    a.s3[n] = s3.empty() ? 0 : s3[i];
    a.w[n] = w.empty() ? 0 : w[i];
    a.numel[n] = numel[i];
    a.tidx[n] = static_cast<int32_t>(i);
    a.start[n] = blocks;
    blocks += static_cast<int32_t>(nb);
    ++n;
  }
  flush();
}

template <typename T> constexpr int code_of();
template <> constexpr int code_of<float>() { return kF32; }
template <> constexpr int code_of<bf16>() { return kBF16; }
template <> constexpr int code_of<f16>() { return kF16; }
template <> constexpr int code_of<double>() { return kF64; }

// (parameter, gradient, state, fp32 master) combinations of the update kernels
#define OPT_DTYPE_COMBOS(COMBO)            \
  COMBO(float, float, float, false)        \
  COMBO(float, bf16, float, false)         \
  COMBO(bf16, bf16, bf16, false)           \
  COMBO(bf16, bf16, float, false)          \
  COMBO(bf16, bf16, float, true)           \
  COMBO(bf16, float, float, true)          \
  COMBO(f16, f16, f16, false)              \
  COMBO(f16, f16, float, false)            \
  COMBO(f16, f16, float, true)             \
  COMBO(f16, float, float, true)           \
  COMBO(double, double, double, false)

// Runtime dtype codes -> one of the combinations above, in the style of common.h's dispatchers:
// f(TypeTag<P>, TypeTag<G>, TypeTag<S>, std::bool_constant<MASTER>) names the launch once. Any
// other combination throws "<what>: unsupported dtype combination p= g= s= master=".
template <typename F>
void dispatch_opt_combo(int p_dtype, int g_dtype, int s_dtype, bool has_master, const char* what, F&& f) {
#define X(P, G, S, M)                                                                                     \
  if (p_dtype == code_of<P>() && g_dtype == code_of<G>() && s_dtype == code_of<S>() && has_master == M) \
    return f(TypeTag<P>{}, TypeTag<G>{}, TypeTag<S>{}, std::bool_constant<M>{});
  OPT_DTYPE_COMBOS(X)
#undef X
  throw std::runtime_error(std::string(what) + ": unsupported dtype combination p=" + std::to_string(p_dtype) +
                           " g=" + std::to_string(g_dtype) + " s=" + std::to_string(s_dtype) +
                           " master=" + std::to_string(has_master));
}

// The layer-wise rules (optim_layerwise.hip: kLars, kLamb) behind mt_rule's entry. s3 carries each
// leaf's address in the partials workspace (2 entries per 4096-element chunk, in compute precision)
// and RuleHyper::tscale is written: the trust ratio each leaf used. LARS: beta1 = rho, beta2 = trust.
void mt_layerwise(const std::vector<uintptr_t>& param, const std::vector<uintptr_t>& grad,
                  const std::vector<uintptr_t>& s1, const std::vector<uintptr_t>& s2,
                  const std::vector<uintptr_t>& s3, const std::vector<uintptr_t>& master,
                  const std::vector<int64_t>& numel, int p_dtype, int g_dtype, int s_dtype, const RuleHyper& h,
                  hipStream_t stream);

}  // namespace fluxmpi
