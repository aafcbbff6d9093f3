// Fused multi-tensor optimiser steps for gfx950 (K3/K4 of SURVEY §2.4).
//
// The reference delegates to Optimisers.jl, i.e. one broadcast kernel per
// expression per leaf (src/optimizer.jl:22). Adam alone is ~4 passes over
// g, x, m, v per leaf. Here one launch updates every leaf of a bucket in a
// single pass: read g, x (or the fp32 master), m, v once; write x, m, v once.
//
// Numerics follow Optimisers.jl exactly, in the element type's precision
// (fp32 math for bf16/fp16/fp32, fp64 math for fp64):
//   Adam:     m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g^2
//             dx = m / (1-b1^t) / (sqrt(v / (1-b2^t)) + eps) * lr   [+ wd*x: AdamW chain]
//             x -= dx
//   Descent:  x -= lr*g
//   Momentum: v = rho*v + lr*g ; x -= v
//   Nesterov: dx = -rho^2*v + (1+rho)*lr*g ; v = rho*v - lr*g ; x -= dx
// Every rule first forms its gradient, in compute precision, as
//   g = clamp(g_in * grad_scale [* dev_gscale] [* tscale[leaf]], -delta, delta)   (delta == 0: no clamp)
// (grad_scale: host, e.g. 1/world; dev_gscale: one device scalar, the global-norm clip;
// tscale: one device scalar per leaf of the call, the ClipNorm chain; delta: ClipGrad).
//
// Gradient clipping needs norms first: mt_leaf_sumsq is a deterministic two-launch multi-tensor
// sum of squares (one partial per 4096-element workgroup, then one workgroup per leaf reduces
// that leaf's partials in a fixed order — no float atomics, so two runs agree bit for bit) whose
// finish also writes the per-leaf scale min(1, omega / (grad_scale * sqrt(sumsq))); clip_total
// folds the per-leaf sums into one device slot {sum, norm, scale} for global-norm clipping.
// Nothing is read back to the host: the whole sequence is HIP-graph capturable.
//
// Loss scaling (DDP(loss_scale=...)) lives here too: mt_check_finite, the exact per-element inf / NaN
// test into one sticky int32 flag (also the CHECK instantiation of the sum-of-squares pass, so an
// engine that takes norms reads its gradients once); AdamHyper / SgdHyper::dev_skip, on which a
// workgroup returns before it touches a tensor (a template flag: without it the kernels are the
// code they were); dev_pre, the inverse scale multiplied into the norms; and loss_scale_update,
// GradScaler's rule on the scaler's device block, one thread.
//
// Optional fp32 master weights give the mixed-precision layout (bf16 param +
// fp32 master/m/v); without them the state dtype equals the parameter dtype,
// which is Optimisers.jl's `zero(x)` layout (bit-compatible state trees).
#include <stdexcept>
#include <string>
#include <vector>

#include "../api.h"
#include "optim_common.h"
#include "optim_sr.h"

namespace fluxmpi {
namespace {

template <typename P, typename G, typename S, bool MASTER>
struct AdamElem {
  using C = typename Comp<P>::type;
  C lr, b1, b2, eps, bc1, bc2, wd, gs, ts, delta;
  // rnd: the stores' rounding policy (optim_sr.h), slot 0 the parameter, 1 / 2 the moments
  template <typename Rnd>
  __device__ __forceinline__ void operator()(P& p, G g_in, S& m_io, S& v_io, float& w, const Rnd& rnd) const {
#pragma clang fp contract(off)  // as written: see the note above the rule functors of optim_rules.hip
    const C g = clip_grad(static_cast<C>(g_in) * gs * ts, delta);
    const C m = b1 * static_cast<C>(m_io) + (C(1) - b1) * g;
    const C v = b2 * static_cast<C>(v_io) + (C(1) - b2) * (g * g);
    C x = MASTER ? static_cast<C>(w) : static_cast<C>(p);
    C dx = m / bc1 / (sqrt(v / bc2) + eps) * lr;
    if (wd != C(0)) dx += wd * x;
    x -= dx;
    m_io = rnd.template cast<S>(m, 1);
    v_io = rnd.template cast<S>(v, 2);
    if (MASTER) w = static_cast<float>(x);
    p = rnd.template cast<P>(x, 0);
  }
};

// Sr: empty (round to nearest: the kernel and its arguments are what they were without the pack), or
// one SrArgs, a third kernel parameter that only the stochastic-rounding instantiations take.
template <typename P, typename G, typename S, bool MASTER, bool SKIP, typename... Sr>
__global__ __launch_bounds__(kThreads) void mt_adam_kernel(OptArgs a, AdamHyper h, Sr... sr) {
  using C = typename Comp<P>::type;
  if (step_skipped<SKIP>(h.dev_skip)) return;
  const Chunk ch = chunk_of(a);
  const int t = ch.t;
  const SrCtx<sizeof...(Sr) != 0> rc(t, sr...);
  constexpr int kSrStates = std::is_same_v<S, bf16> ? 2 : 0;

  AdamElem<P, G, S, MASTER> op;
  C lr = static_cast<C>(h.lr), bc1 = static_cast<C>(h.bc1), bc2 = static_cast<C>(h.bc2);
  if (h.dev != nullptr) {  // graph mode: step-dependent scalars live on the device
    lr = static_cast<C>(h.dev[0]);
    bc1 = C(1) - static_cast<C>(h.dev[1]);
    bc2 = C(1) - static_cast<C>(h.dev[2]);
  }
  op.lr = lr; op.bc1 = bc1; op.bc2 = bc2;
  op.b1 = static_cast<C>(h.beta1); op.b2 = static_cast<C>(h.beta2); op.eps = static_cast<C>(h.eps);
  op.wd = static_cast<C>(h.weight_decay);
  op.gs = static_cast<C>(h.grad_scale) * (h.dev_gscale ? static_cast<C>(*h.dev_gscale) : C(1));
  op.ts = h.tscale ? static_cast<const C*>(h.tscale)[a.tidx[t]] : C(1);
  op.delta = h.clip_delta;

  P* __restrict__ p = reinterpret_cast<P*>(a.p[t]);
  const G* __restrict__ g = reinterpret_cast<const G*>(a.g[t]);
  S* __restrict__ m = reinterpret_cast<S*>(a.s1[t]);
  S* __restrict__ v = reinterpret_cast<S*>(a.s2[t]);
  float* __restrict__ w = reinterpret_cast<float*>(a.w[t]);
  const int tid = threadIdx.x;
  const bool vec = aligned16(p) && aligned16(g) && aligned16(m) && aligned16(v) && (!MASTER || aligned16(w)) &&
                   rc.vec_ok();
  int64_t scalar_from = ch.base;
  if (vec) {
    const int64_t nvec = (ch.end - ch.base) / kVec;
#pragma unroll
    for (int k = 0; k < kIters; ++k) {
      const int64_t vi = tid + k * kThreads;
      if (vi < nvec) {
        const int64_t off = ch.base + vi * kVec;
        P pv[kVec]; G gv[kVec]; S mv[kVec]; S vv[kVec]; float wv[kVec];
        load8(g + off, gv);
        load8(m + off, mv);
        load8(v + off, vv);
        if (MASTER) load8(w + off, wv); else load8(p + off, pv);
        const auto rv = rc.vec(off, kSrStates);
#pragma unroll
        for (int j = 0; j < kVec; ++j) op(pv[j], gv[j], mv[j], vv[j], wv[j], rv.at(j));
        store8(m + off, mv);
        store8(v + off, vv);
        if (MASTER) store8(w + off, wv);
        store8(p + off, pv);
      }
    }
    scalar_from = ch.base + nvec * kVec;
  }
  for (int64_t i = scalar_from + tid; i < ch.end; i += kThreads) {
    P pv = p[i];
    S mv = m[i], vv = v[i];
    float wv = MASTER ? w[i] : 0.f;
    op(pv, g[i], mv, vv, wv, rc.one(i, kSrStates));
    m[i] = mv; v[i] = vv;
    if (MASTER) w[i] = wv;
    p[i] = pv;
  }
}


template <typename P, typename G, typename S, bool MASTER>
struct SgdElem {
  using C = typename Comp<P>::type;
  C lr, rho, wd, gs, ts, delta;
  int mode;  // 0 descent, 1 momentum, 2 nesterov
  template <typename Rnd>
  __device__ __forceinline__ void operator()(P& p, G g_in, S& buf, float& w, const Rnd& rnd) const {
#pragma clang fp contract(off)
    C x = MASTER ? static_cast<C>(w) : static_cast<C>(p);
    C g = clip_grad(static_cast<C>(g_in) * gs * ts, delta);
    if (wd != C(0)) g += wd * x;
    C dx;
    if (mode == 0) {
      dx = g * lr;
    } else if (mode == 1) {
      const C vel = rho * static_cast<C>(buf) + lr * g;
      buf = rnd.template cast<S>(vel, 1);
      dx = vel;
    } else {
      const C vel0 = static_cast<C>(buf);
      dx = -(rho * rho) * vel0 + (C(1) + rho) * lr * g;
      buf = rnd.template cast<S>(rho * vel0 - lr * g, 1);
    }
    x -= dx;
    if (MASTER) w = static_cast<float>(x);
    p = rnd.template cast<P>(x, 0);
  }
};

template <typename P, typename G, typename S, bool MASTER, bool SKIP, typename... Sr>  // Sr: as in mt_adam_kernel
__global__ __launch_bounds__(kThreads) void mt_sgd_kernel(OptArgs a, SgdHyper h, Sr... sr) {
  using C = typename Comp<P>::type;
  if (step_skipped<SKIP>(h.dev_skip)) return;
  const Chunk ch = chunk_of(a);
  const int t = ch.t;
  const SrCtx<sizeof...(Sr) != 0> rc(t, sr...);
  SgdElem<P, G, S, MASTER> op;
  op.lr = h.dev_lr ? static_cast<C>(*h.dev_lr) : static_cast<C>(h.lr);
  op.rho = static_cast<C>(h.momentum); op.wd = static_cast<C>(h.weight_decay);
  op.gs = static_cast<C>(h.grad_scale) * (h.dev_gscale ? static_cast<C>(*h.dev_gscale) : C(1));
  op.ts = h.tscale ? static_cast<const C*>(h.tscale)[a.tidx[t]] : C(1);
  op.delta = h.clip_delta;
  op.mode = h.momentum == 0. ? 0 : (h.nesterov ? 2 : 1);
  P* __restrict__ p = reinterpret_cast<P*>(a.p[t]);
  const G* __restrict__ g = reinterpret_cast<const G*>(a.g[t]);
  S* __restrict__ buf = reinterpret_cast<S*>(a.s1[t]);
  float* __restrict__ w = reinterpret_cast<float*>(a.w[t]);
  const bool has_buf = op.mode != 0;
  const int tid = threadIdx.x;
  const bool vec = aligned16(p) && aligned16(g) && (!has_buf || aligned16(buf)) && (!MASTER || aligned16(w)) &&
                   rc.vec_ok();
  const int sr_states = std::is_same_v<S, bf16> && has_buf ? 1 : 0;
  int64_t scalar_from = ch.base;
  if (vec) {
    const int64_t nvec = (ch.end - ch.base) / kVec;
#pragma unroll
    for (int k = 0; k < kIters; ++k) {
      const int64_t vi = tid + k * kThreads;
      if (vi < nvec) {
        const int64_t off = ch.base + vi * kVec;
        P pv[kVec]; G gv[kVec]; S bv[kVec]; float wv[kVec];
        load8(g + off, gv);
        if (has_buf) load8(buf + off, bv);
        if (MASTER) load8(w + off, wv); else load8(p + off, pv);
        const auto rv = rc.vec(off, sr_states);
#pragma unroll
        for (int j = 0; j < kVec; ++j) op(pv[j], gv[j], bv[j], wv[j], rv.at(j));
        if (has_buf) store8(buf + off, bv);
        if (MASTER) store8(w + off, wv);
        store8(p + off, pv);
      }
    }
    scalar_from = ch.base + nvec * kVec;
  }
  for (int64_t i = scalar_from + tid; i < ch.end; i += kThreads) {
    P pv = p[i];
    S bv = has_buf ? buf[i] : S(0);
    float wv = MASTER ? w[i] : 0.f;
    op(pv, g[i], bv, wv, rc.one(i, sr_states));
    if (has_buf) buf[i] = bv;
    if (MASTER) w[i] = wv;
    p[i] = pv;
  }
}


// ---- deterministic multi-tensor sum of squares + clip scales -------------------------------
// launch 1: the job layout of the update kernels; workgroup b writes partials[pbase + b].
// CHECK: the pass also tests every element it reads for inf / NaN and raises flag[0] (loss scaling:
// no second read of the gradients); the sums are the bits of CHECK == false.
template <typename G, bool CHECK>
__global__ __launch_bounds__(kThreads) void mt_sumsq_partial_kernel(OptArgs a, typename Acc<G>::type* __restrict__ partials,
                                                                     int32_t* __restrict__ flag) {
  using A = typename Acc<G>::type;
  const Chunk ch = chunk_of(a);
  const int t = ch.t;
  const G* __restrict__ g = reinterpret_cast<const G*>(a.g[t]);
  const int tid = threadIdx.x;
  A acc = A(0);
  bool bad = false;
  int64_t scalar_from = ch.base;
  if (aligned16(g)) {
    const int64_t nvec = (ch.end - ch.base) / kVec;
#pragma unroll
    for (int k = 0; k < kIters; ++k) {
      const int64_t vi = tid + k * kThreads;
      if (vi < nvec) {
        G gv[kVec];
        load8(g + ch.base + vi * kVec, gv);
#pragma unroll
        for (int j = 0; j < kVec; ++j) {
          const A x = static_cast<A>(gv[j]);
          acc += x * x;
          if (CHECK) bad |= nonfinite(gv[j]);
        }
      }
    }
    scalar_from = ch.base + nvec * kVec;
  }
  for (int64_t i = scalar_from + tid; i < ch.end; i += kThreads) {
    const G gi = g[i];
    const A x = static_cast<A>(gi);
    acc += x * x;
    if (CHECK) bad |= nonfinite(gi);
  }
  if (CHECK) note_found(bad);
  const A s = block_sum(acc);  // (its barrier is the block-wide OR's too)
  if (tid == 0) partials[a.pbase + static_cast<int>(blockIdx.x)] = s;
  if (CHECK) raise_noted(flag);
}

// the non-finite test alone, in the same job layout (an engine that takes no norms): one read of the
// gradients, nothing written but the flag
template <typename G>
__global__ __launch_bounds__(kThreads) void mt_check_finite_kernel(OptArgs a, int32_t* __restrict__ flag) {
  const Chunk ch = chunk_of(a);
  const G* __restrict__ g = reinterpret_cast<const G*>(a.g[ch.t]);
  const int tid = threadIdx.x;
  bool bad = false;
  int64_t scalar_from = ch.base;
  if (aligned16(g)) {
    const int64_t nvec = (ch.end - ch.base) / kVec;
#pragma unroll
    for (int k = 0; k < kIters; ++k) {
      const int64_t vi = tid + k * kThreads;
      if (vi < nvec) {
        G gv[kVec];
        load8(g + ch.base + vi * kVec, gv);
#pragma unroll
        for (int j = 0; j < kVec; ++j) bad |= nonfinite(gv[j]);
      }
    }
    scalar_from = ch.base + nvec * kVec;
  }
  for (int64_t i = scalar_from + tid; i < ch.end; i += kThreads) bad |= nonfinite(g[i]);
  note_found(bad);
  __syncthreads();
  raise_noted(flag);
}

// torch.clamp(omega / nrm, max=1): nrm 0 -> 1, nrm NaN -> NaN, nrm inf -> 0
template <typename A>
__device__ __forceinline__ A clip_scale(A omega, A nrm) {
  const A r = omega / nrm;
  return r > A(1) ? A(1) : r;
}

// launch 2: workgroup t adds leaf t's partials in a fixed order (thread i takes partials i,
// i + 256, ... in sequence, then block_sum) -> sumsq[leaf], scale[leaf]
template <typename A>
__global__ __launch_bounds__(kThreads) void mt_sumsq_finish_kernel(OptArgs a, const A* __restrict__ partials,
                                                                    A* __restrict__ sumsq, A* __restrict__ scale,
                                                                    float omega, float gs,
                                                                    const float* __restrict__ dev_pre) {
  const int t = blockIdx.x;
  const A* __restrict__ p = partials + a.pbase;
  A acc = A(0);
  for (int j = a.start[t] + threadIdx.x; j < a.start[t + 1]; j += kThreads) acc += p[j];
  const A s = block_sum(acc);
  if (threadIdx.x == 0) {
    const int leaf = a.tidx[t];
    sumsq[leaf] = s;
    if (scale != nullptr) {
      A nrm = static_cast<A>(gs) * sqrt(s);
      if (dev_pre != nullptr) nrm *= static_cast<A>(*dev_pre);  // the norm of the unscaled gradient
      scale[leaf] = clip_scale(static_cast<A>(omega), nrm);
    }
  }
}

// one workgroup: slot[0] = (accumulate ? slot[0] : 0) + sum_t sumsq[t] (fixed order),
// slot[1] = gs * sqrt(slot[0]) (the gradient norm), slot[2] = omega > 0 ? clip scale : 1; with
// dev_pre (the inverse loss scale) slot[1] and slot[2] are multiplied by it: the norm of the
// unscaled gradient, and the one device scalar that unscales and clips in the update kernels
template <typename A>
__global__ __launch_bounds__(kThreads) void clip_total_kernel(const A* __restrict__ sumsq, int64_t n,
                                                               float* __restrict__ slot, int accumulate,
                                                               float omega, float gs,
                                                               const float* __restrict__ dev_pre) {
  A acc = A(0);
  for (int64_t j = threadIdx.x; j < n; j += kThreads) acc += sumsq[j];
  const A s = block_sum(acc);
  if (threadIdx.x == 0) {
    const float total = (accumulate ? slot[0] : 0.f) + static_cast<float>(s);
    float nrm = gs * sqrtf(total);
    if (dev_pre != nullptr) nrm *= *dev_pre;
    const float cs = omega > 0.f ? clip_scale(omega, nrm) : 1.f;
    slot[0] = total;
    slot[1] = nrm;
    slot[2] = dev_pre != nullptr ? *dev_pre * cs : cs;
  }
}

__global__ void adam_advance_kernel(float* dev, float b1, float b2, const int32_t* dev_skip) {
  if (threadIdx.x == 0 && blockIdx.x == 0) {
    if (dev_skip != nullptr && *dev_skip != 0) return;  // a skipped step does not count
    dev[1] *= b1;
    dev[2] *= b2;
  }
}

// GradScaler's rule on the scaler's device block (api.h: loss_scale_update), one thread
__global__ void loss_scale_update_kernel(int32_t* __restrict__ blk, float growth, float backoff, int interval,
                                         float min_scale, float max_scale) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  float* f = reinterpret_cast<float*>(blk);
  float scale = f[0];
  int tracker = blk[2];
  const int flag = blk[5];
  if (flag != 0) {
    scale *= backoff;
    tracker = 0;
    blk[3] += 1;
  } else if (++tracker == interval) {
    scale *= growth;
    tracker = 0;
  }
  scale = fminf(fmaxf(scale, min_scale), max_scale);
  f[0] = scale;
  f[1] = 1.f / scale;
  blk[2] = tracker;
  blk[4] = flag != 0 ? 1 : 0;
  blk[5] = 0;
}

}  // namespace

void mt_adam(const std::vector<uintptr_t>& param, const std::vector<uintptr_t>& grad,
             const std::vector<uintptr_t>& m, const std::vector<uintptr_t>& v,
             const std::vector<uintptr_t>& master, const std::vector<int64_t>& numel,
             int p_dtype, int g_dtype, int s_dtype, const AdamHyper& h, hipStream_t stream, const SrHyper* sr) {
  const bool has_master = !master.empty();
  if (m.size() != numel.size() || v.size() != numel.size()) throw std::runtime_error("mt_adam: need m and v");
  if (sr != nullptr) sr_check_combo(*sr, numel.size(), p_dtype, g_dtype, s_dtype, has_master, "mt_adam");
  for_each_group(param, grad, m, v, {}, master, numel, [&](const OptArgs& a, int blocks) {
    if (sr != nullptr) {
      const SrArgs sa = sr_args_for(*sr, a);
      dispatch_bool(s_dtype == kBF16, [&](auto sb) {
        dispatch_bool(h.dev_skip != nullptr, [&](auto skip) {
          using S = std::conditional_t<decltype(sb)::value, bf16, float>;
          mt_adam_kernel<bf16, bf16, S, false, decltype(skip)::value, SrArgs><<<blocks, kThreads, 0, stream>>>(a, h, sa);
        });
      });
      FLUXMPI_HIP_CHECK(hipGetLastError());
      return;
    }
    dispatch_opt_combo(p_dtype, g_dtype, s_dtype, has_master, "mt_adam", [&](auto p, auto g, auto s, auto master) {
      dispatch_bool(h.dev_skip != nullptr, [&](auto skip) {
        mt_adam_kernel<typename decltype(p)::type, typename decltype(g)::type, typename decltype(s)::type,
                       decltype(master)::value, decltype(skip)::value><<<blocks, kThreads, 0, stream>>>(a, h);
      });
    });
    FLUXMPI_HIP_CHECK(hipGetLastError());
  });
}

void adam_advance(float* dev, float beta1, float beta2, hipStream_t stream, const int32_t* dev_skip) {
  adam_advance_kernel<<<1, 64, 0, stream>>>(dev, beta1, beta2, dev_skip);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

void mt_sgd(const std::vector<uintptr_t>& param, const std::vector<uintptr_t>& grad,
            const std::vector<uintptr_t>& buf, const std::vector<uintptr_t>& master,
            const std::vector<int64_t>& numel, int p_dtype, int g_dtype, int s_dtype,
            const SgdHyper& h, hipStream_t stream, const SrHyper* sr) {
  const bool has_master = !master.empty();
  if (h.momentum != 0. && buf.size() != numel.size())
    throw std::runtime_error("mt_sgd: momentum needs buffers");
  if (sr != nullptr) sr_check_combo(*sr, numel.size(), p_dtype, g_dtype, s_dtype, has_master, "mt_sgd");
  for_each_group(param, grad, buf, {}, {}, master, numel, [&](const OptArgs& a, int blocks) {
    if (sr != nullptr) {
      const SrArgs sa = sr_args_for(*sr, a);
      dispatch_bool(s_dtype == kBF16, [&](auto sb) {
        dispatch_bool(h.dev_skip != nullptr, [&](auto skip) {
          using S = std::conditional_t<decltype(sb)::value, bf16, float>;
          mt_sgd_kernel<bf16, bf16, S, false, decltype(skip)::value, SrArgs><<<blocks, kThreads, 0, stream>>>(a, h, sa);
        });
      });
      FLUXMPI_HIP_CHECK(hipGetLastError());
      return;
    }
    dispatch_opt_combo(p_dtype, g_dtype, s_dtype, has_master, "mt_sgd", [&](auto p, auto g, auto s, auto master) {
      dispatch_bool(h.dev_skip != nullptr, [&](auto skip) {
        mt_sgd_kernel<typename decltype(p)::type, typename decltype(g)::type, typename decltype(s)::type,
                      decltype(master)::value, decltype(skip)::value><<<blocks, kThreads, 0, stream>>>(a, h);
      });
    });
    FLUXMPI_HIP_CHECK(hipGetLastError());
  });
}

int64_t sumsq_partials(const std::vector<int64_t>& numel) {
  int64_t nb = 0;
  for (int64_t n : numel)
    if (n > 0) nb += (n + kChunk - 1) / kChunk;
  return nb;
}

namespace {
template <typename G>
void leaf_sumsq_impl(const std::vector<uintptr_t>& grad, const std::vector<int64_t>& numel, void* partials,
                     void* sumsq, void* scale, float omega, float grad_scale, hipStream_t stream,
                     int32_t* flag, const float* dev_pre) {
  using A = typename Acc<G>::type;
  bool empty = false;
  for (int64_t n : numel) empty = empty || n <= 0;
  if (empty) {
    // leaves without elements never reach a kernel: sum 0, scale 1 (memset nodes: capturable)
    FLUXMPI_HIP_CHECK(hipMemsetAsync(sumsq, 0, numel.size() * sizeof(A), stream));
    if (scale != nullptr) {
      const A one = A(1);
      for (size_t i = 0; i < numel.size(); ++i)
        if (numel[i] <= 0) {
          if constexpr (sizeof(A) == 4) {
            FLUXMPI_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(static_cast<A*>(scale) + i),
                                                __builtin_bit_cast(int, one), 1, stream));
          } else {  // 1.0 as two 32-bit words, low word first
            const uint64_t bits = __builtin_bit_cast(uint64_t, one);
            int* w = reinterpret_cast<int*>(static_cast<A*>(scale) + i);
            FLUXMPI_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(w), static_cast<int>(bits & 0xffffffffu), 1, stream));
            FLUXMPI_HIP_CHECK(hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(w + 1), static_cast<int>(bits >> 32), 1, stream));
          }
        }
    }
  }
  for_each_group(grad, grad, {}, {}, {}, {}, numel, [&](const OptArgs& a, int blocks) {
    dispatch_bool(flag != nullptr, [&](auto check) {
      mt_sumsq_partial_kernel<G, decltype(check)::value><<<blocks, kThreads, 0, stream>>>(a, static_cast<A*>(partials), flag);
    });
    FLUXMPI_HIP_CHECK(hipGetLastError());
    mt_sumsq_finish_kernel<A><<<a.n, kThreads, 0, stream>>>(a, static_cast<const A*>(partials), static_cast<A*>(sumsq),
                                                            static_cast<A*>(scale), omega, grad_scale, dev_pre);
    FLUXMPI_HIP_CHECK(hipGetLastError());
  });
}
}  // namespace

void mt_leaf_sumsq(const std::vector<uintptr_t>& grad, const std::vector<int64_t>& numel, int g_dtype,
                   void* partials, void* sumsq, void* scale, float omega, float grad_scale, hipStream_t stream,
                   int32_t* nonfinite_flag, const float* dev_pre) {
  dispatch_float64(
      g_dtype, [&] { return "mt_leaf_sumsq: unsupported gradient dtype " + std::to_string(g_dtype); }, [&](auto t) {
        leaf_sumsq_impl<typename decltype(t)::type>(grad, numel, partials, sumsq, scale, omega, grad_scale, stream,
                                                    nonfinite_flag, dev_pre);
      });
}

void mt_check_finite(const std::vector<uintptr_t>& grad, const std::vector<int64_t>& numel, int g_dtype,
                     int32_t* flag, hipStream_t stream) {
  if (flag == nullptr) throw std::runtime_error("mt_check_finite: needs the flag");
  dispatch_float64(
      g_dtype, [&] { return "mt_check_finite: unsupported gradient dtype " + std::to_string(g_dtype); }, [&](auto t) {
        for_each_group(grad, grad, {}, {}, {}, {}, numel, [&](const OptArgs& a, int blocks) {
          mt_check_finite_kernel<typename decltype(t)::type><<<blocks, kThreads, 0, stream>>>(a, flag);
          FLUXMPI_HIP_CHECK(hipGetLastError());
        });
      });
}

void loss_scale_update(void* block, float growth, float backoff, int interval, float min_scale, float max_scale,
                       hipStream_t stream) {
  if (block == nullptr) throw std::runtime_error("loss_scale_update: needs the scaler block");
  loss_scale_update_kernel<<<1, 64, 0, stream>>>(static_cast<int32_t*>(block), growth, backoff, interval, min_scale,
                                                 max_scale);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

void clip_total(const void* sumsq, int64_t n, int acc_dtype, float* slot, int accumulate, float omega,
                float grad_scale, hipStream_t stream, const float* dev_pre) {
  if (acc_dtype == kF32)
    clip_total_kernel<float><<<1, kThreads, 0, stream>>>(static_cast<const float*>(sumsq), n, slot, accumulate, omega,
                                                         grad_scale, dev_pre);
  else if (acc_dtype == kF64)
    clip_total_kernel<double><<<1, kThreads, 0, stream>>>(static_cast<const double*>(sumsq), n, slot, accumulate, omega,
                                                          grad_scale, dev_pre);
  else
    throw std::runtime_error("clip_total: sums are fp32 or fp64");
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace fluxmpi
