// Fused multi-tensor steps for the rest of the Optimisers.jl rule set: RMSProp, AdaGrad, Lion,
// AdaMax, AMSGrad, NAdam, AdaBelief, AdaDelta. One generic kernel in the job layout of
// mt_adam_kernel (optim_common.h), parameterised by a per-element functor: one pass reads the
// gradient, the parameter (or its fp32 master) and the rule's one to three state tensors and
// writes them back once.
//
// Every element goes through the same prologue and epilogue, in compute precision (fp32 math for
// bf16 / fp16 / fp32 leaves, fp64 for fp64):
//   g  = clamp(g_in * grad_scale [* dev_gscale] [* tscale[leaf]], -delta, delta)
//   dx = rule(g, state...)            (the table below; the state is updated on the way)
//   if (wd) dx += wd * x ; x -= dx    (an OptimiserChain(rule, WeightDecay(wd)))
//
//   RMSProp:   acc = rho*acc + (1-rho)*g^2 ;                 dx = g*lr / (sqrt(acc) + eps)
//   AdaGrad:   acc += g^2 ;                                   dx = g*lr / (sqrt(acc) + eps)
//   Lion:      dx = lr * sign(b1*m + (1-b1)*g) ;              m = b2*m + (1-b2)*g   (sign(0) = 0)
//   AdaMax:    m = b1*m + (1-b1)*g ; u = max(b2*u, |g|) ;     dx = lr/(1-b1^t) * m / (u + eps)
//   AMSGrad:   m, v as Adam ; vh = max(vh, v) ;               dx = lr * m / (sqrt(vh) + eps)
//   NAdam:     m, v as Adam ;
//              dx = (b1*m/(1-b1*b1^t) + (1-b1)*g/(1-b1^t)) / (sqrt(v*b2/(1-b2^t)) + eps) * lr
//   AdaBelief: m as Adam ; s = b2*s + (1-b2)*(g-m)^2 + eps ;  dx = lr*m/(1-b1^t) / (sqrt(s/(1-b2^t)) + eps)
//   AdaDelta:  acc = rho*acc + (1-rho)*g^2 ; dx = g*sqrt(D+eps)/sqrt(acc+eps) ; D = rho*D + (1-rho)*dx^2
//
// lr, b1^t and b2^t come from the host arguments or, when given, from the device block
// {lr, b1^t, b2^t} ({lr} for the rules without bias correction): Adam's scheme, advanced by
// adam_advance, so a captured graph replays correct steps. No atomics, no LDS. With
// RuleHyper::dev_skip (loss scaling) a workgroup first reads that one device word and, when it is
// set, returns before it touches any tensor.
#include <stdexcept>
#include <string>
#include <vector>

#include "../api.h"
#include "optim_common.h"
#include "optim_sr.h"

namespace fluxmpi {
namespace {

// max with torch.maximum's NaN behaviour (either operand NaN -> NaN)
template <typename C>
__device__ __forceinline__ C nan_max(C a, C b) {
  return a != a ? a : (b != b ? b : (a > b ? a : b));
}

// The step's scalars in compute precision. bt1 / bt2: beta1^t / beta2^t.
template <typename C>
struct RuleScalars {
  C lr, b1, b2, eps, bt1, bt2;
};

// Rule functors: dx = op(g, s1, s2, s3) and the new state. kStates: state tensors the rule
// keeps; kBt: it reads beta^t (bias correction). No fp contraction in any element functor of the
// optimiser kernels: which product of a*b + c*d the compiler fused differed between the vector and
// the scalar path of one kernel (Lion fp32: a packed fma against two multiplies and an add), so a
// leaf's bits depended on its alignment. As written, both paths round alike.
template <typename C>
struct RmsPropRule {
  static constexpr int kStates = 1;
  static constexpr bool kBt = false;
  RuleScalars<C> h;
  __device__ __forceinline__ C operator()(C g, C& acc, C&, C&) const {
#pragma clang fp contract(off)
    acc = h.b1 * acc + (C(1) - h.b1) * (g * g);
    return g * h.lr / (sqrt(acc) + h.eps);
  }
};

template <typename C>
struct AdaGradRule {
  static constexpr int kStates = 1;
  static constexpr bool kBt = false;
  RuleScalars<C> h;
  __device__ __forceinline__ C operator()(C g, C& acc, C&, C&) const {
#pragma clang fp contract(off)
    acc = acc + g * g;
    return g * h.lr / (sqrt(acc) + h.eps);
  }
};

template <typename C>
struct LionRule {
  static constexpr int kStates = 1;
  static constexpr bool kBt = false;
  RuleScalars<C> h;
  __device__ __forceinline__ C operator()(C g, C& m, C&, C&) const {
#pragma clang fp contract(off)
    const C a = h.b1 * m + (C(1) - h.b1) * g;
    m = h.b2 * m + (C(1) - h.b2) * g;
    // torch.sign: 0 -> 0, NaN -> NaN (a * 0 keeps the NaN)
    const C s = a > C(0) ? C(1) : (a < C(0) ? C(-1) : a * C(0));
    return h.lr * s;
  }
};

template <typename C>
struct AdaMaxRule {
  static constexpr int kStates = 2;
  static constexpr bool kBt = true;
  RuleScalars<C> h;
  __device__ __forceinline__ C operator()(C g, C& m, C& u, C&) const {
#pragma clang fp contract(off)
    m = h.b1 * m + (C(1) - h.b1) * g;
    u = nan_max(h.b2 * u, g < C(0) ? -g : g);
    return h.lr / (C(1) - h.bt1) * m / (u + h.eps);
  }
};

template <typename C>
struct AmsGradRule {
  static constexpr int kStates = 3;
  static constexpr bool kBt = false;
  RuleScalars<C> h;
  __device__ __forceinline__ C operator()(C g, C& m, C& v, C& vh) const {
#pragma clang fp contract(off)
    m = h.b1 * m + (C(1) - h.b1) * g;
    v = h.b2 * v + (C(1) - h.b2) * (g * g);
    vh = nan_max(vh, v);
    return h.lr * m / (sqrt(vh) + h.eps);
  }
};

template <typename C>
struct NAdamRule {
  static constexpr int kStates = 2;
  static constexpr bool kBt = true;
  RuleScalars<C> h;
  __device__ __forceinline__ C operator()(C g, C& m, C& v, C&) const {
#pragma clang fp contract(off)
    m = h.b1 * m + (C(1) - h.b1) * g;
    v = h.b2 * v + (C(1) - h.b2) * (g * g);
    const C num = h.b1 * m / (C(1) - h.b1 * h.bt1) + (C(1) - h.b1) * g / (C(1) - h.bt1);
    return num / (sqrt(v * h.b2 / (C(1) - h.bt2)) + h.eps) * h.lr;
  }
};

template <typename C>
struct AdaBeliefRule {
  static constexpr int kStates = 2;
  static constexpr bool kBt = true;
  RuleScalars<C> h;
  __device__ __forceinline__ C operator()(C g, C& m, C& s, C&) const {
#pragma clang fp contract(off)
    m = h.b1 * m + (C(1) - h.b1) * g;
    const C d = g - m;
    s = h.b2 * s + (C(1) - h.b2) * (d * d) + h.eps;
    return h.lr * m / (C(1) - h.bt1) / (sqrt(s / (C(1) - h.bt2)) + h.eps);
  }
};

template <typename C>
struct AdaDeltaRule {
  static constexpr int kStates = 2;
  static constexpr bool kBt = false;
  RuleScalars<C> h;
  __device__ __forceinline__ C operator()(C g, C& acc, C& delta, C&) const {
#pragma clang fp contract(off)
    acc = h.b1 * acc + (C(1) - h.b1) * (g * g);
    const C dx = g * sqrt(delta + h.eps) / sqrt(acc + h.eps);
    delta = h.b1 * delta + (C(1) - h.b1) * (dx * dx);
    return dx;
  }
};

// prologue + rule + epilogue of one element; the state tensors beyond R::kStates are not touched
template <typename R, typename P, typename G, typename S, bool MASTER>
struct RuleElem {
  using C = typename Comp<P>::type;
  R rule;
  C wd, gs, ts, delta;
  // rnd: the stores' rounding policy (optim_sr.h), slot 0 the parameter, 1..3 the states
  template <typename Rnd>
  __device__ __forceinline__ void operator()(P& p, G g_in, S& a_io, S& b_io, S& c_io, float& w,
                                             const Rnd& rnd) const {
#pragma clang fp contract(off)
    const C g = clip_grad(static_cast<C>(g_in) * gs * ts, delta);
    C a = static_cast<C>(a_io);
    C b = R::kStates > 1 ? static_cast<C>(b_io) : C(0);
    C c = R::kStates > 2 ? static_cast<C>(c_io) : C(0);
    C x = MASTER ? static_cast<C>(w) : static_cast<C>(p);
    C dx = rule(g, a, b, c);
    if (wd != C(0)) dx += wd * x;
    x -= dx;
    a_io = rnd.template cast<S>(a, 1);
    if (R::kStates > 1) b_io = rnd.template cast<S>(b, 2);
    if (R::kStates > 2) c_io = rnd.template cast<S>(c, 3);
    if (MASTER) w = static_cast<float>(x);
    p = rnd.template cast<P>(x, 0);
  }
};

// Sr: empty (round to nearest: the kernel and its arguments are what they were without the pack), or
// one SrArgs (optim_sr.h), a third kernel parameter that only the stochastic-rounding instantiations take.
template <template <typename> class RuleT, typename P, typename G, typename S, bool MASTER, bool SKIP,
          typename... Sr>
__global__ __launch_bounds__(kThreads) void mt_rule_kernel(OptArgs a, RuleHyper h, Sr... sr) {
  using C = typename Comp<P>::type;
  if (step_skipped<SKIP>(h.dev_skip)) return;
  using R = RuleT<C>;
  constexpr int NS = R::kStates;
  const Chunk ch = chunk_of(a);
  const int t = ch.t;
  const SrCtx<sizeof...(Sr) != 0> rc(t, sr...);
  constexpr int kSrStates = std::is_same_v<S, bf16> ? NS : 0;

  RuleElem<R, P, G, S, MASTER> op;
  C lr = static_cast<C>(h.lr), bt1 = static_cast<C>(h.bt1), bt2 = static_cast<C>(h.bt2);
  if (h.dev != nullptr) {  // graph mode: step-dependent scalars live on the device
    lr = static_cast<C>(h.dev[0]);
    if (R::kBt) {  // the block has beta^t entries only for the rules that read them
      bt1 = static_cast<C>(h.dev[1]);
      bt2 = static_cast<C>(h.dev[2]);
    }
  }
  op.rule.h.lr = lr; op.rule.h.bt1 = bt1; op.rule.h.bt2 = bt2;
  op.rule.h.b1 = static_cast<C>(h.beta1); op.rule.h.b2 = static_cast<C>(h.beta2);
  op.rule.h.eps = static_cast<C>(h.eps);
  op.wd = static_cast<C>(h.weight_decay);
  op.gs = static_cast<C>(h.grad_scale) * (h.dev_gscale ? static_cast<C>(*h.dev_gscale) : C(1));
  op.ts = h.tscale ? static_cast<const C*>(h.tscale)[a.tidx[t]] : C(1);
  op.delta = h.clip_delta;

  P* __restrict__ p = reinterpret_cast<P*>(a.p[t]);
  const G* __restrict__ g = reinterpret_cast<const G*>(a.g[t]);
  S* __restrict__ s1 = reinterpret_cast<S*>(a.s1[t]);
  S* __restrict__ s2 = reinterpret_cast<S*>(a.s2[t]);
  S* __restrict__ s3 = reinterpret_cast<S*>(a.s3[t]);
  float* __restrict__ w = reinterpret_cast<float*>(a.w[t]);
  const int tid = threadIdx.x;
  const bool vec = aligned16(p) && aligned16(g) && aligned16(s1) && (NS < 2 || aligned16(s2)) &&
                   (NS < 3 || aligned16(s3)) && (!MASTER || aligned16(w)) && rc.vec_ok();
  int64_t scalar_from = ch.base;
  if (vec) {
    const int64_t nvec = (ch.end - ch.base) / kVec;
#pragma unroll
    for (int k = 0; k < kIters; ++k) {
      const int64_t vi = tid + k * kThreads;
      if (vi < nvec) {
        const int64_t off = ch.base + vi * kVec;
        P pv[kVec]; G gv[kVec]; S av[kVec]; S bv[kVec]; S cv[kVec]; float wv[kVec];
        load8(g + off, gv);
        load8(s1 + off, av);
        if (NS > 1) load8(s2 + off, bv);
        if (NS > 2) load8(s3 + off, cv);
        if (MASTER) load8(w + off, wv); else load8(p + off, pv);
        const auto rv = rc.vec(off, kSrStates);
#pragma unroll
        for (int j = 0; j < kVec; ++j) op(pv[j], gv[j], av[j], bv[j], cv[j], wv[j], rv.at(j));
        store8(s1 + off, av);
        if (NS > 1) store8(s2 + off, bv);
        if (NS > 2) store8(s3 + off, cv);
        if (MASTER) store8(w + off, wv);
        store8(p + off, pv);
      }
    }
    scalar_from = ch.base + nvec * kVec;
  }
  for (int64_t i = scalar_from + tid; i < ch.end; i += kThreads) {
    P pv = p[i];
    S av = s1[i];
    S bv = NS > 1 ? s2[i] : S(0);
    S cv = NS > 2 ? s3[i] : S(0);
    float wv = MASTER ? w[i] : 0.f;
    op(pv, g[i], av, bv, cv, wv, rc.one(i, kSrStates));
    s1[i] = av;
    if (NS > 1) s2[i] = bv;
    if (NS > 2) s3[i] = cv;
    if (MASTER) w[i] = wv;
    p[i] = pv;
  }
}


template <template <typename> class RuleT>
void launch_rule(const std::vector<uintptr_t>& param, const std::vector<uintptr_t>& grad,
                 const std::vector<uintptr_t>& s1, const std::vector<uintptr_t>& s2,
                 const std::vector<uintptr_t>& s3, const std::vector<uintptr_t>& master,
                 const std::vector<int64_t>& numel, int p_dtype, int g_dtype, int s_dtype, const RuleHyper& h,
                 hipStream_t stream, const SrHyper* sr) {
  constexpr int NS = RuleT<float>::kStates;
  const size_t N = numel.size();
  // every state tensor the kernel dereferences must be there: a missing list would be a null pointer
  if (s1.size() != N || (NS > 1 && s2.size() != N) || (NS > 2 && s3.size() != N))
    throw std::runtime_error("mt_rule: rule " + std::to_string(h.kind) + " needs " + std::to_string(NS) +
                             " state list(s) as long as the parameter list");
  const bool has_master = !master.empty();
  if (sr != nullptr) sr_check_combo(*sr, N, p_dtype, g_dtype, s_dtype, has_master, "mt_rule");
  for_each_group(param, grad, s1, s2, s3, master, numel, [&](const OptArgs& a, int blocks) {
    if (sr != nullptr) {
      const SrArgs sa = sr_args_for(*sr, a);
      dispatch_bool(s_dtype == kBF16, [&](auto sb) {
        dispatch_bool(h.dev_skip != nullptr, [&](auto skip) {
          using S = std::conditional_t<decltype(sb)::value, bf16, float>;
          mt_rule_kernel<RuleT, bf16, bf16, S, false, decltype(skip)::value, SrArgs><<<blocks, kThreads, 0, stream>>>(a, h, sa);
        });
      });
      FLUXMPI_HIP_CHECK(hipGetLastError());
      return;
    }
    dispatch_opt_combo(p_dtype, g_dtype, s_dtype, has_master, "mt_rule", [&](auto p, auto g, auto s, auto master) {
      dispatch_bool(h.dev_skip != nullptr, [&](auto skip) {
        mt_rule_kernel<RuleT, typename decltype(p)::type, typename decltype(g)::type, typename decltype(s)::type,
                       decltype(master)::value, decltype(skip)::value><<<blocks, kThreads, 0, stream>>>(a, h);
      });
    });
    FLUXMPI_HIP_CHECK(hipGetLastError());
  });
}

}  // namespace

void mt_rule(const std::vector<uintptr_t>& param, const std::vector<uintptr_t>& grad,
             const std::vector<uintptr_t>& s1, const std::vector<uintptr_t>& s2,
             const std::vector<uintptr_t>& s3, const std::vector<uintptr_t>& master,
             const std::vector<int64_t>& numel, int p_dtype, int g_dtype, int s_dtype, const RuleHyper& h,
             hipStream_t stream, const SrHyper* sr) {
  if (sr != nullptr && (h.kind == kLars || h.kind == kLamb))
    throw std::runtime_error("mt_rule: LARS / LAMB have no stochastic-rounding kernels");
#define RULE(K, T) \
  case K: launch_rule<T>(param, grad, s1, s2, s3, master, numel, p_dtype, g_dtype, s_dtype, h, stream, sr); break;
  switch (h.kind) {
    RULE(kRmsProp, RmsPropRule)
    RULE(kAdaGrad, AdaGradRule)
    RULE(kLion, LionRule)
    RULE(kAdaMax, AdaMaxRule)
    RULE(kAmsGrad, AmsGradRule)
    RULE(kNAdam, NAdamRule)
    RULE(kAdaBelief, AdaBeliefRule)
    RULE(kAdaDelta, AdaDeltaRule)
    case kLars:
    case kLamb: mt_layerwise(param, grad, s1, s2, s3, master, numel, p_dtype, g_dtype, s_dtype, h, stream); break;
    default: throw std::runtime_error("mt_rule: unknown rule " + std::to_string(h.kind));
  }
#undef RULE
}

}  // namespace fluxmpi
