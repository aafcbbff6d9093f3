// Layer-wise adaptive rules on the fused multi-tensor layout (optim_common.h): LARS (You et al.
// 2017) and LAMB (You et al. 2020). The trust ratio of a leaf needs two norms over the whole leaf
// before its first element can be updated, so a step is two phases over the same job list, in
// compute precision (fp32 math for bf16 / fp16 / fp32 leaves, fp64 for fp64):
//
//   g = g_in * grad_scale [* dev_gscale]          x: the parameter (its fp32 master where there is one)
//
//   LARS   stats: workgroup partials of sum x^2 and sum g^2
//          apply: q = (|x| > 0 && |g| > 0) ? trust*|x| / (|g| + wd*|x| + eps) : 1
//                 vel = rho*vel + lr * q*(g + wd*x) ; x -= vel
//   LAMB   stats: m = b1*m + (1-b1)*g ; v = b2*v + (1-b2)*g^2 (written back, in the state's dtype);
//                 u = m/(1-b1^t) / (sqrt(v/(1-b2^t)) + eps) + wd*x from the STORED m, v;
//                 workgroup partials of sum x^2 and sum u^2
//          apply: q = (|x| > 0 && |u| > 0) ? |x| / |u| : 1 ; u again from m, v, x ; x -= lr*q*u
//
// stats: workgroup c of a leaf with nb chunks stores its two sums whole at part[c] and part[nb + c]
// (part: the leaf's 2*nb entries of the caller's workspace, its address riding in the s3 slot) —
// no atomics, no zero fill. The leaf's partials are then added in mt_sumsq_finish_kernel's fixed
// order (thread i takes partials i, i + 256, ... in sequence, then block_sum), so q is the same bit
// pattern in every workgroup, in every run and on every rank that holds the same replica. That
// fold is either the apply kernel's prologue (every workgroup of the leaf re-reads its 2*nb
// partials: one launch less) or, for groups with a leaf of more than kFoldLaunchChunks chunks, a
// launch of its own with one workgroup per leaf that leaves q in the ratio table for the apply
// kernel to read. The ratio each leaf used is written to ratio[tidx] (RuleHyper::tscale) either
// way. lr and beta^t come from the host arguments or the device block {lr[, b1^t, b2^t]}, as for
// Adam; nothing is read back, so a step is HIP-graph capturable. With RuleHyper::dev_skip (loss
// scaling) every workgroup of all three kernels first reads that one device word and, when it is set,
// returns: moments, velocity, parameters and the ratio table keep the previous step's values.
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../api.h"
#include "optim_common.h"

namespace fluxmpi {
namespace {

// a leaf with more chunks than this folds its partials in a launch of its own: in the prologue
// every workgroup re-reads 2*nb partials (8 nb bytes in fp32) beside the ~100 KB of its own chunk.
// Measured on one leaf (profiles/layerwise_fold_sweep.jsonl): the prologue is ~1 us ahead up to 2048
// chunks, level at 4096 (16.8M elements, 32 KB re-read) and 6 % / 11 % behind at 8192 / 16384
constexpr int kFoldLaunchChunks = 4096;

template <typename C>
struct LwScalars {
  C lr, b1, b2, eps, bc1, bc2, wd, gs, trust;  // b1: LARS' rho
};

template <typename C>
__device__ __forceinline__ LwScalars<C> lw_scalars(const RuleHyper& h, bool lamb) {
  LwScalars<C> s;
  C lr = static_cast<C>(h.lr), bt1 = static_cast<C>(h.bt1), bt2 = static_cast<C>(h.bt2);
  if (h.dev != nullptr) {  // graph mode: step-dependent scalars live on the device
    lr = static_cast<C>(h.dev[0]);
    if (lamb) {
      bt1 = static_cast<C>(h.dev[1]);
      bt2 = static_cast<C>(h.dev[2]);
    }
  }
  s.lr = lr; s.bc1 = C(1) - bt1; s.bc2 = C(1) - bt2;
  s.b1 = static_cast<C>(h.beta1); s.b2 = static_cast<C>(h.beta2); s.eps = static_cast<C>(h.eps);
  s.trust = static_cast<C>(h.beta2);
  s.wd = static_cast<C>(h.weight_decay);
  s.gs = static_cast<C>(h.grad_scale) * (h.dev_gscale ? static_cast<C>(*h.dev_gscale) : C(1));
  return s;
}

// LAMB's update direction from the stored moments (both phases call this on the same values)
template <typename C>
__device__ __forceinline__ C lamb_u(const LwScalars<C>& s, C m, C v, C x) {
#pragma clang fp contract(off)  // as written: see the note above the rule functors of optim_rules.hip
  C u = m / s.bc1 / (sqrt(v / s.bc2) + s.eps);
  if (s.wd != C(0)) u += s.wd * x;
  return u;
}

// the trust ratio from the leaf's sums of squares (sx: of x; sy: of g (LARS) / u (LAMB))
template <bool LAMB, typename C>
__device__ __forceinline__ C lw_ratio(const LwScalars<C>& s, C sx, C sy) {
#pragma clang fp contract(off)
  const C xn = sqrt(sx), yn = sqrt(sy);
  if (!(xn > C(0) && yn > C(0))) return C(1);
  return LAMB ? xn / yn : s.trust * xn / (yn + s.wd * xn + s.eps);
}

// the leaf's partials in the fixed order; both sums valid in every thread
template <typename A>
__device__ __forceinline__ void lw_fold(const A* __restrict__ part, int nb, A& sx, A& sy) {
  A ax = A(0), ay = A(0);
  for (int j = threadIdx.x; j < nb; j += kThreads) {
    ax += part[j];
    ay += part[nb + j];
  }
  block_sum2(ax, ay, sx, sy);
}

template <bool LAMB, bool SKIP, typename P, typename G, typename S, bool MASTER>
__global__ __launch_bounds__(kThreads) void lw_stats_kernel(OptArgs a, RuleHyper h) {
  using C = typename Comp<P>::type;
  if (step_skipped<SKIP>(h.dev_skip)) return;  // LAMB: m and v stay; the partials too (nobody reads them)
  const Chunk ch = chunk_of(a);
  const int t = ch.t, c = ch.c, nb = ch.nb;
  const LwScalars<C> s = lw_scalars<C>(h, LAMB);

  const P* __restrict__ p = reinterpret_cast<const P*>(a.p[t]);
  const G* __restrict__ g = reinterpret_cast<const G*>(a.g[t]);
  S* __restrict__ m = reinterpret_cast<S*>(a.s1[t]);
  S* __restrict__ v = reinterpret_cast<S*>(a.s2[t]);
  const float* __restrict__ w = reinterpret_cast<const float*>(a.w[t]);
  C* __restrict__ part = reinterpret_cast<C*>(a.s3[t]);
  const int tid = threadIdx.x;

  C ax = C(0), ay = C(0);
  // one element: x, the scaled gradient and (LAMB) the moments in and out
  auto elem = [&](C x, G g_in, S& m_io, S& v_io) {
#pragma clang fp contract(off)
    const C gg = static_cast<C>(g_in) * s.gs;
    ax += x * x;
    if (LAMB) {
      m_io = static_cast<S>(s.b1 * static_cast<C>(m_io) + (C(1) - s.b1) * gg);
      v_io = static_cast<S>(s.b2 * static_cast<C>(v_io) + (C(1) - s.b2) * (gg * gg));
      const C u = lamb_u(s, static_cast<C>(m_io), static_cast<C>(v_io), x);
      ay += u * u;
    } else {
      ay += gg * gg;
    }
  };

  // A thread owns the same elements whether or not the leaf is 16-byte aligned (unaligned: element
  // loads in the vector layout), so its sums add in one order and the ratio does not depend on alignment.
  const bool vec = aligned16(g) && (MASTER ? aligned16(w) : aligned16(p)) && (!LAMB || (aligned16(m) && aligned16(v)));
  const int64_t nvec = (ch.end - ch.base) / kVec;
#pragma unroll
  for (int k = 0; k < kIters; ++k) {
    const int64_t vi = tid + k * kThreads;
    if (vi < nvec) {
      const int64_t off = ch.base + vi * kVec;
      P pv[kVec]; G gv[kVec]; S mv[kVec]; S vv[kVec]; float wv[kVec];
      load8_any(vec, g + off, gv);
      if (LAMB) { load8_any(vec, m + off, mv); load8_any(vec, v + off, vv); }
      if (MASTER) load8_any(vec, w + off, wv); else load8_any(vec, p + off, pv);
#pragma unroll
      for (int j = 0; j < kVec; ++j)
        elem(MASTER ? static_cast<C>(wv[j]) : static_cast<C>(pv[j]), gv[j], mv[j], vv[j]);
      if (LAMB) { store8_any(vec, m + off, mv); store8_any(vec, v + off, vv); }
    }
  }
  const int64_t scalar_from = ch.base + nvec * kVec;
  for (int64_t i = scalar_from + tid; i < ch.end; i += kThreads) {
    S mv = LAMB ? m[i] : S(0), vv = LAMB ? v[i] : S(0);
    elem(MASTER ? static_cast<C>(w[i]) : static_cast<C>(p[i]), g[i], mv, vv);
    if (LAMB) { m[i] = mv; v[i] = vv; }
  }
  C sx, sy;
  block_sum2(ax, ay, sx, sy);
  if (tid == 0) {
    part[c] = sx;
    part[nb + c] = sy;
  }
}

// the fold as a launch of its own: workgroup t leaves leaf t's ratio in the table
template <bool LAMB, bool SKIP, typename C>
__global__ __launch_bounds__(kThreads) void lw_fold_kernel(OptArgs a, RuleHyper h) {
  if (step_skipped<SKIP>(h.dev_skip)) return;  // the ratio table stays as the previous step wrote it
  const int t = blockIdx.x;
  const LwScalars<C> s = lw_scalars<C>(h, LAMB);
  C sx, sy;
  lw_fold(reinterpret_cast<const C*>(a.s3[t]), a.start[t + 1] - a.start[t], sx, sy);
  if (threadIdx.x == 0) static_cast<C*>(const_cast<void*>(h.tscale))[a.tidx[t]] = lw_ratio<LAMB>(s, sx, sy);
}

// FOLD: the fold is this kernel's prologue; else q is read from the ratio table
template <bool LAMB, bool FOLD, bool SKIP, typename P, typename G, typename S, bool MASTER>
__global__ __launch_bounds__(kThreads) void lw_apply_kernel(OptArgs a, RuleHyper h) {
  using C = typename Comp<P>::type;
  if (step_skipped<SKIP>(h.dev_skip)) return;  // before the fold: the ratio table stays too
  const Chunk ch = chunk_of(a);
  const int t = ch.t, c = ch.c;
  const LwScalars<C> s = lw_scalars<C>(h, LAMB);
  const int tid = threadIdx.x;

  C* __restrict__ ratio = static_cast<C*>(const_cast<void*>(h.tscale));
  C q;
  if (FOLD) {
    C sx, sy;
    lw_fold(reinterpret_cast<const C*>(a.s3[t]), ch.nb, sx, sy);
    q = lw_ratio<LAMB>(s, sx, sy);
    if (c == 0 && tid == 0) ratio[a.tidx[t]] = q;
  } else {
    q = ratio[a.tidx[t]];
  }
  const C step = s.lr * q;  // LAMB: x -= (lr*q) * u

  P* __restrict__ p = reinterpret_cast<P*>(a.p[t]);
  const G* __restrict__ g = reinterpret_cast<const G*>(a.g[t]);
  S* __restrict__ s1 = reinterpret_cast<S*>(a.s1[t]);        // LARS: the velocity; LAMB: m
  const S* __restrict__ s2 = reinterpret_cast<const S*>(a.s2[t]);  // LAMB: v
  float* __restrict__ w = reinterpret_cast<float*>(a.w[t]);

  // one element: LARS reads the gradient and rewrites the velocity; LAMB reads m and v
  auto elem = [&](P& p_io, G g_in, S& a_io, S v_in, float& w_io) {
#pragma clang fp contract(off)
    C x = MASTER ? static_cast<C>(w_io) : static_cast<C>(p_io);
    if (LAMB) {
      x -= step * lamb_u(s, static_cast<C>(a_io), static_cast<C>(v_in), x);
    } else {
      C d = static_cast<C>(g_in) * s.gs;
      if (s.wd != C(0)) d += s.wd * x;
      const C vel = s.b1 * static_cast<C>(a_io) + s.lr * (q * d);
      a_io = static_cast<S>(vel);
      x -= vel;
    }
    if (MASTER) w_io = static_cast<float>(x);
    p_io = static_cast<P>(x);
  };

  const bool vec = aligned16(p) && aligned16(s1) && (LAMB ? aligned16(s2) : aligned16(g)) && (!MASTER || aligned16(w));
  int64_t scalar_from = ch.base;
  if (vec) {
    const int64_t nvec = (ch.end - ch.base) / kVec;
#pragma unroll
    for (int k = 0; k < kIters; ++k) {
      const int64_t vi = tid + k * kThreads;
      if (vi < nvec) {
        const int64_t off = ch.base + vi * kVec;
        P pv[kVec]; G gv[kVec]; S av[kVec]; S bv[kVec]; float wv[kVec];
        load8(s1 + off, av);
        if (LAMB) load8(s2 + off, bv); else load8(g + off, gv);
        if (MASTER) load8(w + off, wv); else load8(p + off, pv);
#pragma unroll
        for (int j = 0; j < kVec; ++j) elem(pv[j], gv[j], av[j], bv[j], wv[j]);
        if (!LAMB) store8(s1 + off, av);
        if (MASTER) store8(w + off, wv);
        store8(p + off, pv);
      }
    }
    scalar_from = ch.base + nvec * kVec;
  }
  for (int64_t i = scalar_from + tid; i < ch.end; i += kThreads) {
    P pv = p[i];
    S av = s1[i];
    const S bv = LAMB ? s2[i] : S(0);
    const G gv = LAMB ? G(0) : g[i];
    float wv = MASTER ? w[i] : 0.f;
    elem(pv, gv, av, bv, wv);
    if (!LAMB) s1[i] = av;
    if (MASTER) w[i] = wv;
    p[i] = pv;
  }
}

// FLUXMPI_LAYERWISE_FOLD = prologue | launch pins the fold variant (measurements; read at every call,
// so one process can capture both); else by leaf size
int fold_override() {
  const char* e = std::getenv("FLUXMPI_LAYERWISE_FOLD");
  if (e == nullptr || *e == 0 || std::strcmp(e, "auto") == 0) return -1;
  if (std::strcmp(e, "prologue") == 0) return 0;
  if (std::strcmp(e, "launch") == 0) return 1;
  throw std::runtime_error(std::string("FLUXMPI_LAYERWISE_FOLD: prologue, launch or auto, got ") + e);
}

template <bool LAMB>
void launch_layerwise(const std::vector<uintptr_t>& param, const std::vector<uintptr_t>& grad,
                      const std::vector<uintptr_t>& s1, const std::vector<uintptr_t>& s2,
                      const std::vector<uintptr_t>& part, const std::vector<uintptr_t>& master,
                      const std::vector<int64_t>& numel, int p_dtype, int g_dtype, int s_dtype, const RuleHyper& h,
                      hipStream_t stream) {
  const size_t N = numel.size();
  const char* name = LAMB ? "mt_rule(lamb)" : "mt_rule(lars)";
  // every list the kernels dereference must be there: a missing one would be a null pointer
  if (s1.size() != N || (LAMB && s2.size() != N) || part.size() != N)
    throw std::runtime_error(std::string(name) + ": needs " + (LAMB ? "m, v" : "the velocity") +
                             " and the partials' address (s3) per leaf");
  for (size_t i = 0; i < N; ++i)
    if (numel[i] > 0 && part[i] == 0) throw std::runtime_error(std::string(name) + ": leaf without a partials address");
  if (h.tscale == nullptr) throw std::runtime_error(std::string(name) + ": needs the ratio table (tscale)");
  if (h.clip_delta != 0.f) throw std::runtime_error(std::string(name) + ": no gradient clamp in the layer-wise kernels");
  const bool has_master = !master.empty();
  const int pin = fold_override();
  for_each_group(param, grad, s1, s2, part, master, numel, [&](const OptArgs& a, int blocks) {
    int most = 0;
    for (int t = 0; t < a.n; ++t) most = std::max(most, a.start[t + 1] - a.start[t]);
    const bool own_launch = pin >= 0 ? pin == 1 : most > kFoldLaunchChunks;
    dispatch_opt_combo(p_dtype, g_dtype, s_dtype, has_master, name, [&](auto p, auto g, auto s, auto master) {
      using P = typename decltype(p)::type;
      using G = typename decltype(g)::type;
      using S = typename decltype(s)::type;
      constexpr bool M = decltype(master)::value;
      dispatch_bool(h.dev_skip != nullptr, [&](auto skip) {
        constexpr bool K = decltype(skip)::value;
        lw_stats_kernel<LAMB, K, P, G, S, M><<<blocks, kThreads, 0, stream>>>(a, h);
        FLUXMPI_HIP_CHECK(hipGetLastError());
        if (own_launch) {
          lw_fold_kernel<LAMB, K, typename Comp<P>::type><<<a.n, kThreads, 0, stream>>>(a, h);
          FLUXMPI_HIP_CHECK(hipGetLastError());
          lw_apply_kernel<LAMB, false, K, P, G, S, M><<<blocks, kThreads, 0, stream>>>(a, h);
        } else {
          lw_apply_kernel<LAMB, true, K, P, G, S, M><<<blocks, kThreads, 0, stream>>>(a, h);
        }
      });
    });
    FLUXMPI_HIP_CHECK(hipGetLastError());
  });
}

}  // namespace

void mt_layerwise(const std::vector<uintptr_t>& param, const std::vector<uintptr_t>& grad,
                  const std::vector<uintptr_t>& s1, const std::vector<uintptr_t>& s2,
                  const std::vector<uintptr_t>& s3, const std::vector<uintptr_t>& master,
                  const std::vector<int64_t>& numel, int p_dtype, int g_dtype, int s_dtype, const RuleHyper& h,
                  hipStream_t stream) {
  if (h.kind == kLamb)
    launch_layerwise<true>(param, grad, s1, s2, s3, master, numel, p_dtype, g_dtype, s_dtype, h, stream);
  else
    launch_layerwise<false>(param, grad, s1, s2, s3, master, numel, p_dtype, g_dtype, s_dtype, h, stream);
}

}  // namespace fluxmpi
