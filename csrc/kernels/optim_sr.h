// Stochastic rounding of the bf16 stores of the fused optimiser kernels (DDP(master_weights=False,
// stochastic_rounding=...)): a counter-based generator inside the update kernels, so that a store is
// unbiased and a pure-bf16 parameter / moment layout can be trained with.
//
// The rounding sr(x, r) of an fp32 value with bits u and 16 random bits r: the bf16 with bits
// (u + r) >> 16; inf / NaN (exponent field all ones) take the round-to-nearest cast. A value bf16
// represents is unchanged for every r, the sign is kept (the add acts on the magnitude bits), and
// P(away from zero) = (u & 0xffff) / 65536 exactly. A finite value above the largest bf16 may carry
// into +-inf: correct stochastic rounding.
//
// The generator is Philox4x32-10. One call yields 128 bits = 8 x 16: one kVec vector. For element i
// of a leaf: e = offset[leaf] + i, q = e >> 3, j = e & 7; key (seed lo, seed hi), counter (q lo, q hi,
// stream * 4 + slot, step); r_j = (w[j >> 1] >> (16 * (j & 1))) & 0xffff. slot: 0 the parameter,
// 1..3 the state tensors. The bits depend on e alone, so the 16-byte vector path (taken when
// offset % 8 == 0) and the scalar path agree, and so do one launch over a flat bucket and per-leaf
// launches over its slices.
//
// SrArgs reaches a kernel as a third parameter that only the stochastic-rounding instantiations have (a
// parameter pack that is empty otherwise): OptArgs and the round-to-nearest kernels (Rnd =
// RoundNearest below, an empty type whose cast is static_cast) are what they were.
#pragma once
#include <stdexcept>
#include <string>
#include <type_traits>

#include "optim_common.h"

namespace fluxmpi {

// words of the step block (api.h: sr_advance)
constexpr int kSrStep = 0;

struct SrArgs {
  int64_t offset[kMaxT];     // per leaf of the launch: index of its first element in the random stream
  uint32_t key0, key1;       // the seed's halves
  uint32_t stream4;          // stream * 4
  uint32_t step;             // host step (dev_step == nullptr)
  const uint32_t* dev_step;  // optional device block {step, 7 unused}: wave-uniform read
};

struct Philox4 {
  uint32_t w[4];
};

__device__ __forceinline__ Philox4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0,
                                                 uint32_t k1) {
  constexpr uint32_t kM0 = 0xD2511F53u, kM1 = 0xCD9E8D57u, kW0 = 0x9E3779B9u, kW1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    // 32 x 32 -> 64 as one product each (one v_mad_u64_u32 rather than a hi / lo multiply pair)
    const uint64_t p0 = static_cast<uint64_t>(kM0) * c0;
    const uint64_t p1 = static_cast<uint64_t>(kM1) * c2;
    const uint32_t n0 = static_cast<uint32_t>(p1 >> 32) ^ c1 ^ k0;
    const uint32_t n2 = static_cast<uint32_t>(p0 >> 32) ^ c3 ^ k1;
    c1 = static_cast<uint32_t>(p1);
    c3 = static_cast<uint32_t>(p0);
    c0 = n0;
    c2 = n2;
    k0 += kW0;  // (wave-uniform: scalar adds)
    k1 += kW1;
  }
  return {{c0, c1, c2, c3}};
}

__device__ __forceinline__ bf16 sr_bf16(float x, uint32_t r16) {
  const uint32_t u = __builtin_bit_cast(uint32_t, x);
  if ((u & 0x7f800000u) == 0x7f800000u) return static_cast<bf16>(x);
  return __builtin_bit_cast(bf16, static_cast<uint16_t>((u + r16) >> 16));
}

// The rounding policies of the element functors: cast<T>(x, slot) is the store of x into a tensor of
// type T. RoundNearest: static_cast, no state (the kernels without stochastic rounding).
struct RoundNearest {
  template <typename T, typename C>
  __device__ __forceinline__ T cast(C x, int) const { return static_cast<T>(x); }
};

// One element's random bits, r[slot]; only bf16 stores from fp32 read them.
struct RoundStochastic {
  uint32_t r[4];
  template <typename T, typename C>
  __device__ __forceinline__ T cast(C x, int slot) const {
    if constexpr (std::is_same_v<T, bf16> && std::is_same_v<C, float>) return sr_bf16(x, r[slot]);
    else return static_cast<T>(x);
  }
};

// The step's generator state of one leaf, wave-uniform.
struct SrLeaf {
  int64_t offset;
  uint32_t key0, key1, stream4, step;
  __device__ __forceinline__ Philox4 words(int64_t q, int slot) const {
    return philox4x32_10(static_cast<uint32_t>(q), static_cast<uint32_t>(static_cast<uint64_t>(q) >> 32),
                         stream4 + static_cast<uint32_t>(slot), step, key0, key1);
  }
  // vector path: the 8 elements from leaf index `i` on share q (offset and i are multiples of 8)
  __device__ __forceinline__ Philox4 vec_words(int64_t i, int slot) const { return words((offset + i) >> 3, slot); }
  static __device__ __forceinline__ uint32_t pick(const Philox4& p, int j) {
    return (p.w[j >> 1] >> (16 * (j & 1))) & 0xffffu;
  }
  // scalar path: element i's 16 bits of `slot`
  __device__ __forceinline__ uint32_t scalar_bits(int64_t i, int slot) const {
    const int64_t e = offset + i;
    const Philox4 p = words(e >> 3, slot);
    const int j = static_cast<int>(e & 7);
    const uint32_t w = j < 4 ? (j < 2 ? p.w[0] : p.w[1]) : (j < 6 ? p.w[2] : p.w[3]);  // no indexed register file
    return (w >> (16 * (j & 1))) & 0xffffu;
  }
};

__device__ __forceinline__ SrLeaf sr_leaf(const SrArgs& s, int t) {
  return {s.offset[t], s.key0, s.key1, s.stream4, s.dev_step != nullptr ? s.dev_step[kSrStep] : s.step};
}

// What a kernel body sees of all this, by its SR flag. SrCtx<false> is empty and every call on it
// compiles to nothing: the round-to-nearest kernels. `ns`: how many state slots (1..ns) draw bits —
// the rule's state count when the states are bf16, else 0; slot 0 (the parameter) always does.
template <bool SR> struct SrCtx;

template <> struct SrCtx<false> {
  struct Vec {
    __device__ __forceinline__ RoundNearest at(int) const { return {}; }
  };
  __device__ __forceinline__ explicit SrCtx(int) {}
  __device__ __forceinline__ bool vec_ok() const { return true; }
  __device__ __forceinline__ Vec vec(int64_t, int) const { return {}; }
  __device__ __forceinline__ RoundNearest one(int64_t, int) const { return {}; }
};

template <> struct SrCtx<true> {
  struct Vec {
    Philox4 p[4];
    __device__ __forceinline__ RoundStochastic at(int j) const {
      return {{SrLeaf::pick(p[0], j), SrLeaf::pick(p[1], j), SrLeaf::pick(p[2], j), SrLeaf::pick(p[3], j)}};
    }
  };
  SrLeaf l;
  __device__ __forceinline__ SrCtx(int t, const SrArgs& s) : l(sr_leaf(s, t)) {}
  __device__ __forceinline__ bool vec_ok() const { return (l.offset & 7) == 0; }
  __device__ __forceinline__ Vec vec(int64_t i, int ns) const {
    Vec v{};
    v.p[0] = l.vec_words(i, 0);
#pragma unroll
    for (int s = 1; s < 4; ++s)
      if (s <= ns) v.p[s] = l.vec_words(i, s);
    return v;
  }
  __device__ __forceinline__ RoundStochastic one(int64_t i, int ns) const {
    RoundStochastic r{};
    r.r[0] = l.scalar_bits(i, 0);
#pragma unroll
    for (int s = 1; s < 4; ++s)
      if (s <= ns) r.r[s] = l.scalar_bits(i, s);
    return r;
  }
};

// Host side: the launch's SrArgs from the call's (api.h: SrHyper) and the launch's leaves.
inline SrArgs sr_args_for(const SrHyper& h, const OptArgs& a) {
  SrArgs s{};
  for (int k = 0; k < a.n; ++k) s.offset[k] = h.offsets != nullptr ? h.offsets[a.tidx[k]] : 0;
  s.key0 = static_cast<uint32_t>(h.seed);
  s.key1 = static_cast<uint32_t>(h.seed >> 32);
  s.stream4 = h.stream * 4u;
  s.step = h.step;
  s.dev_step = h.dev_step;
  return s;
}

inline void sr_check(const SrHyper& h, size_t leaves, const char* what) {
  if (h.stream >= (1u << 30)) throw std::runtime_error(std::string(what) + ": the stream id must be below 2^30");
  if (h.offsets != nullptr && h.n_offsets != leaves)
    throw std::runtime_error(std::string(what) + ": one offset per leaf");
  for (size_t i = 0; h.offsets != nullptr && i < leaves; ++i)
    if (h.offsets[i] < 0) throw std::runtime_error(std::string(what) + ": offsets are not negative");
}

// the update kernels with stochastic rounding exist for bf16 parameters and gradients without a master,
// with bf16 or fp32 states
inline void sr_check_combo(const SrHyper& h, size_t leaves, int p_dtype, int g_dtype, int s_dtype, bool has_master,
                           const char* what) {
  sr_check(h, leaves, what);
  if (p_dtype != kBF16 || g_dtype != kBF16 || (s_dtype != kBF16 && s_dtype != kF32) || has_master)
    throw std::runtime_error(std::string(what) + ": stochastic rounding is for bf16 parameters and gradients without "
                             "a master, states bf16 or fp32; got p=" + std::to_string(p_dtype) + " g=" +
                             std::to_string(g_dtype) + " s=" + std::to_string(s_dtype) + " master=" +
                             std::to_string(has_master));
}

}  // namespace fluxmpi
