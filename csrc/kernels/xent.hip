// Fused softmax cross-entropy for classifier heads — gfx950: row loss, gradient and top-k rank.
//
// Logits x [B, C] (bf16 / fp16 / fp32, contiguous), all arithmetic fp32, rows indexed in int64.
// One 64-lane wavefront per row, 4 rows per 256-thread workgroup, a persistent grid that walks
// rows row, row + step, ... (layernorm.hip's shape).
//
//   forward   m = max_j x_j, e_j = exp2((x_j - m) log2e), s = sum_j e_j, lse = m + ln2 log2(s)
//             loss_row = W lse - d;  rank = #{j : x_j > x_y} + #{j < y : x_j == x_y}
//   finish    loss = sum_b loss_row[b] (fixed order) [* fl32(1/B)];  the meter block += the batch
//   backward  r = 1 / s, p_j = exp2((x_j - m) log2e) r, dx_j = (p_j W - t_j) gs, one rounding
//
// Target forms (a mode word, wave-uniform branches):
//   hard    labels y, smoothing eps:  d = (1 - eps) x_y + eps mean(x), W = 1
//   mixed   labels, partner row B - 1 - b, lam by value or from a device word, rest = fl32(1 - lam):
//           d = (1 - eps)(lam x_y + rest x_yp) + (lam + rest) eps mean(x), W = lam + rest
//   dense   t [B, C] (fp32 / bf16 / fp16), t' = t (1 - eps) + eps / C:  d = sum t' x, W = sum t'
//
// Register path (C % 8 == 0, C <= 8192, 16-byte aligned bases): the row stays in registers in its
// stored form between the passes (16-byte loads, every load unconditional, lanes past the row
// masked in the math); up to 4 vectors per lane the next row's loads are issued before the
// current row's reductions. General path (any other C >= 1, or an unaligned base): a lane takes
// elements lane, lane + 64, ... in a loop, online softmax (running max, rescaled sum) in the first
// sweep; no load leaves the tensor. Labels are compared, never used as an address: a label outside
// [0, C) gives a wrong number, not a fault. No LDS (but the finish kernel's block sum), no atomics.
#include <stdexcept>
#include <string>

#include "../api.h"
#include "optim_common.h"  // kThreads, block_sum (the fixed-order block reduction)

namespace fluxmpi {
namespace {

constexpr int kWaves = kThreads / 64;
// log2(e) and ln(2) as fp32 head + tail: (x - m) log2e and ln2 log2(s) then carry no error of the
// constant's own rounding (0.22 u and 0.05 u of the product), one fma more each
constexpr float kLog2eHi = 1.4426950216293335f, kLog2eLo = 1.925963033500309e-8f;
constexpr float kLn2Hi = 0.6931471824645996f, kLn2Lo = -1.904654299957767e-9f;
constexpr float kLowest = -3.4028234663852886e38f;  // the running max starts here: -inf - -inf would be NaN
enum : int { kHard = 0, kMixed = 1, kDense = 2 };
enum : int { kMean = 0, kSum = 1, kNone = 2 };

__device__ __forceinline__ float fast_exp2(float x) { return __builtin_amdgcn_exp2f(x); }  // bare v_exp_f32
// exp(d) for d = x - m <= 0 (subtracted first): one rounding of the argument
__device__ __forceinline__ float exp_of(float d) { return fast_exp2(fmaf(d, kLog2eHi, d * kLog2eLo)); }
__device__ __forceinline__ float fast_log2(float x) { return __builtin_amdgcn_logf(x); }   // bare v_log_f32

__device__ __forceinline__ float wave_sum(float v) { return wave_sum_dpp(v); }

// max over all 64 lanes, wave-uniform: DPP row maxima, then the four row results read as scalars
// (wave_sum_dpp's shape; EXEC must be full)
__device__ __forceinline__ float wave_max(float v) {
  v = fmaxf(v, dpp_f<0xB1>(v));   // quad_perm [1,0,3,2]
  v = fmaxf(v, dpp_f<0x4E>(v));   // quad_perm [2,3,0,1]
  v = fmaxf(v, dpp_f<0x124>(v));  // row_ror:4
  v = fmaxf(v, dpp_f<0x128>(v));  // row_ror:8
  const int b = __builtin_bit_cast(int, v);
  return fmaxf(fmaxf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 0)),
                     __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 16))),
               fmaxf(__builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 32)),
                     __builtin_bit_cast(float, __builtin_amdgcn_readlane(b, 48))));
}

// integer wave sum in the same style (the rank is an exact count for any C)
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}
__device__ __forceinline__ int wave_sum_int(int v) {
  v += dpp_i<0xB1>(v);
  v += dpp_i<0x4E>(v);
  v += dpp_i<0x124>(v);
  v += dpp_i<0x128>(v);
  return (__builtin_amdgcn_readlane(v, 0) + __builtin_amdgcn_readlane(v, 16)) +
         (__builtin_amdgcn_readlane(v, 32) + __builtin_amdgcn_readlane(v, 48));
}

// what a launch knows about the targets
struct XentTarget {
  const void* labels;     // [B] int32 / int64, or null (dense without rank)
  const void* dense;      // [B, C], or null
  const float* dev_lam;   // mixed: lam read from this device word when not null
  float lam, eps;
  int mode, label_i64;
};

__device__ __forceinline__ int64_t label_at(const XentTarget& t, int64_t row) {
  return t.label_i64 ? static_cast<const int64_t*>(t.labels)[row]
                     : static_cast<int64_t>(static_cast<const int32_t*>(t.labels)[row]);
}

// a row's target in the label forms: t_j = [j == y] wy + [j == yp] wp + u
struct RowTarget {
  int64_t y = -1, yp = -1;
  float lam = 1.f, rest = 0.f, W = 1.f, ome = 1.f;
};

__device__ __forceinline__ RowTarget row_target(const XentTarget& t, int64_t row, int64_t B) {
  RowTarget o;
  o.ome = 1.f - t.eps;
  if (t.labels != nullptr) o.y = label_at(t, row);
  if (t.mode == kMixed) {
    o.yp = label_at(t, B - 1 - row);
    o.lam = t.dev_lam != nullptr ? *t.dev_lam : t.lam;
    o.rest = 1.f - o.lam;
    o.W = o.lam + o.rest;
  }
  return o;
}

// A lane's vectors lane + 64 i of a row; lanes past the row load vector 0 and are masked
template <int VPL>
struct Lanes {
  int vc[VPL > 0 ? VPL : 1];
  bool act[VPL > 0 ? VPL : 1];
  __device__ __forceinline__ Lanes(int lane, int nv) {
#pragma unroll
    for (int i = 0; i < VPL; ++i) {
      const int v = lane + i * 64;
      act[i] = v < nv;
      vc[i] = act[i] ? v : 0;
    }
  }
};

// a row's label values, read beside the row: x_y and x_yp through a clamped index (the load is
// unconditional and stays inside the row whatever the label is; a label outside [0, C) gives 0)
struct RowHead {
  RowTarget rt;
  float xy, xp;
};

template <typename T>
__device__ __forceinline__ RowHead row_head(const T* __restrict__ x, const XentTarget& t, int64_t row, int64_t B,
                                            int64_t C) {
  RowHead h;
  h.rt = row_target(t, row, B);
  auto pick = [&](int64_t y) {
    const int64_t c = y < 0 ? 0 : (y >= C ? C - 1 : y);
    const float v = to_f(x[row * C + c]);
    return c == y ? v : 0.f;
  };
  h.xy = pick(h.rt.y);
  h.xp = pick(h.rt.yp);
  return h;
}

// One row of the forward. `sweep(fn)` visits the lane's elements: fn(x_c, t_c, below, active) with
// below = [c < y] (the tie rule of the rank).
// ONLINE (general path): the first sweep keeps a running max and a rescaled sum.
template <bool ONLINE, bool DENSE, typename S>
__device__ __forceinline__ void fwd_row(S&& sweep, const XentTarget& t, const RowHead& h, int64_t row, float inv_c,
                                        float eps_c, int lane, float* __restrict__ loss_row,
                                        float* __restrict__ m_out, float* __restrict__ s_out,
                                        int32_t* __restrict__ rank_out) {
  const RowTarget& rt = h.rt;
  const float xy = h.xy;
  float mx = kLowest, sl = 0.f, sx = 0.f, dd = 0.f, ww = 0.f;
  sweep([&](float f, float tv, int below, bool act) {
    if (ONLINE) {
      const float mn = fmaxf(mx, f);
      sl = sl * exp_of(mx - mn) + exp_of(f - mn);
      mx = mn;
    } else {
      mx = act ? fmaxf(mx, f) : mx;
    }
    if (DENSE) {
      const float tp = tv * rt.ome + eps_c;
      dd += act ? tp * f : 0.f;
      ww += act ? tp : 0.f;
    } else {
      sx += act ? f : 0.f;
    }
  });
  const float m = wave_max(mx);
  float s = 0.f;
  if (ONLINE) s = wave_sum(sl * exp_of(mx - m));
  const bool want_rank = rank_out != nullptr;
  if (!ONLINE || want_rank) {
    int cnt = 0;
    float sl2 = 0.f;
    sweep([&](float f, float tv, int below, bool act) {
      if (!ONLINE) sl2 += act ? exp_of(f - m) : 0.f;
      const int beats = (f > xy ? 1 : 0) | ((f == xy ? 1 : 0) & below);
      cnt += act ? beats : 0;
    });
    if (!ONLINE) s = wave_sum(sl2);
    if (want_rank) {
      cnt = wave_sum_int(cnt);
      if (lane == 0) rank_out[row] = cnt;
    }
  }
  const float l2 = fast_log2(s);
  const float lse = fmaf(kLn2Lo, l2, fmaf(kLn2Hi, l2, m));
  float d, W;
  if (DENSE) {
    d = wave_sum(dd);
    W = wave_sum(ww);
  } else {
    const float mean = wave_sum(sx) * inv_c;
    W = rt.W;  // 1 in the hard form
    if (t.mode == kMixed) d = rt.ome * (rt.lam * xy + rt.rest * h.xp) + W * (t.eps * mean);
    else d = rt.ome * xy + t.eps * mean;
  }
  if (lane == 0) {
    loss_row[row] = W * lse - d;
    m_out[row] = m;
    s_out[row] = s;
  }
}

// One row of the backward: `emit(fn)` visits the lane's elements and stores fn(base, j, x_c, t_c);
// `tsum(fn)` (dense) sums fn(t_c) over the lane's elements.
template <bool DENSE, typename E, typename TS>
__device__ __forceinline__ void bwd_row(E&& emit, TS&& tsum, const XentTarget& t, const RowTarget& rt, float eps_c,
                                        float m, float s, float gs) {
  const float r = 1.0f / s;
  float W = rt.W;
  if (DENSE) W = wave_sum(tsum([&](float tv) { return tv * rt.ome + eps_c; }));
  const float wy = rt.ome * rt.lam, wp = rt.ome * rt.rest, u = W * eps_c;
  emit([&](int64_t base, int j, float f, float tv) {
    const float p = exp_of(f - m) * r;
    float tj;
    if (DENSE) tj = tv * rt.ome + eps_c;
    else tj = ((j == rt.y - base ? wy : 0.f) + (j == rt.yp - base ? wp : 0.f)) + u;
    return (p * W - tj) * gs;
  });
}

template <typename T, int VPL, typename TT, bool DENSE>
__global__ __launch_bounds__(kThreads) void xent_fwd_kernel(const T* __restrict__ x, XentTarget t,
                                                            float* __restrict__ loss_row, float* __restrict__ m_out,
                                                            float* __restrict__ s_out, int32_t* __restrict__ rank_out,
                                                            int64_t B, int64_t C) {
  const int lane = threadIdx.x & 63;
  const int64_t step = static_cast<int64_t>(gridDim.x) * kWaves;
  int64_t row = static_cast<int64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6);
  if (row >= B) return;  // no block-level synchronisation below
  const float inv_c = 1.f / static_cast<float>(C);
  const float eps_c = t.eps / static_cast<float>(C);
  const TT* __restrict__ td = static_cast<const TT*>(t.dense);
  if constexpr (VPL == 0) {
    for (; row < B; row += step) {
      const T* __restrict__ xr = x + row * C;
      const TT* __restrict__ tr = DENSE ? td + row * C : nullptr;
      const RowHead h = row_head(x, t, row, B, C);
      auto sweep = [&](auto&& fn) {
        for (int64_t c = lane; c < C; c += 64) fn(to_f(xr[c]), DENSE ? to_f(tr[c]) : 0.f, c < h.rt.y ? 1 : 0, true);
      };
      fwd_row<true, DENSE>(sweep, t, h, row, inv_c, eps_c, lane, loss_row, m_out, s_out, rank_out);
    }
  } else {
    const Lanes<VPL> L(lane, static_cast<int>(C / 8));
    constexpr int TV = DENSE ? VPL : 1;
    struct Buf {
      T x[VPL][8];
      TT t[TV][8];
      RowHead h;
    };
    auto load = [&](int64_t rw, Buf& o) {
      o.h = row_head(x, t, rw, B, C);
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        load8(x + rw * C + L.vc[i] * 8, o.x[i]);
        if (DENSE) load8(td + rw * C + L.vc[i] * 8, o.t[DENSE ? i : 0]);
      }
    };
    auto process = [&](int64_t rw, const Buf& c) {
      auto sweep = [&](auto&& fn) {
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
          // bit j: element j of this vector lies below the label (one mask per vector, not a compare per element)
          const int64_t nb = c.h.rt.y - static_cast<int64_t>(L.vc[i]) * 8;
          const unsigned below = nb <= 0 ? 0u : (nb >= 8 ? 0xFFu : (1u << static_cast<int>(nb)) - 1u);
#pragma unroll
          for (int j = 0; j < 8; ++j)
            fn(to_f(c.x[i][j]), DENSE ? to_f(c.t[DENSE ? i : 0][j]) : 0.f, static_cast<int>((below >> j) & 1u),
               L.act[i]);
        }
      };
      fwd_row<false, DENSE>(sweep, t, c.h, rw, inv_c, eps_c, lane, loss_row, m_out, s_out, rank_out);
    };
    // PF (up to 4 vectors per lane): the next row's loads in flight during this row's reductions
    // (unconditional: the last row re-reads itself); wider rows would spill the second buffer
    constexpr bool PF = VPL <= 4;
    Buf cur;
    load(row, cur);
    while (true) {
      const int64_t nrow = row + step;
      const bool more = nrow < B;
      if (PF) {
        Buf nxt;
        load(more ? nrow : row, nxt);
        process(row, cur);
        if (!more) break;
        cur = nxt;
      } else {
        process(row, cur);
        if (!more) break;
        load(nrow, cur);
      }
      row = nrow;
    }
  }
}

// One workgroup: thread i adds loss_row[i], loss_row[i + 256], ... in sequence, then block_sum
// (mt_sumsq_finish_kernel's order: the same bits in every run). meter: {fp64 sum of the row
// losses, int64 rows, int64 rank < k0, int64 rank < k1}, updated by one thread with plain stores.
__global__ __launch_bounds__(kThreads) void xent_finish_kernel(const float* __restrict__ loss_row,
                                                               const int32_t* __restrict__ rank,
                                                               float* __restrict__ loss, void* __restrict__ meter,
                                                               int64_t B, float scale, int k0, int k1) {
  float acc = 0.f;
  for (int64_t j = threadIdx.x; j < B; j += kThreads) acc += loss_row[j];
  const float sum = block_sum(acc);
  if (loss != nullptr && threadIdx.x == 0) loss[0] = sum * scale;
  if (meter == nullptr) return;
  double c0 = 0.0, c1 = 0.0;  // counts: exact in fp64
  for (int64_t j = threadIdx.x; j < B; j += kThreads) {
    const int32_t r = rank[j];
    c0 += r < k0 ? 1.0 : 0.0;
    c1 += r < k1 ? 1.0 : 0.0;
  }
  double t0, t1;
  block_sum2(c0, c1, t0, t1);
  if (threadIdx.x == 0) {
    double* ms = static_cast<double*>(meter);
    int64_t* mi = static_cast<int64_t*>(meter);
    ms[0] += static_cast<double>(sum);
    mi[1] += B;
    mi[2] += static_cast<int64_t>(t0);
    mi[3] += static_cast<int64_t>(t1);
  }
}

template <typename T, int VPL, typename TT, bool DENSE>
__global__ __launch_bounds__(kThreads) void xent_bwd_kernel(const T* __restrict__ x, XentTarget t,
                                                            const float* __restrict__ m_in,
                                                            const float* __restrict__ s_in,
                                                            const float* __restrict__ g, T* __restrict__ dx,
                                                            int64_t B, int64_t C, int reduction, float inv_b) {
  const int lane = threadIdx.x & 63;
  const int64_t step = static_cast<int64_t>(gridDim.x) * kWaves;
  int64_t row = static_cast<int64_t>(blockIdx.x) * kWaves + (threadIdx.x >> 6);
  if (row >= B) return;
  const float eps_c = t.eps / static_cast<float>(C);
  const TT* __restrict__ td = static_cast<const TT*>(t.dense);
  auto gs_of = [&](int64_t rw) { return reduction == kNone ? g[rw] : (reduction == kMean ? g[0] * inv_b : g[0]); };
  if constexpr (VPL == 0) {
    for (; row < B; row += step) {
      const T* __restrict__ xr = x + row * C;
      T* __restrict__ dr = dx + row * C;
      const TT* __restrict__ tr = DENSE ? td + row * C : nullptr;
      auto emit = [&](auto&& fn) {
        for (int64_t c = lane; c < C; c += 64) dr[c] = from_f<T>(fn(c, 0, to_f(xr[c]), DENSE ? to_f(tr[c]) : 0.f));
      };
      auto tsum = [&](auto&& fn) {
        float a = 0.f;
        if (DENSE)
          for (int64_t c = lane; c < C; c += 64) a += fn(to_f(tr[c]));
        return a;
      };
      bwd_row<DENSE>(emit, tsum, t, row_target(t, row, B), eps_c, m_in[row], s_in[row], gs_of(row));
    }
  } else {
    const Lanes<VPL> L(lane, static_cast<int>(C / 8));
    constexpr int TV = DENSE ? VPL : 1;
    struct Buf {
      T x[VPL][8];
      TT t[TV][8];
      float m, s, gs;
    };
    auto load = [&](int64_t rw, Buf& o) {
      o.m = m_in[rw];
      o.s = s_in[rw];
      o.gs = gs_of(rw);
#pragma unroll
      for (int i = 0; i < VPL; ++i) {
        load8(x + rw * C + L.vc[i] * 8, o.x[i]);
        if (DENSE) load8(td + rw * C + L.vc[i] * 8, o.t[DENSE ? i : 0]);
      }
    };
    auto process = [&](int64_t rw, const Buf& c) {
      auto emit = [&](auto&& fn) {
#pragma unroll
        for (int i = 0; i < VPL; ++i) {
          T o[8];
#pragma unroll
          for (int j = 0; j < 8; ++j)
            o[j] = from_f<T>(fn(static_cast<int64_t>(L.vc[i] * 8), j, to_f(c.x[i][j]),
                                DENSE ? to_f(c.t[DENSE ? i : 0][j]) : 0.f));
          if (L.act[i]) store8(dx + rw * C + L.vc[i] * 8, o);
        }
      };
      auto tsum = [&](auto&& fn) {
        float a = 0.f;
        if (DENSE) {
#pragma unroll
          for (int i = 0; i < VPL; ++i)
#pragma unroll
            for (int j = 0; j < 8; ++j) a += L.act[i] ? fn(to_f(c.t[DENSE ? i : 0][j])) : 0.f;
        }
        return a;
      };
      bwd_row<DENSE>(emit, tsum, t, row_target(t, rw, B), eps_c, c.m, c.s, c.gs);
    };
    constexpr bool PF = VPL <= 4;
    Buf cur;
    load(row, cur);
    while (true) {
      const int64_t nrow = row + step;
      const bool more = nrow < B;
      if (PF) {
        Buf nxt;
        load(more ? nrow : row, nxt);  // unconditional: the last row re-reads itself
        process(row, cur);
        if (!more) break;
        cur = nxt;
      } else {
        process(row, cur);
        if (!more) break;
        load(nrow, cur);
      }
      row = nrow;
    }
  }
}

// vectors per lane of the register path, 0 for the general path
int xent_vpl(int64_t C, bool aligned) {
  if (!aligned || C % 8 != 0 || C < 8 || C > 8192) return 0;
  const int v = static_cast<int>((C / 8 + 63) / 64);
  for (int c : {1, 2, 3, 4, 6, 8, 12, 16})
    if (c >= v) return c;
  return 0;
}

bool aligned16_host(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

// logits dtype x dense-target dtype (or none) x the vectors-per-lane variants:
// f(TypeTag<T>, TypeTag<TT>, bool_constant<DENSE>, VPL)
template <typename F>
void dispatch_xent(const char* who, int dtype, bool dense, int tdtype, int vpl, F&& f) {
  const std::string w(who);
  dispatch_float(dtype, w + ": logits must be bf16, fp16 or fp32", [&](auto t) {
    dispatch_int<0, 1, 2, 3, 4, 6, 8, 12, 16>(vpl, w + ": no kernel for this C", [&](auto v) {
      if (!dense) {
        f(t, TypeTag<float>{}, std::false_type{}, v);
      } else {
        dispatch_float(tdtype, w + ": dense targets must be fp32, bf16 or fp16",
                       [&](auto tt) { f(t, tt, std::true_type{}, v); });
      }
    });
  });
}

XentTarget make_target(const char* who, const void* labels, const void* target, int label_dtype, int mode, float eps,
                       float lam, const float* dev_lam) {
  const std::string w(who);
  if (mode != kHard && mode != kMixed && mode != kDense) throw std::runtime_error(w + ": mode is 0 (hard), 1 (mixed) or 2 (dense)");
  if (mode == kDense ? target == nullptr : labels == nullptr)
    throw std::runtime_error(w + ": the mode's targets are missing");
  if (labels != nullptr && label_dtype != static_cast<int>(kI32) && label_dtype != static_cast<int>(kI64))
    throw std::runtime_error(w + ": labels must be int32 or int64");
  if (!(eps >= 0.f && eps < 1.f)) throw std::runtime_error(w + ": label smoothing must lie in [0, 1)");
  return XentTarget{labels, mode == kDense ? target : nullptr, mode == kMixed ? dev_lam : nullptr, lam, eps, mode,
                    label_dtype == static_cast<int>(kI64)};
}

template <typename K>
unsigned row_grid(K kernel, int64_t B) {
  int64_t blocks = resident_blocks(reinterpret_cast<const void*>(kernel), kThreads, 0);
  const int64_t need = (B + kWaves - 1) / kWaves;
  if (blocks > need) blocks = need;
  return static_cast<unsigned>(blocks < 1 ? 1 : blocks);
}

}  // namespace

void xent_fwd(const void* x, const void* labels, const void* target, float* loss_row, float* m, float* s,
              int32_t* rank, int64_t B, int64_t C, int dtype, int label_dtype, int target_dtype, int mode, float eps,
              float lam, const float* dev_lam, hipStream_t stream) {
  if (B < 1 || C < 1) throw std::runtime_error("xent_fwd: need B >= 1 and C >= 1");
  if (x == nullptr || loss_row == nullptr || m == nullptr || s == nullptr)
    throw std::runtime_error("xent_fwd: null pointer");
  const XentTarget t = make_target("xent_fwd", labels, target, label_dtype, mode, eps, lam, dev_lam);
  if (rank != nullptr && labels == nullptr) throw std::runtime_error("xent_fwd: the rank needs labels");
  const bool dense = mode == kDense;
  const int vpl = xent_vpl(C, aligned16_host(x) && (!dense || aligned16_host(target)));
  dispatch_xent("xent_fwd", dtype, dense, target_dtype, vpl, [&](auto tt, auto dt, auto dn, auto v) {
    using T = typename decltype(tt)::type;
    auto k = xent_fwd_kernel<T, decltype(v)::value, typename decltype(dt)::type, decltype(dn)::value>;
    k<<<row_grid(k, B), kThreads, 0, stream>>>(static_cast<const T*>(x), t, loss_row, m, s, rank, B, C);
  });
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

void xent_finish(const float* loss_row, const int32_t* rank, float* loss, void* meter, int64_t B, int reduction,
                 int k0, int k1, hipStream_t stream) {
  if (B < 1 || loss_row == nullptr) throw std::runtime_error("xent_finish: need B >= 1 and the row losses");
  if (loss == nullptr && meter == nullptr) throw std::runtime_error("xent_finish: nothing to write");
  if (meter != nullptr && rank == nullptr) throw std::runtime_error("xent_finish: the meter needs the ranks");
  if (reduction != kMean && reduction != kSum) throw std::runtime_error("xent_finish: reduction is 0 (mean) or 1 (sum)");
  const float scale = reduction == kMean ? static_cast<float>(1.0 / static_cast<double>(B)) : 1.f;
  xent_finish_kernel<<<1, kThreads, 0, stream>>>(loss_row, rank, loss, meter, B, scale, k0, k1);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

void xent_bwd(const void* x, const void* labels, const void* target, const float* m, const float* s, const float* g,
              void* dx, int64_t B, int64_t C, int dtype, int label_dtype, int target_dtype, int mode, int reduction,
              float eps, float lam, const float* dev_lam, hipStream_t stream) {
  if (B < 1 || C < 1) throw std::runtime_error("xent_bwd: need B >= 1 and C >= 1");
  if (x == nullptr || m == nullptr || s == nullptr || g == nullptr || dx == nullptr)
    throw std::runtime_error("xent_bwd: null pointer");
  if (reduction != kMean && reduction != kSum && reduction != kNone)
    throw std::runtime_error("xent_bwd: reduction is 0 (mean), 1 (sum) or 2 (none)");
  const XentTarget t = make_target("xent_bwd", labels, target, label_dtype, mode, eps, lam, dev_lam);
  const bool dense = mode == kDense;
  const int vpl = xent_vpl(C, aligned16_host(x) && aligned16_host(dx) && (!dense || aligned16_host(target)));
  const float inv_b = static_cast<float>(1.0 / static_cast<double>(B));
  dispatch_xent("xent_bwd", dtype, dense, target_dtype, vpl, [&](auto tt, auto dt, auto dn, auto v) {
    using T = typename decltype(tt)::type;
    auto k = xent_bwd_kernel<T, decltype(v)::value, typename decltype(dt)::type, decltype(dn)::value>;
    k<<<row_grid(k, B), kThreads, 0, stream>>>(static_cast<const T*>(x), t, m, s, g, static_cast<T*>(dx), B, C,
                                               reduction, inv_b);
  });
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace fluxmpi
