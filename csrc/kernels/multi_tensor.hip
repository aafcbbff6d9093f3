// Multi-tensor copy / cast / scale / fill / sum-of-squares for gfx950.
//
// K1/K2 of SURVEY §2.4: the reference moves every gradient leaf through host
// memory one at a time (src/optimizer.jl:47,62; src/mpi_extensions.jl:97-155).
// Here a single launch gathers many leaves into one contiguous, 16 B-aligned
// communication bucket (pack) or scatters the reduced bucket back (unpack),
// optionally casting (bf16 <-> fp32) and scaling (e.g. 1/world) on the fly.
//
// Work decomposition: workgroup b owns elements [c*kChunk, (c+1)*kChunk) of
// tensor t, where (t, c) comes from a prefix table carried in the kernel
// arguments. Each lane moves 8 elements per step with 16 B vector accesses;
// 4 steps are issued before any store so every lane keeps 4 loads in flight.
#include <stdexcept>
#include <string>
#include <vector>

#include "../api.h"
#include "common.h"

namespace fluxmpi {
namespace {

constexpr int kThreads = 256;
constexpr int kVec = 8;
constexpr int kIters = 4;
constexpr int kChunk = kThreads * kVec * kIters;  // 8192 elements per workgroup
constexpr int kMaxT = 40;

struct CopyArgs {
  uintptr_t src[kMaxT];
  uintptr_t dst[kMaxT];
  int64_t numel[kMaxT];
  int32_t start[kMaxT + 1];
  int n;
};

// The product type of a copy: fp64 when the source or the destination is fp64 (the caller's double
// scale, unrounded), else fp32 (the scale rounded once to fp32 on the host). One IEEE multiply in
// that type, then one round-to-nearest-even conversion to Tout.
template <typename Tin, typename Tout>
using Prod = std::conditional_t<std::is_same_v<Tin, double> || std::is_same_v<Tout, double>, double, float>;

template <typename Tin, typename Tout>
__device__ __forceinline__ Tout cvt(Tin x, Prod<Tin, Tout> scale) {
  Prod<Tin, Tout> p = static_cast<Prod<Tin, Tout>>(x) * scale;
  // fp16 stores: keep the multiply apart from the conversion. The compiler otherwise contracts the scalar
  // loops' pair into v_fma_mixlo_f16 x, scale, +0, and (-0) * scale + (+0) is +0: the sign of a zero was lost
  if constexpr (std::is_same_v<Tout, f16> && std::is_same_v<Prod<Tin, Tout>, float>) asm("" : "+v"(p));
  return static_cast<Tout>(p);
}

template <typename Tin, typename Tout>
__global__ __launch_bounds__(kThreads) void mt_copy_kernel(CopyArgs a, Prod<Tin, Tout> scale) {
  const int b = blockIdx.x;
  const int t = find_tensor(a.start, a.n, b);
  const int64_t base = static_cast<int64_t>(b - a.start[t]) * kChunk;
  const int64_t n = a.numel[t];
  const int64_t end = base + kChunk < n ? base + kChunk : n;
  const Tin* __restrict__ src = reinterpret_cast<const Tin*>(a.src[t]);
  Tout* __restrict__ dst = reinterpret_cast<Tout*>(a.dst[t]);
  const int tid = threadIdx.x;
  const bool same_bits = sizeof(Tin) == sizeof(Tout);
  if (aligned16(src) && aligned16(dst)) {
    const int64_t nvec = (end - base) / kVec;  // full 8-element vectors in this chunk
    Tin in[kIters][kVec];
#pragma unroll
    for (int k = 0; k < kIters; ++k) {
      const int64_t v = tid + k * kThreads;
      if (v < nvec) load8(src + base + v * kVec, in[k]);
    }
#pragma unroll
    for (int k = 0; k < kIters; ++k) {
      const int64_t v = tid + k * kThreads;
      if (v < nvec) {
        Tout o[kVec];
#pragma unroll
        for (int j = 0; j < kVec; ++j) o[j] = cvt<Tin, Tout>(in[k][j], scale);
        store8(dst + base + v * kVec, o);
      }
    }
    for (int64_t i = base + nvec * kVec + tid; i < end; i += kThreads) dst[i] = cvt<Tin, Tout>(src[i], scale);
  } else {
    (void)same_bits;
    for (int64_t i = base + tid; i < end; i += kThreads) dst[i] = cvt<Tin, Tout>(src[i], scale);
  }
}

template <typename T>
__global__ __launch_bounds__(kThreads) void mt_fill_kernel(CopyArgs a, typename Acc<T>::type value) {
  const int b = blockIdx.x;
  const int t = find_tensor(a.start, a.n, b);
  const int64_t base = static_cast<int64_t>(b - a.start[t]) * kChunk;
  const int64_t n = a.numel[t];
  const int64_t end = base + kChunk < n ? base + kChunk : n;
  T* __restrict__ dst = reinterpret_cast<T*>(a.dst[t]);
  const T val = static_cast<T>(value);
  const int tid = threadIdx.x;
  if (aligned16(dst)) {
    const int64_t nvec = (end - base) / kVec;
    T o[kVec];
#pragma unroll
    for (int j = 0; j < kVec; ++j) o[j] = val;
#pragma unroll
    for (int k = 0; k < kIters; ++k) {
      const int64_t v = tid + k * kThreads;
      if (v < nvec) store8(dst + base + v * kVec, o);
    }
    for (int64_t i = base + nvec * kVec + tid; i < end; i += kThreads) dst[i] = val;
  } else {
    for (int64_t i = base + tid; i < end; i += kThreads) dst[i] = val;
  }
}

__device__ __forceinline__ float wave_sum(float x) { return wave_sum_dpp(x); }  // common.h

template <typename T>
__global__ __launch_bounds__(kThreads) void mt_sumsq_kernel(CopyArgs a, float* out) {
  __shared__ float partial[kThreads / 64];
  const int b = blockIdx.x;
  const int t = find_tensor(a.start, a.n, b);
  const int64_t base = static_cast<int64_t>(b - a.start[t]) * kChunk;
  const int64_t n = a.numel[t];
  const int64_t end = base + kChunk < n ? base + kChunk : n;
  const T* __restrict__ src = reinterpret_cast<const T*>(a.src[t]);
  const int tid = threadIdx.x;
  float acc = 0.f;
  if (aligned16(src)) {
    const int64_t nvec = (end - base) / kVec;
#pragma unroll
    for (int k = 0; k < kIters; ++k) {
      const int64_t v = tid + k * kThreads;
      if (v < nvec) {
        T in[kVec];
        load8(src + base + v * kVec, in);
#pragma unroll
        for (int j = 0; j < kVec; ++j) {
          const float f = static_cast<float>(in[j]);
          acc = fmaf(f, f, acc);
        }
      }
    }
    for (int64_t i = base + nvec * kVec + tid; i < end; i += kThreads) {
      const float f = static_cast<float>(src[i]);
      acc = fmaf(f, f, acc);
    }
  } else {
    for (int64_t i = base + tid; i < end; i += kThreads) {
      const float f = static_cast<float>(src[i]);
      acc = fmaf(f, f, acc);
    }
  }
  acc = wave_sum(acc);
  if ((tid & 63) == 0) partial[tid >> 6] = acc;
  __syncthreads();
  if (tid == 0) {
    float s = 0.f;
#pragma unroll
    for (int w = 0; w < kThreads / 64; ++w) s += partial[w];
    atomicAdd(out, s);
  }
}

// Build launch groups of <= kMaxT non-empty tensors.
template <typename F>
void for_each_group(const std::vector<uintptr_t>& src, const std::vector<uintptr_t>& dst,
                    const std::vector<int64_t>& numel, F&& launch) {
  CopyArgs a{};
  int n = 0;
  int32_t blocks = 0;
  auto flush = [&]() {
    if (n == 0) return;
    a.n = n;
    a.start[n] = blocks;
    launch(a, blocks);
    a = CopyArgs{};
    n = 0;
    blocks = 0;
  };
  for (size_t i = 0; i < numel.size(); ++i) {
    if (numel[i] <= 0) continue;
    const int64_t nb = (numel[i] + kChunk - 1) / kChunk;
    if (nb > (int64_t(1) << 30)) throw std::runtime_error("mt kernel: tensor too large");
    if (n == kMaxT || int64_t(blocks) + nb > (int64_t(1) << 30)) flush();
    a.src[n] = src.empty() ? 0 : src[i];
    a.dst[n] = dst.empty() ? 0 : dst[i];
    a.numel[n] = numel[i];
    a.start[n] = blocks;
    blocks += static_cast<int32_t>(nb);
    ++n;
  }
  flush();
}

}  // namespace

void mt_copy(const std::vector<uintptr_t>& src, const std::vector<uintptr_t>& dst,
             const std::vector<int64_t>& numel, int in_dtype, int out_dtype, double scale,
             hipStream_t stream) {
  if (src.size() != numel.size() || dst.size() != numel.size())
    throw std::runtime_error("mt_copy: list length mismatch");
  const auto bad_in = [&] { return "mt_copy: unsupported input dtype " + std::to_string(in_dtype); };
  const auto bad_out = [&] {
    return in_dtype == kF64 ? std::string("mt_copy: fp64 -> low precision not supported")
                            : "mt_copy: unsupported output dtype " + std::to_string(out_dtype);
  };
  for_each_group(src, dst, numel, [&](const CopyArgs& a, int blocks) {
    dispatch_float64(in_dtype, bad_in, [&](auto in) {
      dispatch_float64(out_dtype, bad_out, [&](auto out) {
        using Tin = typename decltype(in)::type;
        using Tout = typename decltype(out)::type;
        if constexpr (std::is_same_v<Tin, double> && sizeof(Tout) == 2) dispatch_fail(bad_out);
        else mt_copy_kernel<Tin, Tout><<<blocks, kThreads, 0, stream>>>(a, static_cast<Prod<Tin, Tout>>(scale));
      });
    });
    FLUXMPI_HIP_CHECK(hipGetLastError());
  });
}

void mt_fill(const std::vector<uintptr_t>& dst, const std::vector<int64_t>& numel, int dtype,
             double value, hipStream_t stream) {
  for_each_group({}, dst, numel, [&](const CopyArgs& a, int blocks) {
    dispatch_float64(dtype, "mt_fill: unsupported dtype", [&](auto t) {
      // fp64 leaves take the caller's double, the others the value rounded once to fp32
      using T = typename decltype(t)::type;
      mt_fill_kernel<T><<<blocks, kThreads, 0, stream>>>(a, static_cast<typename Acc<T>::type>(value));
    });
    FLUXMPI_HIP_CHECK(hipGetLastError());
  });
}

void mt_sumsq(const std::vector<uintptr_t>& src, const std::vector<int64_t>& numel, int dtype,
              float* out, hipStream_t stream) {
  for_each_group(src, {}, numel, [&](const CopyArgs& a, int blocks) {
    dispatch_float(dtype, "mt_sumsq: unsupported dtype", [&](auto t) {
      mt_sumsq_kernel<typename decltype(t)::type><<<blocks, kThreads, 0, stream>>>(a, out);
    });
    FLUXMPI_HIP_CHECK(hipGetLastError());
  });
}

}  // namespace fluxmpi
