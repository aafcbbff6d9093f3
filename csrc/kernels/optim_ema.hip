// Exponential moving average of the weights (DDP(ema=...), optimisers.ema_update), fused and on device.
//
//   e <- e + omd * (x - e)        omd = 1 - decay_t
//
// in exactly this form: x == e leaves e's bits alone whatever omd is, and no product of two large
// terms is formed. x is the fp32 master of a leaf that has one, else the parameter (fp32, bf16, fp16,
// fp64) taken to the compute type; e is stored in the compute type (fp32; fp64 for fp64 sources).
//
// mt_ema is one streaming pass in the update kernels' job layout (optim_common.h: one workgroup per
// 4096-element chunk, up to 24 leaves per launch, 16-byte vector path when both pointers are aligned,
// scalar path for unaligned leaves and tails): 12 B per element behind an fp32 master. The engine
// enqueues it right behind a bucket's update launch, when the master it reads was written a moment
// ago. Two wave-uniform words can call a launch off before it loads tensor data: the loss scaler's
// skip flag (step_skipped) and the EMA block's `hold` (an optimiser step that is not an EMA step:
// DDP(ema=EMA(every=k))). No atomics, no LDS, no scratch.
//
// ema_advance is the one-thread bookkeeping of the EMA device block after a step's launches, as
// adam_advance is for beta^t: update / step counters, the next step's hold, the warmed-up decay.
// Nothing is read back by the host: the sequence is HIP-graph capturable.
#include <stdexcept>
#include <string>
#include <vector>

#include "../api.h"
#include "optim_common.h"

namespace fluxmpi {
namespace {

// words of the EMA device block (api.h: ema_advance)
constexpr int kEmaOmd = 0, kEmaDecay = 1, kEmaUpdates = 2, kEmaSince = 3, kEmaHold = 4;

template <typename C>
__device__ __forceinline__ C ema_elem(C e, C x, C omd) {
#pragma clang fp contract(off)  // three roundings, as written: the reference's bits
  const C d = x - e;
  const C s = omd * d;
  return e + s;
}

template <typename X, bool SKIP>
__global__ __launch_bounds__(kThreads) void mt_ema_kernel(OptArgs a, double omd_host,
                                                          const int32_t* __restrict__ dev_block,
                                                          const int32_t* __restrict__ dev_skip) {
  using C = typename Comp<X>::type;
  if (step_skipped<SKIP>(dev_skip)) return;
  C omd = static_cast<C>(omd_host);
  if (dev_block != nullptr) {  // engine mode: the device value wins, as dev_hyper does for lr
    if (dev_block[kEmaHold] != 0) return;
    omd = static_cast<C>(__builtin_bit_cast(float, dev_block[kEmaOmd]));
  }
  const Chunk ch = chunk_of(a);
  C* __restrict__ e = reinterpret_cast<C*>(a.p[ch.t]);
  const X* __restrict__ x = reinterpret_cast<const X*>(a.g[ch.t]);
  const int tid = threadIdx.x;
  int64_t scalar_from = ch.base;
  if (aligned16(e) && aligned16(x)) {
    const int64_t nvec = (ch.end - ch.base) / kVec;
#pragma unroll
    for (int k = 0; k < kIters; ++k) {
      const int64_t vi = tid + k * kThreads;
      if (vi < nvec) {
        const int64_t off = ch.base + vi * kVec;
        X xv[kVec]; C ev[kVec];
        load8(x + off, xv);
        load8(e + off, ev);
#pragma unroll
        for (int j = 0; j < kVec; ++j) ev[j] = ema_elem(ev[j], static_cast<C>(xv[j]), omd);
        store8(e + off, ev);
      }
    }
    scalar_from = ch.base + nvec * kVec;
  }
  for (int64_t i = scalar_from + tid; i < ch.end; i += kThreads) e[i] = ema_elem(e[i], static_cast<C>(x[i]), omd);
}

__global__ void ema_advance_kernel(int32_t* __restrict__ blk, float decay, int warmup, int every,
                                   const int32_t* __restrict__ dev_skip) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (dev_skip != nullptr && *dev_skip != 0) return;  // a skipped step does not count
  int n = blk[kEmaUpdates], k = blk[kEmaSince];
  if (blk[kEmaHold] == 0) {
    n += 1;
    k = 0;
  } else {
    k += 1;
  }
  float d = decay;
  if (warmup) d = fminf(decay, (1.f + static_cast<float>(n)) / (10.f + static_cast<float>(n)));
  float* f = reinterpret_cast<float*>(blk);
  f[kEmaOmd] = 1.f - d;
  f[kEmaDecay] = d;
  blk[kEmaUpdates] = n;
  blk[kEmaSince] = k;
  blk[kEmaHold] = k + 1 < every ? 1 : 0;
}

}  // namespace

void mt_ema(const std::vector<uintptr_t>& ema, const std::vector<uintptr_t>& src, const std::vector<int64_t>& numel,
            int src_dtype, double omd, const int32_t* dev_block, const int32_t* dev_skip, hipStream_t stream) {
  dispatch_float64(
      src_dtype, [&] { return "mt_ema: unsupported source dtype " + std::to_string(src_dtype); }, [&](auto x) {
        dispatch_bool(dev_skip != nullptr, [&](auto skip) {
          for_each_group(ema, src, {}, {}, {}, {}, numel, [&](const OptArgs& a, int blocks) {
            mt_ema_kernel<typename decltype(x)::type, decltype(skip)::value><<<blocks, kThreads, 0, stream>>>(
                a, omd, dev_block, dev_skip);
            FLUXMPI_HIP_CHECK(hipGetLastError());
          });
        });
      });
}

void ema_advance(void* block, float decay, int warmup, int every, const int32_t* dev_skip, hipStream_t stream) {
  if (block == nullptr) throw std::runtime_error("ema_advance: needs the EMA block");
  if (every < 1) throw std::runtime_error("ema_advance: every must be >= 1");
  ema_advance_kernel<<<1, 64, 0, stream>>>(static_cast<int32_t*>(block), decay, warmup, every, dev_skip);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace fluxmpi
