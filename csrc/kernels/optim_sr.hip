// Stochastic rounding as a stand-alone multi-tensor cast, and the step counter of the generator.
//
// mt_stochastic_round: dst (bf16) = sr(src (fp32)) with the rounding and the Philox4x32-10 counter
// layout of optim_sr.h, slot 0 — what the *_sr update kernels do to their parameter store, in their job
// layout (optim_common.h: one workgroup per 4096-element chunk, up to 24 leaves per launch, 16-byte
// vector path when both pointers are aligned and the leaf's offset is a multiple of 8, scalar path for
// the rest and for tails; both draw the same bits for the same element). 6 B per element. No atomics,
// no LDS, no scratch.
//
// sr_advance is the one-thread bookkeeping of the step block {uint32 step, 7 unused} after a step's
// launches, as adam_advance is for beta^t: step += 1, unless the loss scaler called the step off.
// Nothing is read back by the host: the sequence is HIP-graph capturable.
#include <stdexcept>
#include <string>
#include <vector>

#include "../api.h"
#include "optim_common.h"
#include "optim_sr.h"

namespace fluxmpi {
namespace {

template <bool SKIP>
__global__ __launch_bounds__(kThreads) void mt_stochastic_round_kernel(OptArgs a, SrArgs sr,
                                                                       const int32_t* __restrict__ dev_skip) {
  if (step_skipped<SKIP>(dev_skip)) return;
  const Chunk ch = chunk_of(a);
  const SrCtx<true> rc(ch.t, sr);
  bf16* __restrict__ d = reinterpret_cast<bf16*>(a.p[ch.t]);
  const float* __restrict__ x = reinterpret_cast<const float*>(a.g[ch.t]);
  const int tid = threadIdx.x;
  int64_t scalar_from = ch.base;
  if (aligned16(d) && aligned16(x) && rc.vec_ok()) {
    const int64_t nvec = (ch.end - ch.base) / kVec;
#pragma unroll
    for (int k = 0; k < kIters; ++k) {
      const int64_t vi = tid + k * kThreads;
      if (vi < nvec) {
        const int64_t off = ch.base + vi * kVec;
        float xv[kVec]; bf16 dv[kVec];
        load8(x + off, xv);
        const auto rv = rc.vec(off, 0);
#pragma unroll
        for (int j = 0; j < kVec; ++j) dv[j] = rv.at(j).template cast<bf16>(xv[j], 0);
        store8(d + off, dv);
      }
    }
    scalar_from = ch.base + nvec * kVec;
  }
  for (int64_t i = scalar_from + tid; i < ch.end; i += kThreads) d[i] = rc.one(i, 0).template cast<bf16>(x[i], 0);
}

__global__ void sr_advance_kernel(uint32_t* __restrict__ blk, const int32_t* __restrict__ dev_skip) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  if (dev_skip != nullptr && *dev_skip != 0) return;  // a skipped step does not count
  blk[kSrStep] += 1u;
}

}  // namespace

void mt_stochastic_round(const std::vector<uintptr_t>& dst, const std::vector<uintptr_t>& src,
                         const std::vector<int64_t>& numel, const SrHyper& sr, const int32_t* dev_skip,
                         hipStream_t stream) {
  sr_check(sr, numel.size(), "mt_stochastic_round");
  dispatch_bool(dev_skip != nullptr, [&](auto skip) {
    for_each_group(dst, src, {}, {}, {}, {}, numel, [&](const OptArgs& a, int blocks) {
      mt_stochastic_round_kernel<decltype(skip)::value><<<blocks, kThreads, 0, stream>>>(a, sr_args_for(sr, a),
                                                                                         dev_skip);
      FLUXMPI_HIP_CHECK(hipGetLastError());
    });
  });
}

void sr_advance(void* block, const int32_t* dev_skip, hipStream_t stream) {
  if (block == nullptr) throw std::runtime_error("sr_advance: needs the step block");
  sr_advance_kernel<<<1, 64, 0, stream>>>(static_cast<uint32_t*>(block), dev_skip);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace fluxmpi
