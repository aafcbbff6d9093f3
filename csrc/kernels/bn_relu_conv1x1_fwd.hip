// bn2 apply + ReLU + conv3 (1x1 expansion, Cin -> 4 Cin) forward of a ResNet bottleneck in one
// streaming kernel — gfx950. (Cin, Cout) = (64, 256) and (128, 512), bf16 NHWC.
//
// Unfused, bn_norm_kernel reads c2 and writes a2 = relu(bn2(c2)), and the expansion GEMM reads a2
// straight back, runs 2 to 4 k-tiles per 128 x 128 tile (mostly prologue and epilogue) and adds
// 2 x 128 float atomics per tile for bn3's statistics. Here a persistent workgroup owns the whole
// filter in registers and loops over 32-pixel tiles (tile = blockIdx.x, += gridDim.x):
//   * lane (row r, channel vector v) holds one 16-B vector of c2 per tile; the next tile's load was
//     issued before this tile's MFMAs;
//   * a2 = relu(fmaf(x, scale, shift)) rounded to bf16: scale / shift are bn_finalize_fwd_kernel's
//     (bit-identical to bn_norm_kernel's prologue), kept in LDS planes a lane reads 16 B apart from
//     its neighbours; the vector goes to global (the backward still reads a2) and into the LDS
//     tile [32][Cin + 8];
//   * c3^T tile = W . a2^T: wave w owns cout 64 w .. + 63 x the 32 pixels. A = W fragments (16
//     contiguous bytes of the K-major [Cout][Cin] filter per lane: loaded from global once, 32 / 64
//     VGPRs); B = a2 rows by ds_read_b128. The transposed product leaves a lane 4 consecutive cout of
//     one pixel: 8-B writes into the LDS staging tile [32][Cout + 8];
//   * the staging tile goes out as 16-B vectors, a wave storing whole rows (the tile is one
//     contiguous 16 / 32 KiB piece of c3). The lane that stores a vector also adds its ROUNDED
//     values to its per-channel sum and sum of squares: a lane keeps the same 8 channels for the
//     whole kernel, 16 accumulators.
// At the end the workgroup reduces the accumulators through LDS and issues one atomicAdd per column
// and moment into shard blockIdx.x % 64 of the BatchNorm workspace [64][2][Cout]. Rows past P (the
// partial last tile) are zero in the a2 tile, so they add nothing to the sums, and are written to
// neither output.
#include <stdexcept>
#include <string>

#include "../api.h"
#include "c3_frag.h"
#include "common.h"

namespace fluxmpi {
namespace {

constexpr int kTP = 32;      // pixels per tile
constexpr int kShards = 64;  // must match batchnorm.hip

template <int CIN>
struct Cfg {
  static constexpr int kCo = 4 * CIN;
  static constexpr int kWaves = kCo / 64;  // 64 cout per wave
  static constexpr int kThreads = 64 * kWaves;
  static constexpr int kVecIn = CIN / 8, kVecOut = kCo / 8;  // 16-B vectors per row of c2 / c3
  // LDS row strides in elements: + 8 keeps 16-B alignment and staggers the rows over the banks
  static constexpr int kLdA = CIN + 8, kLdC = kCo + 8;
  static constexpr int kKS = CIN / 32;             // 32-deep k-steps
  static constexpr int kRpp = kThreads / kVecOut;  // rows of the staging tile the workgroup stores at once (8)
  static constexpr int kPasses = kTP / kRpp;
  static_assert(kThreads * 8 == kTP * CIN, "one c2 vector per lane and tile");
  static_assert(kThreads % kVecIn == 0 && kThreads % kVecOut == 0, "a lane keeps its channels across tiles");
  static_assert(kThreads == kCo, "one lane per column issues the atomics");
  static_assert(kRpp * 2 * kCo * 4 <= kTP * kLdC * 2, "the final reduction reuses the staging tile");
};

struct Args {
  const bf16* c2;      // [P][Cin]
  const float* scale;  // [Cin]
  const float* shift;  // [Cin]
  const bf16* wt;      // [Cout][Cin]
  bf16* a2;            // [P][Cin]
  bf16* c3;            // [P][Cout]
  float* stats;        // [64][2][Cout]
  int64_t P;
};

template <int CIN, int MINW>
__global__ __launch_bounds__(Cfg<CIN>::kThreads, MINW) void bn_relu_conv1x1_fwd_kernel(Args p) {
  using C = Cfg<CIN>;
  constexpr int kCo = C::kCo;
  __shared__ __attribute__((aligned(16))) bf16 atile[kTP * C::kLdA];
  __shared__ __attribute__((aligned(16))) bf16 ctile[kTP * C::kLdC];
  // scale / shift as [2][2][Cin / 8][4]: a lane's float4 reads of its channel vector are 16 B from its
  // neighbours' (see conv3bn3_bwd.hip on what 32 B apart cost)
  __shared__ __attribute__((aligned(16))) float ksm[2 * CIN];
  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int row = t / C::kVecIn, cv = t % C::kVecIn;     // this lane's c2 / a2 vector of a tile
  const int orow = t / C::kVecOut, ov = t % C::kVecOut;  // its first c3 vector of a tile (the others kRpp rows on)
  const int64_t ntiles = (p.P + kTP - 1) / kTP;

  for (int c = t; c < CIN; c += C::kThreads) {
    const int slot = ((c >> 2) & 1) * (CIN / 2) + (c >> 3) * 4 + (c & 3);  // [half][vector][element]
    ksm[slot] = p.scale[c];
    ksm[CIN + slot] = p.shift[c];
  }
  // this wave's filter fragments (cout 64 wave .. + 63 x all Cin), straight from global, once
  bf16x8 wf[4][C::kKS];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int ks = 0; ks < C::kKS; ++ks)
      wf[j][ks] = *reinterpret_cast<const bf16x8*>(p.wt + (64 * wave + 16 * j + (lane & 15)) * CIN + 32 * ks +
                                                   8 * (lane >> 4));
  __syncthreads();

  uint4 qc;
  // a tile's base address is wave-uniform and a lane's offset within it 32-bit; rows past P (the
  // partial last tile) re-read the tile's last valid row and are zeroed on the way to LDS
  auto issue = [&](int64_t tl) {
    const int64_t p0 = tl * kTP;
    const int nr = p.P - p0 < kTP ? static_cast<int>(p.P - p0) : kTP;  // >= 1
    const int r = row < nr ? row : nr - 1;
    qc = reinterpret_cast<const uint4*>(p.c2 + p0 * CIN)[static_cast<unsigned>(r) * C::kVecIn + cv];
  };

  float s[8], q[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) s[j] = q[j] = 0.f;

  int64_t tl = blockIdx.x;
  if (tl < ntiles) issue(tl);
  for (; tl < ntiles; tl += gridDim.x) {
    const int64_t p0 = tl * kTP;
    const int nr = p.P - p0 < kTP ? static_cast<int>(p.P - p0) : kTP;  // the tile's valid rows (uniform)
    // an offset the compiler cannot see through: the loop-invariant coefficient reads stay in the
    // loop instead of being hoisted into 16 VGPRs held across it
    int opq = 0;
    asm volatile("" : "+v"(opq));
    const float4* kl = reinterpret_cast<const float4*>(ksm + opq) + cv;
    float sc[8], sh[8];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const float4 ka = kl[hf * (CIN / 8)], kb = kl[(CIN / 4) + hf * (CIN / 8)];
      sc[4 * hf + 0] = ka.x; sc[4 * hf + 1] = ka.y; sc[4 * hf + 2] = ka.z; sc[4 * hf + 3] = ka.w;
      sh[4 * hf + 0] = kb.x; sh[4 * hf + 1] = kb.y; sh[4 * hf + 2] = kb.z; sh[4 * hf + 3] = kb.w;
    }
    // a2 of this lane's vector -> global and LDS (rows past P: zeros in LDS, nothing in global)
    {
      bf16 tx[8];
      __builtin_memcpy(tx, &qc, 16);
      const bool ok = row < nr;
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        float f = fmaf(static_cast<float>(tx[j]), sc[j], sh[j]);  // == norm_vec of batchnorm.hip
        f = f > 0.f ? f : 0.f;
        o[j] = ok ? static_cast<bf16>(f) : static_cast<bf16>(0.f);
      }
      *reinterpret_cast<bf16x8*>(atile + row * C::kLdA + cv * 8) = o;
      if (ok) *reinterpret_cast<bf16x8*>(p.a2 + p0 * CIN + static_cast<unsigned>(row * CIN + cv * 8)) = o;
    }
    __syncthreads();
    // the next tile's load flies under this tile's MFMAs and stores
    if (tl + gridDim.x < ntiles) issue(tl + gridDim.x);

    // c3^T [cout][pixel] = W [cout][cin] . a2^T [cin][pixel]: this wave's 64 cout x the 32 pixels
    // (16 pixels at a time: both halves' accumulators and B fragments live at once cost the 128 -> 512
    // kernel its second workgroup per CU)
    {
      const bf16* brow = atile + (lane & 15) * C::kLdA + 8 * (lane >> 4);
      bf16* crow = ctile + (lane & 15) * C::kLdC + 64 * wave + 4 * (lane >> 4);
#pragma unroll
      for (int i = 0; i < kTP / 16; ++i) {
        f32x4 acc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[j] = f32x4{0.f, 0.f, 0.f, 0.f};
        // one B fragment ahead of the MFMAs, no more (all kKS at once are 16 VGPRs at Cin = 128)
        bf16x8 fb = *reinterpret_cast<const bf16x8*>(brow + 16 * i * C::kLdA);
#pragma unroll
        for (int ks = 0; ks < C::kKS; ++ks) {
          bf16x8 fn = fb;
          if (ks + 1 < C::kKS) fn = *reinterpret_cast<const bf16x8*>(brow + 16 * i * C::kLdA + 32 * (ks + 1));
#pragma unroll
          for (int j = 0; j < 4; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[j][ks], fb, acc[j], 0, 0, 0);
          __builtin_amdgcn_sched_barrier(0);
          fb = fn;
        }
        // acc[j][r] = c3[pixel 16 i + (lane & 15)][cout 64 wave + 16 j + 4 (lane >> 4) + r]
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          bf16x4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = static_cast<bf16>(acc[j][r]);
          *reinterpret_cast<bf16x4*>(crow + 16 * i * C::kLdC + 16 * j) = o;
        }
        __builtin_amdgcn_sched_barrier(0);
      }
    }
    __syncthreads();
    // the staging tile -> c3 in whole rows, and the rounded values into this lane's sums (the next
    // iteration's first barrier lies between these reads and the next writes of the staging tile)
    {
      // (a uniform base per pass + one lane offset, a uniform row limit per pass: per-pass lane
      // offsets and row numbers held across the loop are what spilled)
      const bf16* cb = ctile + orow * C::kLdC + ov * 8;
      const unsigned oo = static_cast<unsigned>(orow * kCo + ov * 8);
#pragma unroll
      for (int ps = 0; ps < C::kPasses; ++ps) {
        const bf16x8 v = *reinterpret_cast<const bf16x8*>(cb + C::kRpp * ps * C::kLdC);
        bf16* ob = p.c3 + (p0 + C::kRpp * ps) * kCo;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const float f = static_cast<float>(v[j]);
          s[j] += f;
          q[j] = fmaf(f, f, q[j]);
        }
        if (orow < nr - C::kRpp * ps) *reinterpret_cast<bf16x8*>(ob + oo) = v;
      }
    }
  }

  // the kRpp lanes of a channel vector meet in LDS (over the staging tile); one atomic per column and moment
  __syncthreads();
  float* red = reinterpret_cast<float*>(ctile);  // [kRpp][2][Cout]
#pragma unroll
  for (int hf = 0; hf < 2; ++hf) {
    *reinterpret_cast<float4*>(red + (orow * 2 + 0) * kCo + ov * 8 + 4 * hf) =
        float4{s[4 * hf], s[4 * hf + 1], s[4 * hf + 2], s[4 * hf + 3]};
    *reinterpret_cast<float4*>(red + (orow * 2 + 1) * kCo + ov * 8 + 4 * hf) =
        float4{q[4 * hf], q[4 * hf + 1], q[4 * hf + 2], q[4 * hf + 3]};
  }
  __syncthreads();
  float ts = 0.f, tq = 0.f;
#pragma unroll
  for (int g = 0; g < C::kRpp; ++g) {
    ts += red[(g * 2 + 0) * kCo + t];
    tq += red[(g * 2 + 1) * kCo + t];
  }
  float* shard = p.stats + static_cast<size_t>(blockIdx.x % kShards) * 2 * kCo;
  atomicAdd(shard + t, ts);
  atomicAdd(shard + kCo + t, tq);
}

template <int CIN, int MINW>
void launch(const Args& a, hipStream_t stream) {
  using C = Cfg<CIN>;
  auto k = bn_relu_conv1x1_fwd_kernel<CIN, MINW>;
  // one resident round, never more workgroups than tiles
  const int64_t ntiles = (a.P + kTP - 1) / kTP;
  const int64_t slots = resident_blocks(reinterpret_cast<const void*>(k), C::kThreads, 0);
  k<<<static_cast<unsigned>(ntiles < slots ? ntiles : slots), C::kThreads, 0, stream>>>(a);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace

bool bn_relu_conv1x1_fwd_supported(int Cin, int Cout) { return (Cin == 64 && Cout == 256) || (Cin == 128 && Cout == 512); }

void bn_relu_conv1x1_fwd(const void* c2, const float* scale, const float* shift, const void* wt, void* a2, void* c3,
                         float* stats, int64_t P, int Cin, int Cout, hipStream_t stream) {
  if (!bn_relu_conv1x1_fwd_supported(Cin, Cout) || P < 1 || P > (INT64_MAX >> 12))
    throw std::runtime_error("bn_relu_conv1x1_fwd: needs (Cin, Cout) = (64, 256) or (128, 512) and P >= 1; got P=" +
                             std::to_string(P) + ", Cin=" + std::to_string(Cin) + ", Cout=" + std::to_string(Cout));
  if (c2 == nullptr || scale == nullptr || shift == nullptr || wt == nullptr || a2 == nullptr || c3 == nullptr ||
      stats == nullptr)
    throw std::runtime_error("bn_relu_conv1x1_fwd: c2, scale, shift, W, a2, c3 and the statistics workspace are all required");
  uintptr_t bits = 0;
  for (const void* q : {c2, static_cast<const void*>(scale), static_cast<const void*>(shift), wt,
                        static_cast<const void*>(a2), static_cast<const void*>(c3), static_cast<const void*>(stats)})
    bits |= reinterpret_cast<uintptr_t>(q);
  if ((bits & 15u) != 0) throw std::runtime_error("bn_relu_conv1x1_fwd: operands must be 16-byte aligned");
  const Args a{static_cast<const bf16*>(c2), scale, shift, static_cast<const bf16*>(wt), static_cast<bf16*>(a2),
               static_cast<bf16*>(c3), stats, P};
  if (Cin == 64) launch<64, 2>(a, stream);
  else launch<128, 4>(a, stream);
}

}  // namespace fluxmpi
