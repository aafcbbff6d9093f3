// One-pass backward of conv3 (1x1, 128 -> 512) -> bn3 (+ residual, ReLU) of a ResNet stage-2 identity
// block — gfx950. The Cout = 512, Cin = 128 sibling of conv3bn3_bwd.hip (read that file's header first):
// the same semantics (dx3 from bn_dx.h, bit-identical to the dx pass, rounded to bf16 once into an LDS
// tile that feeds both MFMA products; d_a2 in bf16; one fp32 dW slab per workgroup by plain stores;
// rows past P contribute nothing), reached through the same entry (gemm_bf16 mode 4, N = 128, K = 512).
//
// What differs is the budget. dW [512][128] fp32 is 256 KiB, half of a CU's register file, so exactly
// one workgroup is resident per CU and its accumulator takes 128 registers of every lane:
//   * 8 waves (256 registers each), 32-pixel tiles (tile = blockIdx.x, += gridDim.x);
//   * dW: wave w owns cout 64 w .. + 63 x all 128 cin (acc[4][8] f32x4 = 128 registers), K = the tile's
//     32 pixels, both operands by ds_read_b64_tr_b16 from the pixel-major tiles (rows + 8 elements);
//   * d_a2^T tile = W^T . dx3^T: wave w owns cin 16 w .. + 15 x the 32 pixels, K = 512 in 16 steps.
//     Its 16 W^T fragments would be 64 registers: beside the accumulator and the 41 registers of the
//     next tile's loads in flight that spills. So kWReg = 4 of them stay in registers (16) and the other
//     12 live in LDS in FRAGMENT order (per (k-step, wave) 64 lanes x 16 B, contiguous): each lane reads
//     back its own 16 B by ds_read_b128, lanes 16 B apart, which is conflict-free by construction (a
//     dense [cout][cin] image read by transposed reads cost the stage-1 kernel 8-way conflicts). The
//     fragments are formed once per workgroup: W is staged 128 cout at a time through the tile area
//     as a padded [128][136] image and read with ds_read_b64_tr_b16.
//   * LDS: 12 x 8 KiB of fragments (98 304) + dx3 tile 32 x 520 x 2 (33 280) + a2 tile 32 x 136 x 2
//     (8 704) + the coefficient planes [3][2][64][4] (6 144) = 146 432 B.
//   * the next tile's loads (4 + 4 + 1 16-B vectors and 4 mask bytes per lane) are issued before this
//     tile's MFMAs, as in the stage-1 kernel; with one workgroup per CU they fly only under those.
// Element phase: lane (row wave + 8 i, channel vector lane): a wave reads one whole 1 KiB row per load.
// It runs one half of the channel vector at a time over two rows per dx_vec call, so 12 coefficient
// registers are live instead of 24, and the lane addresses of each phase are re-formed in that phase.
// Ends at 256 VGPRs, no scratch (checked at build time: fluxmpi_amd/_build.py NO_SCRATCH).
//
// Built on the way and lost (compiler's resource remarks): the stage-1 element phase as it is (all 24
// coefficients live, addresses kept from the prologue) spilled 92 B per lane at kWReg = 4, 80 at 3 and
// 64 at 2 (what it spilled first were W^T fragments, re-read from scratch every tile); the half-vector
// element phase alone left 24 B at kWReg = 4 and 8 B at 2. kWReg = 2 (LDS 162 816 B) also ends
// without scratch, at 254 VGPRs, with 2 more fragment reads per tile and wave. Not built: 16 waves
// with 16-pixel tiles (the whole W in LDS, dW through v_mfma_f32_32x32x16_bf16): half the bytes in
// flight per CU, and the coefficient registers do not halve with the tile. Measured: ~139 us per block
// at ResNet-50's 256 x 28 x 28 (profiles/c3b3s2_conv3bn3_s2.md).
#include <stdexcept>
#include <string>

#include "../api.h"
#include "bn_dx.h"
#include "c3_frag.h"
#include "common.h"

namespace fluxmpi {
namespace {

constexpr int kThreads = 512, kWaves = kThreads / 64;
constexpr int kCo = 512, kCi = 128;  // conv3: Cin = 128 -> Cout = 512
constexpr int kTP = 32;              // pixels per tile
constexpr int kLdT = kCo + 8;        // dx3 tile [kTP][kLdT]
constexpr int kLdS = kCi + 8;        // a2 tile [kTP][kLdS]; also the W staging image [kStage][kLdS]
constexpr int kKs = kCo / 32;        // k-steps of the d_a2 product
constexpr int kWReg = 4;             // of them: W^T fragments held in registers, the rest in LDS
constexpr int kFrag = 64 * 16;       // bytes of one fragment: a wave's 64 lanes x 16 B
constexpr int kStage = 128;          // cout rows of W staged at once
constexpr int kWBytes = (kKs - kWReg) * kWaves * kFrag, kTBytes = kTP * kLdT * 2, kABytes = kTP * kLdS * 2;
constexpr int kKBytes = 3 * kCo * static_cast<int>(sizeof(float));  // coefficient planes [3][2][64][4]
constexpr int kSmem = kWBytes + kTBytes + kABytes + kKBytes;        // 146 432 B: one workgroup per CU
static_assert(kSmem <= 160 * 1024 && kStage * kLdS * 2 <= kTBytes + kABytes, "LDS budget");
static_assert(kThreads == kCo, "one lane per channel computes the coefficients");
static_assert(kCo / 64 == kWaves && kCi / 16 == kWaves, "a wave owns 64 cout of dW and 16 cin of d_a2");
constexpr int kRpi = kThreads / (kCo / 8);  // rows of a tile the workgroup covers at once (8)
constexpr int kRows = kTP / kRpi;           // rows of a tile per lane (4)
static_assert(kTP * (kCi / 8) == kThreads, "one a2 vector of a tile per lane");

__global__ __launch_bounds__(kThreads) void conv3bn3_s2_bwd_kernel(C3Args p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  char* wfl = smem;  // fragments [kKs - kWReg][kWaves][64 lanes][16 B]
  bf16* tile = reinterpret_cast<bf16*>(smem + kWBytes);
  bf16* atile = reinterpret_cast<bf16*>(smem + kWBytes + kTBytes);
  float* ksm = reinterpret_cast<float*>(smem + kWBytes + kTBytes + kABytes);
  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int vec = lane, r0 = wave;          // this lane's channel vector and its first row of a tile
  const int arow = t >> 4, avec = t & 15;   // its a2 vector
  const int64_t ntiles = (p.P + kTP - 1) / kTP;

  // the per-channel coefficients -> LDS planes [half][vector][element]
  {
    const DxCoef k = dx_coef(t, p.w, nullptr, p.mean, p.inv, p.sum_dy_xhat, p.sum_dy, 1.f / static_cast<float>(p.P));
    const int slot = ((t >> 2) & 1) * (kCo / 2) + (t >> 3) * 4 + (t & 3);
    ksm[slot] = k.a;
    ksm[kCo + slot] = k.b;
    ksm[2 * kCo + slot] = k.d;
  }
  // this wave's W^T fragments (cin 16 wave .. + 15 x all 512 cout): kStage cout at a time through the
  // (still unused) tile area; the first kWReg stay in registers, the others go to the wave's LDS slots
  bf16x8 wf[kWReg];
  char* myfrag = wfl + wave * kFrag + lane * 16;
#pragma unroll
  for (int c = 0; c < kCo / kStage; ++c) {
#pragma unroll
    for (int i = 0; i < kStage * kCi / 8 / kThreads; ++i) {
      const int v = t + i * kThreads;
      const uint4 q = reinterpret_cast<const uint4*>(p.wt)[c * (kStage * kCi / 8) + v];
      *reinterpret_cast<uint4*>(tile + (v >> 4) * kLdS + (v & 15) * 8) = q;
    }
    __syncthreads();
#pragma unroll
    for (int k4 = 0; k4 < kStage / 32; ++k4) {
      const int ks = c * (kStage / 32) + k4;
      const bf16x8 f = frag_tr(tile, kLdS, 32 * k4, 16 * wave);
      if (ks < kWReg) wf[ks < kWReg ? ks : 0] = f;
      else *reinterpret_cast<bf16x8*>(myfrag + (ks - kWReg) * (kWaves * kFrag)) = f;
    }
    __syncthreads();
  }

  uint4 qd[kRows], qx[kRows], qa;
  unsigned mb[kRows];
  // a tile's base addresses are wave-uniform and a lane's offsets within it 32-bit; rows past P
  // (the partial last tile) re-read the tile's last valid row and are zeroed on the way to LDS
  auto issue = [&](int64_t tl) {
    const int64_t p0 = tl * kTP;
    const int nr = p.P - p0 < kTP ? static_cast<int>(p.P - p0) : kTP;  // >= 1
    const bf16* dyb = p.dy + p0 * kCo;
    const bf16* x3b = p.x3 + p0 * kCo;
    const uint8_t* mkb = p.mask + p0 * (kCo / 8);
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      const int r = r0 + kRpi * i < nr ? r0 + kRpi * i : nr - 1;
      const unsigned v = static_cast<unsigned>(r) * (kCo / 8) + vec;
      qd[i] = reinterpret_cast<const uint4*>(dyb)[v];
      qx[i] = reinterpret_cast<const uint4*>(x3b)[v];
      mb[i] = mkb[v];
    }
    const int ra = arow < nr ? arow : nr - 1;
    qa = reinterpret_cast<const uint4*>(p.a2 + p0 * kCi)[static_cast<unsigned>(ra) * (kCi / 8) + avec];
  };

  f32x4 acc[4][8];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  int64_t tl = blockIdx.x;
  if (tl < ntiles) issue(tl);
  for (; tl < ntiles; tl += gridDim.x) {
    const int64_t p0 = tl * kTP;
    // an offset the compiler cannot see through: the loop-invariant coefficient and fragment reads
    // stay in the loop instead of being hoisted into VGPRs held across it
    int opq = 0;
    asm volatile("" : "+v"(opq));
    const float4* kl = reinterpret_cast<const float4*>(ksm + opq) + vec;
    const int nr = p.P - p0 < kTP ? static_cast<int>(p.P - p0) : kTP;  // the tile's valid rows (uniform)
    // dx3 of this lane's vectors -> LDS (rows past P: zeros, not the constant term d). One half of the
    // channel vector at a time, two rows per dx_vec call (elements 0-3: row i, 4-7: row i + 1, each
    // with its channel's coefficients): 12 coefficient registers live instead of 24
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const float4 ka = kl[hf * (kCo / 8)], kb = kl[kCo / 4 + hf * (kCo / 8)], kd = kl[kCo / 2 + hf * (kCo / 8)];
      DxCoef rk[8];
      rk[0] = rk[4] = DxCoef{ka.x, kb.x, kd.x, 0.f};
      rk[1] = rk[5] = DxCoef{ka.y, kb.y, kd.y, 0.f};
      rk[2] = rk[6] = DxCoef{ka.z, kb.z, kd.z, 0.f};
      rk[3] = rk[7] = DxCoef{ka.w, kb.w, kd.w, 0.f};
#pragma unroll
      for (int i = 0; i < kRows; i += 2) {
        bf16 td[2][8], tx[2][8];
        __builtin_memcpy(td[0], &qd[i], 16);
        __builtin_memcpy(td[1], &qd[i + 1], 16);
        __builtin_memcpy(tx[0], &qx[i], 16);
        __builtin_memcpy(tx[1], &qx[i + 1], 16);
        float d[8], xv[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          d[j] = static_cast<float>(td[j >> 2][4 * hf + (j & 3)]);
          xv[j] = static_cast<float>(tx[j >> 2][4 * hf + (j & 3)]);
        }
        const unsigned bits = ((mb[i] >> (4 * hf)) & 15u) | (((mb[i + 1] >> (4 * hf)) & 15u) << 4);
        dx_vec<bf16, 3, false>(d, xv, d, bits, rk);
#pragma unroll
        for (int h = 0; h < 2; ++h) {
          const bool ok = r0 + kRpi * (i + h) < nr;
          bf16x4 o;
#pragma unroll
          for (int j = 0; j < 4; ++j) o[j] = ok ? static_cast<bf16>(xv[4 * h + j]) : static_cast<bf16>(0.f);
          *reinterpret_cast<bf16x4*>(tile + (r0 + kRpi * (i + h)) * kLdT + vec * 8 + 4 * hf) = o;
        }
        __builtin_amdgcn_sched_barrier(0);  // one pair at a time: interleaved, the rows' fp32 temporaries spill
      }
    }
    {
      int tq = t;
      asm volatile("" : "+v"(tq));  // (as lq below)
      *reinterpret_cast<uint4*>(atile + (tq >> 4) * kLdS + (tq & 15) * 8) = (tq >> 4) < nr ? qa : uint4{0u, 0u, 0u, 0u};
    }
    __syncthreads();
    // the next tile's loads fly under this tile's MFMAs
    if (tl + gridDim.x < ntiles) issue(tl + gridDim.x);

    // d_a2^T [cin][pixel] = W^T [cin][cout] . dx3^T [cout][pixel]: this wave's 16 cin x the 32 pixels
    {
      f32x4 da[kTP / 16];
#pragma unroll
      for (int i = 0; i < kTP / 16; ++i) da[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      // the lane's addresses of this phase are formed here from a copy of the lane index the compiler
      // cannot see through: kept from the prologue they are registers held across the element phase
      int lq = lane;
      asm volatile("" : "+v"(lq));
      const bf16* brow = tile + (lq & 15) * kLdT + 8 * (lq >> 4);
      const char* fr = wfl + wave * kFrag + lq * 16;
#pragma unroll
      for (int ks = 0; ks < kKs; ++ks) {
        const bf16x8 fa = ks < kWReg ? wf[ks < kWReg ? ks : 0]
                                     : *reinterpret_cast<const bf16x8*>(fr + (ks - kWReg) * (kWaves * kFrag));
#pragma unroll
        for (int i = 0; i < kTP / 16; ++i) {
          const bf16x8 fb = *reinterpret_cast<const bf16x8*>(brow + 16 * i * kLdT + 32 * ks);
          da[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb, da[i], 0, 0, 0);
        }
      }
      // da[i][r] = d_a2[pixel p0 + 16 i + (lane & 15)][cin 16 wave + 4 (lane >> 4) + r]
      // (uniform tile base + a 32-bit lane offset: no 64-bit per-lane address held across the loop)
      bf16* ob = p.d_a2 + p0 * kCi;
      const unsigned oo = static_cast<unsigned>(lq & 15) * kCi + 16 * wave + 4 * (lq >> 4);
#pragma unroll
      for (int i = 0; i < kTP / 16; ++i) {
        if (16 * i + (lq & 15) < nr) {
          bf16x4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = static_cast<bf16>(da[i][r]);
          *reinterpret_cast<bf16x4*>(ob + oo + 16 * i * kCi) = o;
        }
      }
    }
    // dW [cout][cin] += dx3^T [cout][pixel] . a2 [pixel][cin]: this wave's cout 64 wave .. + 63 x all 128
    // cin (the four dx3^T fragments held, one a2 fragment at a time: all eight at once are 32 registers)
    {
      bf16x8 fa[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = frag_tr(tile, kLdT, 0, wave * 64 + 16 * i);
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        const bf16x8 fb = frag_tr(atile, kLdS, 0, 16 * j);
#pragma unroll
        for (int i = 0; i < 4; ++i) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb, acc[i][j], 0, 0, 0);
      }
    }
    __syncthreads();  // every wave is done with the tiles before the next iteration overwrites them
  }

  // acc[i][j][r] = dW[cout wave * 64 + 16 i + 4 (lane >> 4) + r][cin 16 j + (lane & 15)]
  float* slab = p.ws + static_cast<int64_t>(blockIdx.x) * (kCo * kCi);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 8; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        slab[static_cast<unsigned>((wave * 64 + 16 * i + 4 * (lane >> 4) + r) * kCi + 16 * j + (lane & 15))] = acc[i][j][r];
}

}  // namespace

void conv3bn3_s2_launch(const C3Args& p, int slabs, hipStream_t stream) {
  allow_dynamic_lds(reinterpret_cast<const void*>(&conv3bn3_s2_bwd_kernel), kSmem);
  conv3bn3_s2_bwd_kernel<<<static_cast<unsigned>(slabs), kThreads, kSmem, stream>>>(p);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace fluxmpi
