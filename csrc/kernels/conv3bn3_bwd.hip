// One-pass backward of conv3 (1x1, 64 -> 256) -> bn3 (+ residual, ReLU) of a ResNet stage-1
// identity block — gfx950.
//
// Unfused, the largest activations of the network are streamed three times: bn3's dx pass reads
// (dy, x3, mask) and writes dx3 [P][256]; conv3's input gradient and its weight gradient each
// read dx3 again. Both GEMMs are tiny in FLOPs for those bytes (K = 256 on one, N = 64 on the
// other). This kernel reads (dy, x3, mask, a2) once, forms dx3 in registers with the dx pass's own
// arithmetic (bn_dx.h: bit-identical to what bn_bwd_dx_kernel would have stored), rounds it to
// bf16 into an LDS tile and feeds both MFMA products from that tile:
//   d_a2 [P][64]  = dx3 [P][256] . W [256][64]                       (bf16, written per tile)
//   dW  [256][64] = dx3^T . a2 [P][64]                               (fp32, in registers)
// dx3 itself never reaches memory.
//
// Structure: persistent workgroups of 4 waves, two per CU (232 VGPRs, 56 KiB of LDS each), each
// looping over 32-pixel tiles (tile = blockIdx.x, += gridDim.x); the per-channel dx coefficients
// stay LDS-resident, in planes a lane reads without bank conflicts. Per tile:
//   * the tile's loads (4 + 4 + 1 16-B vectors and 4 mask bytes per lane) were issued before the
//     previous tile's MFMAs, so they fly under them (and under the CU's other workgroup);
//   * lane (row r, channel vector v): dx3 = dx_vec(...) for its 8 channels of 4 rows, bf16 -> LDS;
//   * d_a2^T tile = W^T . dx3^T: wave w owns cin 16 w .. + 15 x the 32 pixels (A = W^T: eight
//     fragments by ds_read_b64_tr_b16 from the [cout][cin] image, once, kept in registers; B = dx3
//     rows by ds_read_b128; the transposed product leaves a lane 4 consecutive cin of one pixel:
//     8-B stores);
//   * dW tile: wave w owns cout 64 w .. + 63 x all 64 cin, K = the tile's 32 pixels (both
//     operands pixel-major in LDS -> ds_read_b64_tr_b16), accumulated across all its tiles.
// (64-pixel tiles need > 256 VGPRs at 4 waves; 8 waves per workgroup leave 128 each: both spill.)
// A workgroup stores its dW partial as one fp32 slab ws[blockIdx.x][256][64] (plain stores; a
// workgroup without tiles stores zeros) and gemm_splitk_reduce sums the slabs: no float atomics,
// no grid barrier. Rows past P are zero in both tiles, so the partial last tile adds nothing.
// The stage-2 form (128 -> 512, one workgroup per CU) is conv3bn3_s2_bwd.hip; conv3bn3_bwd below checks
// the problem for both and launches the one that (N, K) names.
#include <stdexcept>
#include <string>

#include "../api.h"
#include "bn_dx.h"
#include "c3_frag.h"
#include "common.h"

namespace fluxmpi {
namespace {

constexpr int kThreads = 256;
constexpr int kCo = 256, kCi = 64;  // conv3: Cin = 64 -> Cout = 256
constexpr int kTP = 32;             // pixels per tile
// LDS row strides in elements: + 8 keeps 16-B alignment and staggers the rows over the banks
constexpr int kLdT = kCo + 8;  // dx3 tile [kTP][kLdT]
constexpr int kLdS = kCi + 8;  // a2 tile [kTP][kLdS]
constexpr int kLdW = kCi;      // W image [kCo][kLdW] (dense: the padding's 4 KiB hold the coefficients)
constexpr int kWBytes = kCo * kLdW * 2, kTBytes = kTP * kLdT * 2, kABytes = kTP * kLdS * 2;
// coefficients a / b / d as [3][2][32 channel vectors][4]: a lane's float4 reads of its channel
// vector are 16 B apart from its neighbours' (as an array of DxCoef they were 128 B apart: a
// 16-way bank conflict on every read, which was most of the kernel's time)
constexpr int kKBytes = 3 * kCo * static_cast<int>(sizeof(float));
constexpr int kSmem = kWBytes + kTBytes + kABytes + kKBytes;  // 57 344 B: two workgroups per CU
static_assert(kThreads == kCo, "one lane per channel computes the coefficients");
constexpr int kRpi = kThreads / (kCo / 8);  // rows of a tile the workgroup covers at once (8)
constexpr int kRows = kTP / kRpi;           // rows of a tile per lane (4)
constexpr int kAv = kTP * (kCi / 8) / kThreads;  // a2 vectors of a tile per lane (1)

__device__ __forceinline__ void ld4(const float* __restrict__ p, float* v) {
  const float4 a = *reinterpret_cast<const float4*>(p);
  v[0] = a.x; v[1] = a.y; v[2] = a.z; v[3] = a.w;
}

__global__ __launch_bounds__(kThreads, 2) void conv3bn3_bwd_kernel(C3Args p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  bf16* wimg = reinterpret_cast<bf16*>(smem);
  bf16* tile = reinterpret_cast<bf16*>(smem + kWBytes);
  bf16* atile = reinterpret_cast<bf16*>(smem + kWBytes + kTBytes);
  float* ksm = reinterpret_cast<float*>(smem + kWBytes + kTBytes + kABytes);
  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int vec = t & 31, r0 = t >> 5;  // this lane's channel vector and its first row of a tile
  const int arow = t >> 3, avec = t & 7;  // its a2 vector (kAv > 1: the others 32 rows on)
  const int64_t ntiles = (p.P + kTP - 1) / kTP;

  // W -> LDS image [cout][kLdS] (once)
#pragma unroll
  for (int i = 0; i < kCo * kCi / 8 / kThreads; ++i) {
    const int v = t + i * kThreads;
    const uint4 q = reinterpret_cast<const uint4*>(p.wt)[v];
    *reinterpret_cast<uint4*>(wimg + (v >> 3) * kLdW + (v & 7) * 8) = q;
  }
  // the per-channel coefficients -> LDS (in registers they would hold 24 VGPRs across the loop)
  {
    const DxCoef k = dx_coef(t, p.w, nullptr, p.mean, p.inv, p.sum_dy_xhat, p.sum_dy, 1.f / static_cast<float>(p.P));
    const int slot = ((t >> 2) & 1) * 128 + (t >> 3) * 4 + (t & 3);  // [half][vector][element]
    ksm[slot] = k.a;
    ksm[kCo + slot] = k.b;
    ksm[2 * kCo + slot] = k.d;
  }
  __syncthreads();

  // this wave's W^T fragments (cin 16 wave .. + 15 x all 256 cout) stay in registers: read from the
  // dense image every tile, their 8-way bank conflicts were half of the kernel's time
  bf16x8 wf[kCo / 32];
#pragma unroll
  for (int ks = 0; ks < kCo / 32; ++ks) wf[ks] = frag_tr(wimg, kLdW, 32 * ks, 16 * wave);

  uint4 qd[kRows], qx[kRows], qa[kAv];
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
#pragma unroll
    for (int i = 0; i < kAv; ++i) {
      const int ra = arow + 32 * i < nr ? arow + 32 * i : nr - 1;
      qa[i] = reinterpret_cast<const uint4*>(p.a2 + p0 * kCi)[static_cast<unsigned>(ra) * (kCi / 8) + avec];
    }
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  int64_t tl = blockIdx.x;
  if (tl < ntiles) issue(tl);
  for (; tl < ntiles; tl += gridDim.x) {
    const int64_t p0 = tl * kTP;
    // an offset the compiler cannot see through: the loop-invariant coefficient reads stay in
    // the loop instead of being hoisted into 24 VGPRs held across it
    int opq = 0;
    asm volatile("" : "+v"(opq));
    const float4* kl = reinterpret_cast<const float4*>(ksm + opq) + vec;
    DxCoef rk[8];
#pragma unroll
    for (int hf = 0; hf < 2; ++hf) {
      const float4 ka = kl[hf * 32], kb = kl[64 + hf * 32], kd = kl[128 + hf * 32];
      rk[4 * hf + 0] = DxCoef{ka.x, kb.x, kd.x, 0.f};
      rk[4 * hf + 1] = DxCoef{ka.y, kb.y, kd.y, 0.f};
      rk[4 * hf + 2] = DxCoef{ka.z, kb.z, kd.z, 0.f};
      rk[4 * hf + 3] = DxCoef{ka.w, kb.w, kd.w, 0.f};
    }
    // dx3 of this lane's vectors -> LDS (rows past P: zeros, not the constant term d)
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      bf16 td[8], tx[8];
      __builtin_memcpy(td, &qd[i], 16);
      __builtin_memcpy(tx, &qx[i], 16);
      float d[8], xv[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        d[j] = static_cast<float>(td[j]);
        xv[j] = static_cast<float>(tx[j]);
      }
      dx_vec<bf16, 3, false>(d, xv, d, mb[i], rk);
      const bool ok = p0 + r0 + kRpi * i < p.P;
      bf16x8 o;
#pragma unroll
      for (int j = 0; j < 8; ++j) o[j] = ok ? static_cast<bf16>(xv[j]) : static_cast<bf16>(0.f);
      *reinterpret_cast<bf16x8*>(tile + (r0 + kRpi * i) * kLdT + vec * 8) = o;
      __builtin_amdgcn_sched_barrier(0);  // one row at a time: interleaved, the rows' fp32 temporaries spill
    }
#pragma unroll
    for (int i = 0; i < kAv; ++i)
      *reinterpret_cast<uint4*>(atile + (arow + 32 * i) * kLdS + avec * 8) =
          p0 + arow + 32 * i < p.P ? qa[i] : uint4{0u, 0u, 0u, 0u};
    __syncthreads();
    // the next tile's loads fly under this tile's MFMAs
    if (tl + gridDim.x < ntiles) issue(tl + gridDim.x);

    // d_a2^T [cin][pixel] = W^T [cin][cout] . dx3^T [cout][pixel]: this wave's 16 cin x the 32 pixels
    {
      f32x4 da[kTP / 16];
#pragma unroll
      for (int i = 0; i < kTP / 16; ++i) da[i] = f32x4{0.f, 0.f, 0.f, 0.f};
      const bf16* brow = tile + (lane & 15) * kLdT + 8 * (lane >> 4);
#pragma unroll
      for (int ks = 0; ks < kCo / 32; ++ks) {
#pragma unroll
        for (int i = 0; i < kTP / 16; ++i) {
          const bf16x8 fb = *reinterpret_cast<const bf16x8*>(brow + 16 * i * kLdT + 32 * ks);
          da[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(wf[ks], fb, da[i], 0, 0, 0);
        }
      }
      // da[i][r] = d_a2[pixel p0 + 16 i + (lane & 15)][cin 16 wave + 4 (lane >> 4) + r]
      // (uniform tile base + a 32-bit lane offset: no 64-bit per-lane address held across the loop)
      bf16* ob = p.d_a2 + p0 * kCi;
      const unsigned oo = static_cast<unsigned>(lane & 15) * kCi + 16 * wave + 4 * (lane >> 4);
#pragma unroll
      for (int i = 0; i < kTP / 16; ++i) {
        if (p0 + 16 * i + (lane & 15) < p.P) {
          bf16x4 o;
#pragma unroll
          for (int r = 0; r < 4; ++r) o[r] = static_cast<bf16>(da[i][r]);
          *reinterpret_cast<bf16x4*>(ob + oo + 16 * i * kCi) = o;
        }
      }
    }
    // dW [cout][cin] += dx3^T [cout][pixel] . a2 [pixel][cin]
#pragma unroll
    for (int kh = 0; kh < kTP / 32; ++kh) {
      bf16x8 fb[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) fb[j] = frag_tr(atile, kLdS, 32 * kh, 16 * j);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bf16x8 fa = frag_tr(tile, kLdT, 32 * kh, wave * 64 + 16 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb[j], acc[i][j], 0, 0, 0);
      }
    }
    __syncthreads();  // every wave is done with the tiles before the next iteration overwrites them
  }

  // acc[i][j][r] = dW[cout wave * 64 + 16 i + 4 (lane >> 4) + r][cin 16 j + (lane & 15)]
  float* slab = p.ws + static_cast<int64_t>(blockIdx.x) * (kCo * kCi);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        slab[static_cast<unsigned>((wave * 64 + 16 * i + 4 * (lane >> 4) + r) * kCi + 16 * j + (lane & 15))] = acc[i][j][r];
}

}  // namespace

void conv3bn3_bwd(const GemmProblem& g, hipStream_t stream) {
  // (N, K) = (Cin, Cout): (64, 256) here, (128, 512) in conv3bn3_s2_bwd.hip
  const bool s2 = g.N == 128 && g.K == 512;
  if (!((g.N == kCi && g.K == kCo) || s2) || g.M < 1 || g.lda != g.K || g.ldb != g.N || g.ldc != g.N || g.ldr != g.N ||
      !g.a_kmajor || g.b_kmajor || g.bnb_rm != 3)
    throw std::runtime_error("gemm_bf16 mode 4: needs (N, K) = (64, 256) or (128, 512), dense operands (lda = K, ldb = "
                             "ldc = ldr = N), K-major A, N-major B and the 1-bit ReLU mask (bnb_rm = 3); got M=" +
                             std::to_string(g.M) + ", N=" + std::to_string(g.N) + ", K=" + std::to_string(g.K));
  if (g.a == nullptr || g.b == nullptr || g.c == nullptr || g.res == nullptr || g.bnb_x == nullptr ||
      g.bnb_mask == nullptr || g.bnb_mean == nullptr || g.bnb_inv == nullptr || g.a_scale == nullptr ||
      g.a_shift == nullptr || g.stats == nullptr)
    throw std::runtime_error("gemm_bf16 mode 4: dy, W, d_a2, a2 (res), x3 (bnb_x), the mask, mean / invstd, the two "
                             "sums (a_scale / a_shift) and the slab workspace (stats) are all required");
  uintptr_t bits = 0;
  for (const void* q : {g.a, g.b, static_cast<const void*>(g.c), g.res, g.bnb_x, static_cast<const void*>(g.bnb_w),
                        static_cast<const void*>(g.bnb_mean), static_cast<const void*>(g.bnb_inv),
                        static_cast<const void*>(g.a_scale), static_cast<const void*>(g.a_shift),
                        static_cast<const void*>(g.stats)})
    bits |= reinterpret_cast<uintptr_t>(q);
  if ((bits & 15u) != 0) throw std::runtime_error("gemm_bf16 mode 4: operands must be 16-byte aligned");
  // (more workgroups than tiles is allowed: the extra ones store zero slabs)
  if (g.splits < 1 || g.splits > 65535)
    throw std::runtime_error("gemm_bf16 mode 4: splits (the slab count = workgroups) must be in [1, 65535]");
  C3Args p{static_cast<const bf16*>(g.a), static_cast<const bf16*>(g.bnb_x), g.bnb_mask, g.bnb_w, g.bnb_mean,
           g.bnb_inv, g.a_scale, g.a_shift, static_cast<const bf16*>(g.res), static_cast<const bf16*>(g.b),
           static_cast<bf16*>(g.c), g.stats, g.M};
  if (s2) return conv3bn3_s2_launch(p, g.splits, stream);
  allow_dynamic_lds(reinterpret_cast<const void*>(&conv3bn3_bwd_kernel), kSmem);
  conv3bn3_bwd_kernel<<<static_cast<unsigned>(g.splits), kThreads, kSmem, stream>>>(p);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace fluxmpi
