// One-pass backward around the dual BatchNorm of a ResNet stage-1 downsample block,
//   out = relu(bn3(conv3(a2)) + bn_ds(conv_ds(x))),   conv3 and conv_ds both 1x1, 64 -> 256, stride 1
// — gfx950. The two-branch sibling of conv3bn3_bwd.hip (read that file's header first).
//
// Unfused, bn_bwd_dx_dual_kernel reads (dy, c3, c_ds, mask) and writes both input gradients dx3 and
// dx_ds [P][256]; each is then read twice more, by its convolution's input-gradient GEMM and by its
// weight-gradient kernel. This kernel reads (dy, c3, c_ds, mask, a2, x) once, forms dy_eff, dx3 and
// dx_ds in registers with the dx pass's own arithmetic (bn_dx.h: bit-identical to what the dx passes
// store), rounds each to bf16 into its own LDS tile and feeds, per branch, both MFMA products:
//   d_a2    [P][64] = dx3   . W3        dW3   [256][64] = dx3^T   . a2
//   d_xside [P][64] = dx_ds . W_ds      dW_ds [256][64] = dx_ds^T . x
// Neither dx reaches memory.
//
// Structure: one persistent workgroup of 8 waves per CU (112 KiB of LDS), looping over 32-pixel tiles
// (tile = blockIdx.x, += gridDim.x). LDS holds, per branch, conv3bn3_bwd.hip's layout: the filter image,
// the dx tile, the 64-channel operand tile and the coefficient planes. All 8 waves share the element
// phase (lane = (row r of 16, channel vector v): 2 rows of dy, c3, c_ds and the mask byte; waves 0-3
// also stage a2, waves 4-7 x); then waves 0-3 run conv3bn3_bwd.hip's MFMA schedule on the bn3 branch
// and waves 4-7 the same on the downsample branch, each wave with its own W^T fragments and its own
// 64 x 64 piece of its branch's filter gradient in registers. The next tile's loads are issued before
// this tile's MFMAs. A workgroup stores its two filter-gradient partials as fp32 slabs
// ws3[blockIdx.x][256][64] and wsds[blockIdx.x][256][64] (plain stores; a workgroup without tiles
// stores zeros) and gemm_splitk_reduce sums each set: no float atomics, no grid barrier. Rows past P
// are zero in every tile, so the partial last tile adds nothing.
#include <stdexcept>
#include <string>

#include "../api.h"
#include "bn_dx.h"
#include "c3_frag.h"
#include "common.h"

namespace fluxmpi {
namespace {

constexpr int kThreads = 512;
constexpr int kHalf = kThreads / 2;  // the lanes of one branch (waves 0-3 / 4-7)
constexpr int kCo = 256, kCi = 64;   // both convolutions: Cin = 64 -> Cout = 256
constexpr int kTP = 32;              // pixels per tile
// LDS row strides in elements, as in conv3bn3_bwd.hip
constexpr int kLdT = kCo + 8;  // dx tile [kTP][kLdT]
constexpr int kLdS = kCi + 8;  // a2 / x tile [kTP][kLdS]
constexpr int kLdW = kCi;      // W image [kCo][kLdW]
constexpr int kWBytes = kCo * kLdW * 2, kTBytes = kTP * kLdT * 2, kABytes = kTP * kLdS * 2;
constexpr int kKBytes = 3 * kCo * static_cast<int>(sizeof(float));  // coefficient planes [3][2][32][4]
constexpr int kBranch = kWBytes + kTBytes + kABytes + kKBytes;      // 57 344 B per branch
constexpr int kSmem = 2 * kBranch;                                  // 114 688 B: one workgroup per CU
static_assert(kBranch % 16 == 0 && kHalf == kCo, "one lane per channel and branch computes the coefficients");
constexpr int kRpi = kThreads / (kCo / 8);       // rows of a tile the workgroup covers at once (16)
constexpr int kRows = kTP / kRpi;                // rows of a tile per lane (2)
static_assert(kTP * (kCi / 8) == kHalf, "one a2 / x vector of a tile per lane of its branch");

struct Branch {
  const bf16* c;             // the BatchNorm's input [P][256] (c3 / c_ds)
  const float* w;            // its weight (nullable: 1)
  const float* mean;
  const float* inv;
  const float* sum_dy;       // [256] = dbias
  const float* sum_dy_xhat;  // [256] = dweight
  const bf16* a;             // the convolution's input [P][64] (a2 / x)
  const bf16* wt;            // its filter [256][64]
  bf16* da;                  // its input gradient [P][64] (d_a2 / d_xside)
  float* ws;                 // [gridDim.x][256][64]
};

struct DsArgs {
  const bf16* dy;       // [P][256]
  const uint8_t* mask;  // [P * 256 / 8]
  Branch b[2];
  int64_t P;
};

__global__ __launch_bounds__(kThreads) void conv3ds_bwd_kernel(DsArgs p) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int br = wave >> 2, wv = wave & 3;  // this wave's branch and its place among the branch's four
  const int vec = t & 31, r0 = t >> 5;      // this lane's channel vector and its first row of a tile
  const int th = t & (kHalf - 1);           // its index within its branch's lanes
  const int arow = th >> 3, avec = th & 7;  // its a2 / x vector
  const int64_t ntiles = (p.P + kTP - 1) / kTP;
  // this wave's branch: operands of the MFMA phase, and of the a2 / x staging
  char* mine = smem + br * kBranch;
  bf16* wimg = reinterpret_cast<bf16*>(mine);
  bf16* tile = reinterpret_cast<bf16*>(mine + kWBytes);
  bf16* atile = reinterpret_cast<bf16*>(mine + kWBytes + kTBytes);
  const Branch& mb_ = p.b[br];

  // both filters -> their LDS images [cout][kLdW] (once)
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    bf16* img = reinterpret_cast<bf16*>(smem + b * kBranch);
#pragma unroll
    for (int i = 0; i < kCo * kCi / 8 / kThreads; ++i) {
      const int v = t + i * kThreads;
      const uint4 q = reinterpret_cast<const uint4*>(p.b[b].wt)[v];
      *reinterpret_cast<uint4*>(img + (v >> 3) * kLdW + (v & 7) * 8) = q;
    }
  }
  // the per-channel coefficients of both BatchNorms -> LDS: lane th of branch br computes channel th
  {
    const DxCoef k = dx_coef(th, mb_.w, nullptr, mb_.mean, mb_.inv, mb_.sum_dy_xhat, mb_.sum_dy,
                             1.f / static_cast<float>(p.P));
    float* ksm = reinterpret_cast<float*>(mine + kWBytes + kTBytes + kABytes);
    const int slot = ((th >> 2) & 1) * 128 + (th >> 3) * 4 + (th & 3);  // [half][vector][element]
    ksm[slot] = k.a;
    ksm[kCo + slot] = k.b;
    ksm[2 * kCo + slot] = k.d;
  }
  __syncthreads();

  // this wave's W^T fragments of its branch (cin 16 wv .. + 15 x all 256 cout) stay in registers
  bf16x8 wf[kCo / 32];
#pragma unroll
  for (int ks = 0; ks < kCo / 32; ++ks) wf[ks] = frag_tr(wimg, kLdW, 32 * ks, 16 * wv);

  uint4 qd[kRows], qx[2][kRows], qa;
  unsigned mb[kRows];
  // a tile's base addresses are wave-uniform and a lane's offsets within it 32-bit; rows past P
  // (the partial last tile) re-read the tile's last valid row and are zeroed on the way to LDS
  auto issue = [&](int64_t tl) {
    const int64_t p0 = tl * kTP;
    const int nr = p.P - p0 < kTP ? static_cast<int>(p.P - p0) : kTP;  // >= 1
    const bf16* dyb = p.dy + p0 * kCo;
    const bf16* c0b = p.b[0].c + p0 * kCo;
    const bf16* c1b = p.b[1].c + p0 * kCo;
    const uint8_t* mkb = p.mask + p0 * (kCo / 8);
#pragma unroll
    for (int i = 0; i < kRows; ++i) {
      const int r = r0 + kRpi * i < nr ? r0 + kRpi * i : nr - 1;
      const unsigned v = static_cast<unsigned>(r) * (kCo / 8) + vec;
      qd[i] = reinterpret_cast<const uint4*>(dyb)[v];
      qx[0][i] = reinterpret_cast<const uint4*>(c0b)[v];
      qx[1][i] = reinterpret_cast<const uint4*>(c1b)[v];
      mb[i] = mkb[v];
    }
    const int ra = arow < nr ? arow : nr - 1;
    qa = reinterpret_cast<const uint4*>(mb_.a + p0 * kCi)[static_cast<unsigned>(ra) * (kCi / 8) + avec];
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
    // dx3 and dx_ds of this lane's vectors -> the two LDS tiles (rows past P: zeros, not the constant
    // term d). One branch after the other: both branches' coefficients at once would hold 48 VGPRs.
    // dy_eff is formed from the same (dy, mask bits) in both: the same values.
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      // an offset the compiler cannot see through: the loop-invariant coefficient reads stay in
      // the loop instead of being hoisted into VGPRs held across it
      int opq = 0;
      asm volatile("" : "+v"(opq));
      const float4* kl =
          reinterpret_cast<const float4*>(smem + b * kBranch + kWBytes + kTBytes + kABytes + opq) + vec;
      bf16* tb = reinterpret_cast<bf16*>(smem + b * kBranch + kWBytes);
      DxCoef rk[8];
#pragma unroll
      for (int hf = 0; hf < 2; ++hf) {
        const float4 ka = kl[hf * 32], kb = kl[64 + hf * 32], kd = kl[128 + hf * 32];
        rk[4 * hf + 0] = DxCoef{ka.x, kb.x, kd.x, 0.f};
        rk[4 * hf + 1] = DxCoef{ka.y, kb.y, kd.y, 0.f};
        rk[4 * hf + 2] = DxCoef{ka.z, kb.z, kd.z, 0.f};
        rk[4 * hf + 3] = DxCoef{ka.w, kb.w, kd.w, 0.f};
      }
#pragma unroll
      for (int i = 0; i < kRows; ++i) {
        bf16 td[8], tx[8];
        __builtin_memcpy(td, &qd[i], 16);
        __builtin_memcpy(tx, &qx[b][i], 16);
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
        *reinterpret_cast<bf16x8*>(tb + (r0 + kRpi * i) * kLdT + vec * 8) = o;
        __builtin_amdgcn_sched_barrier(0);  // one row at a time: interleaved, the rows' fp32 temporaries spill
      }
    }
    *reinterpret_cast<uint4*>(atile + arow * kLdS + avec * 8) = p0 + arow < p.P ? qa : uint4{0u, 0u, 0u, 0u};
    __syncthreads();
    // the next tile's loads fly under this tile's MFMAs
    if (tl + gridDim.x < ntiles) issue(tl + gridDim.x);

    // d_a^T [cin][pixel] = W^T [cin][cout] . dx^T [cout][pixel]: this wave's 16 cin x the 32 pixels
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
      // da[i][r] = d_a[pixel p0 + 16 i + (lane & 15)][cin 16 wv + 4 (lane >> 4) + r]
      // (uniform tile base + a 32-bit lane offset: no 64-bit per-lane address held across the loop)
      bf16* ob = mb_.da + p0 * kCi;
      const unsigned oo = static_cast<unsigned>(lane & 15) * kCi + 16 * wv + 4 * (lane >> 4);
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
    // dW [cout][cin] += dx^T [cout][pixel] . a [pixel][cin]: this wave's cout 64 wv .. + 63 x all 64 cin
    {
      bf16x8 fb[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) fb[j] = frag_tr(atile, kLdS, 0, 16 * j);
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const bf16x8 fa = frag_tr(tile, kLdT, 0, wv * 64 + 16 * i);
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa, fb[j], acc[i][j], 0, 0, 0);
      }
    }
    __syncthreads();  // every wave is done with the tiles before the next iteration overwrites them
  }

  // acc[i][j][r] = dW[cout wv * 64 + 16 i + 4 (lane >> 4) + r][cin 16 j + (lane & 15)]
  float* slab = mb_.ws + static_cast<int64_t>(blockIdx.x) * (kCo * kCi);
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        slab[static_cast<unsigned>((wv * 64 + 16 * i + 4 * (lane >> 4) + r) * kCi + 16 * j + (lane & 15))] = acc[i][j][r];
}

}  // namespace

void conv3ds_bwd(const void* dy, const uint8_t* mask, const void* c3, const void* cds, const float* w,
                 const float* mean, const float* inv, const float* sum_dy, const float* sum_dy_xhat, const float* w2,
                 const float* mean2, const float* inv2, const float* sum_dy2, const float* sum_dy_xhat2, const void* a2,
                 const void* x, const void* wt3, const void* wtds, void* d_a2, void* d_xside, float* ws3, float* wsds,
                 int64_t P, int slabs, hipStream_t stream) {
  if (P < 1) throw std::runtime_error("conv3ds_bwd: P (pixels) must be >= 1, got " + std::to_string(P));
  uintptr_t bits = 0;
  for (const void* q : {dy, static_cast<const void*>(mask), c3, cds, static_cast<const void*>(mean),
                        static_cast<const void*>(inv), static_cast<const void*>(sum_dy),
                        static_cast<const void*>(sum_dy_xhat), static_cast<const void*>(mean2),
                        static_cast<const void*>(inv2), static_cast<const void*>(sum_dy2),
                        static_cast<const void*>(sum_dy_xhat2), a2, x, wt3, wtds, static_cast<const void*>(d_a2),
                        static_cast<const void*>(d_xside), static_cast<const void*>(ws3),
                        static_cast<const void*>(wsds)}) {
    if (q == nullptr)
      throw std::runtime_error("conv3ds_bwd: dy, the mask, c3, c_ds, both BatchNorms' mean / invstd / two sums, a2, x, "
                               "both filters, d_a2, d_xside and both slab workspaces are all required");
    bits |= reinterpret_cast<uintptr_t>(q);
  }
  bits |= reinterpret_cast<uintptr_t>(w) | reinterpret_cast<uintptr_t>(w2);  // the BatchNorm weights: nullable (1)
  if ((bits & 15u) != 0) throw std::runtime_error("conv3ds_bwd: operands must be 16-byte aligned");
  // (more workgroups than tiles is allowed: the extra ones store zero slabs)
  if (slabs < 1 || slabs > 65535)
    throw std::runtime_error("conv3ds_bwd: slabs (the slab count = workgroups) must be in [1, 65535]");
  allow_dynamic_lds(reinterpret_cast<const void*>(&conv3ds_bwd_kernel), kSmem);
  DsArgs p{static_cast<const bf16*>(dy), mask,
           {Branch{static_cast<const bf16*>(c3), w, mean, inv, sum_dy, sum_dy_xhat, static_cast<const bf16*>(a2),
                   static_cast<const bf16*>(wt3), static_cast<bf16*>(d_a2), ws3},
            Branch{static_cast<const bf16*>(cds), w2, mean2, inv2, sum_dy2, sum_dy_xhat2, static_cast<const bf16*>(x),
                   static_cast<const bf16*>(wtds), static_cast<bf16*>(d_xside), wsds}},
           P};
  conv3ds_bwd_kernel<<<static_cast<unsigned>(slabs), kThreads, kSmem, stream>>>(p);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace fluxmpi
