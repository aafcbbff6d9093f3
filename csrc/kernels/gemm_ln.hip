// Linear + residual add + LayerNorm forward in one launch — gfx950. A workgroup owns whole output rows, so
// the projection output never exists in memory and the row statistics never leave the workgroup:
//
//   acc  = a W^T                          a [M][K], W [N][K] bf16, fp32 on v_mfma_f32_16x16x32_bf16
//   h    = bf16(acc + bias + x)           one rounding, stored
//   f    = float(h)                       the STORED h is what gets normalised (layernorm.hip's arithmetic from
//   mean = sum(f) / N                     here on: two passes over registers, fmaf for the squares and for y)
//   rstd = rsqrt(sum((f - mean)^2) / N + eps)
//   y    = bf16(fmaf((f - mean) * rstd, w, b))      stored; mean, rstd stored fp32 per row
//
// N is 384 or 768 (one instantiation each), K a multiple of 64, any M (gemm_ln_host.h).
//
// Work split. 512 threads, one workgroup per CU, a tile is BM = 64 rows x N columns. The 8 waves are WM (M) x
// WN (N) = 1 x 8 at N = 768 and 2 x 4 at N = 384, so that a wave always owns 96 columns = 6 MFMA column tiles
// (an even count: the epilogue exchanges column tiles in pairs) by RT = 4 / WM row tiles: 96 accumulator
// registers at N = 768, 48 at N = 384. Per 32-deep k-tile a wave reads RT A and 6 B fragments for 6 RT MFMAs.
// (The issue's sketch was 1 x 8 for both N; at N = 384 that leaves 3 column tiles per wave, which cannot pair.)
//
// K loop. Operands go global -> LDS by LDS-DMA (buffer loads, 16 B per lane, a wave instruction = 1 KiB = 16
// rows of the 64-byte stage rows). A stage is [64 A rows | N B rows] x 32 k, 52 KiB at N = 768; three stages
// (156 KiB) form a ring and two k-tiles are always in flight under the one being multiplied. The 16-byte chunk c
// of row r sits in slot c ^ ((r >> 2) & 3): the 16 rows of a fragment read (one chunk each, ds_read_b128) then
// fall into 16 distinct 16-byte bank slots of the 256-byte bank span — gemm_nt.hip's chunk ^ ((row >> 1) & 7)
// for 128-byte rows, restated for 64-byte ones; the swizzle is applied to the lane's SOURCE chunk. Per k-tile:
// one counted s_waitcnt (the k-tile's own DMA groups: B's N / 128 per wave, and A's one on waves 0 - 3, so
// the count differs between the two wave classes), one barrier, the issue of k-tile t + 2 into the stage that
// k-tile t - 1 just left, the MFMAs. Issues past the last tile of a workgroup use an offset outside the buffer
// resource (no memory access, zeros), so the counts never change. A rows past M read as zeros the same way.
//
// Persistent grid (gemm_ln_host.h): the 16-row units of M are dealt to the workgroups as contiguous ranges that
// differ by at most one unit; a workgroup walks its range in 64-row tiles and, in a partial last tile, skips the
// MFMA row tiles it does not own (a wave-uniform branch). The ring runs on across tiles: the next tile's first
// two k-tiles are issued during this tile's last two and land under its epilogue.
//
// Epilogue, from the accumulators. A lane holds row (lane & 15) of each row tile and columns 4 (lane >> 4) + r
// of each column tile. The fp32 accumulators of a column-tile pair are exchanged between lane rows g and g ^ 1
// (v_permlane16_swap, gemm_nt.hip's exchange done before the rounding instead of after), after which a lane
// holds 8 consecutive columns, 32 q + 16 (g & 1) + 8 (g >> 1) of the wave's 96: x is read and h, y are stored
// 16 bytes per lane, bias and the LayerNorm affine are read 8 values at a time (bf16 or fp32 by a wave-uniform
// flag). Row sums: 24 values in the lane in column order, then the 4 lanes of a row (lane ^ 32, lane ^ 16: the
// row's lanes are 16 apart, so these are permlane swaps, not DPP), then the WN waves in wave order through a
// [WN][64] LDS array that every wave sums for itself; once for the mean, once for the centred squares. No
// atomics, one fixed order: the result is bit-identical from run to run and whatever the grid. Longest chain:
// 24 + 2 + 8 additions. Rows outside the workgroup's range are never stored (a lane predicate on every store);
// a row's statistics use that row's values only, so the garbage of unowned rows reaches no stored row.
#include <cstdint>
#include <stdexcept>
#include <string>

#include "../api.h"
#include "common.h"
#include "gemm_ln_host.h"

namespace fluxmpi {
namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((address_space(3))) char lds_char;

constexpr int kRowB = kLnBK * 2;           // bytes of a stage row
constexpr int kAImg = kLnBM * kRowB;       // 4 KiB: the A rows of a stage
constexpr int kRed = 2 * 8 * kLnBM * 4;    // two [WN <= 8][64] fp32 arrays
constexpr uint32_t kOutside = 0x80000000u;  // a buffer offset past every resource's range

struct GemmLnArgs {
  const bf16* a;      // [M][K]
  const bf16* w;      // [N][K]
  const void* bias;   // [N] bf16 / fp32
  const bf16* x;      // [M][N]
  bf16* h;            // [M][N]
  bf16* y;            // [M][N]
  const void* ln_w;   // [N] bf16 / fp32
  const void* ln_b;
  float* mean;        // [M]
  float* rstd;
  int M, K;
  float eps;
  int bias_f32, ln_f32;
};

// __restrict__: the fragment reads get an alias scope of their own, without which the waitcnt pass takes them to
// read what the LDS-DMA just issued writes and drains vmcnt(0) in front of them (mx_wgrad.hip)
__device__ __forceinline__ bf16x8 frag(const char* __restrict__ p) { return *reinterpret_cast<const bf16x8*>(p); }

// gemm_nt.hip's guard: wait states before a later instruction may overwrite a 16-byte store's data registers
__device__ __forceinline__ void store_guard() {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("s_nop 3");
  __builtin_amdgcn_sched_barrier(0);
}

// 8 consecutive parameters from column c (a multiple of 8) as fp32
__device__ __forceinline__ void ld8p(const void* __restrict__ p, int f32, int c, float (&v)[8]) {
  if (f32) {
    const float4 a0 = *reinterpret_cast<const float4*>(static_cast<const float*>(p) + c);
    const float4 a1 = *reinterpret_cast<const float4*>(static_cast<const float*>(p) + c + 4);
    v[0] = a0.x, v[1] = a0.y, v[2] = a0.z, v[3] = a0.w, v[4] = a1.x, v[5] = a1.y, v[6] = a1.z, v[7] = a1.w;
  } else {
    bf16 t[8];
    load8(static_cast<const bf16*>(p) + c, t);
#pragma unroll
    for (int e = 0; e < 8; ++e) v[e] = static_cast<float>(t[e]);
  }
}

template <int N>
__global__ __launch_bounds__(kLnThreads, 2) void gemm_ln_kernel(GemmLnArgs p) {
  constexpr int WM = N == 768 ? 1 : 2, WN = 8 / WM;
  constexpr int RT = 4 / WM;          // row tiles of a wave
  constexpr int CT = 6;               // column tiles of a wave: N / WN / 16
  constexpr int BJ = N / 128;         // B DMA instructions per wave and k-tile
  constexpr int kStage = kAImg + N * kRowB;
  static_assert(N / WN == 16 * CT && kLnStages * kStage + kRed <= 160 * 1024, "geometry");
  __shared__ __attribute__((aligned(1024))) char smem[kLnStages * kStage + kRed];
  float* const red1 = reinterpret_cast<float*>(smem + kLnStages * kStage);
  float* const red2 = red1 + 8 * kLnBM;

  const int G = gridDim.x;
  const int64_t units = gemm_ln_units(p.M);
  const int u0 = static_cast<int>(gemm_ln_range_start(units, G, blockIdx.x));
  const int u1 = static_cast<int>(gemm_ln_range_start(units, G, blockIdx.x + 1));
  const int ntiles = __builtin_amdgcn_readfirstlane((u1 - u0 + 3) / 4);
  if (ntiles <= 0) return;  // workgroup-uniform, before any DMA or barrier
  const int row_end = u1 * kLnUnit < p.M ? u1 * kLnUnit : p.M;  // the workgroup stores rows below this
  const int nk = p.K / kLnBK;                                   // even, >= 2
  const int K2 = p.K * 2;                                       // bytes of an operand row

  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
  const int wm = wave / WN, wn = wave % WN;
  const int fr = lane & 15, g = lane >> 4;

  // ---- LDS-DMA lanes: lane -> row lane >> 2 of the instruction's 16, slot lane & 3, which holds the chunk
  // slot ^ ((row >> 2) & 3); the 16 rows start at a multiple of 16, so (row >> 2) & 3 = lane >> 4
  const uint32_t lane_src = static_cast<uint32_t>((lane >> 2) * K2 + (((lane & 3) ^ (lane >> 4)) << 4));
  const uint32_t laneA = lane_src + static_cast<uint32_t>(16 * (wave & 3) * K2);  // waves 0 - 3: A rows 16 wave ..
  const uint32_t laneB = lane_src + static_cast<uint32_t>(16 * BJ * wave * K2);   // B rows 16 BJ wave + 16 j ..
  const __amdgpu_buffer_rsrc_t arsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<bf16*>(p.a), 0, static_cast<uint32_t>(p.M) * static_cast<uint32_t>(K2), 0x00020000);
  const __amdgpu_buffer_rsrc_t brsrc =
      __builtin_amdgcn_make_buffer_rsrc(const_cast<bf16*>(p.w), 0, static_cast<uint32_t>(N) * static_cast<uint32_t>(K2), 0x00020000);
  // k-tile kt of the tile whose first row is m0 into `stage`; !live: the same instructions, no memory access
  auto issue = [&](int stage, int m0, int kt, bool live) {
    char* s = smem + stage * kStage;
    if (wave < 4) {
      const uint32_t vo = live ? laneA + static_cast<uint32_t>(m0 * K2 + kt * kRowB) : kOutside;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(arsrc, (lds_char*)(s + wave * 1024), 16, vo, 0, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < BJ; ++j) {
      const uint32_t vo = live ? laneB + static_cast<uint32_t>(16 * j * K2 + kt * kRowB) : kOutside;
      __builtin_amdgcn_raw_ptr_buffer_load_lds(brsrc, (lds_char*)(s + kAImg + (wave * BJ + j) * 1024), 16, vo, 0, 0, 0);
    }
  };

  // ---- fragment reads: row lane & 15 of a 16-row tile, chunk lane >> 4 at slot chunk ^ ((row >> 2) & 3)
  const int slot = (g ^ ((fr >> 2) & 3)) << 4;
  const int offA = (wm * RT * 16 + fr) * kRowB + slot;               // + 1 KiB per row tile
  const int offB = kAImg + (wn * CT * 16 + fr) * kRowB + slot;       // + 1 KiB per column tile

  // ---- epilogue lanes: 8 consecutive columns per column-tile pair q, from colx + 32 q
  const int colx = wn * CT * 16 + 16 * (g & 1) + 8 * (g >> 1);
  const __amdgpu_buffer_rsrc_t xrsrc = __builtin_amdgcn_make_buffer_rsrc(
      const_cast<bf16*>(p.x), 0, static_cast<uint32_t>(p.M) * static_cast<uint32_t>(2 * N), 0x00020000);
  const float inv_n = 1.f / static_cast<float>(N);

  f32x4 acc[RT][CT];
  int st = 0;  // the ring stage of the k-tile to multiply next
  auto m0_of = [&](int tt) { return (u0 + 4 * tt) * kLnUnit; };
  issue(0, m0_of(0), 0, true);
  issue(1, m0_of(0), 1, true);

  for (int tt = 0; tt < ntiles; ++tt) {
    const int m0 = __builtin_amdgcn_readfirstlane(m0_of(tt));
    const int left = u1 - u0 - 4 * tt;
    const int nu = __builtin_amdgcn_readfirstlane(left < 4 ? left : 4);  // units this tile owns
    const bool has_next = tt + 1 < ntiles;
    const int m0n = __builtin_amdgcn_readfirstlane(m0_of(has_next ? tt + 1 : tt));
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
      for (int j = 0; j < CT; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    for (int t = 0; t < nk; ++t) {
      // k-tile t has landed once only k-tile t + 1's groups (and anything younger) are outstanding
      if (wave < 4) asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(BJ + 1) : "memory");
      else asm volatile("s_waitcnt vmcnt(%0) lgkmcnt(0)" ::"n"(BJ) : "memory");
      __builtin_amdgcn_sched_barrier(0);
      __builtin_amdgcn_s_barrier();
      __builtin_amdgcn_sched_barrier(0);
      // every wave has left k-tile t - 1: its stage takes k-tile t + 2 (the next tile's first ones at the end)
      const int s2 = st >= 1 ? st - 1 : kLnStages - 1;
      if (t + 2 < nk) issue(s2, m0, t + 2, true);
      else issue(s2, m0n, t + 2 - nk, has_next);
      const char* buf = smem + st * kStage;
      bf16x8 fb[CT], fa[RT];  // every fragment is read (an unowned row tile's lies inside the stage all the same)
#pragma unroll
      for (int j = 0; j < CT; ++j) fb[j] = frag(buf + offB + j * 1024);
#pragma unroll
      for (int i = 0; i < RT; ++i) fa[i] = frag(buf + offA + i * 1024);
#pragma unroll
      for (int i = 0; i < RT; ++i) {
        if (wm * RT + i < nu) {  // wave-uniform: a row tile past the workgroup's range is not computed
#pragma unroll
          for (int j = 0; j < CT; ++j)
            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fb[j], fa[i], acc[i][j], 0, 0, 0);
        }
      }
      st = st + 1 == kLnStages ? 0 : st + 1;
    }

    // ---- epilogue. Pass 1: h = bf16(acc + bias + x), stored; f = float(h) replaces acc; the row sums.
    // After the exchange acc[i][2q][r] / acc[i][2q+1][r] are columns colx + 32 q + r / + 4 + r.
    float s[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) s[i] = 0.f;
#pragma unroll
    for (int q = 0; q < CT / 2; ++q) {
      float bias[8];
      ld8p(p.bias, p.bias_f32, colx + 32 * q, bias);
#pragma unroll
      for (int i = 0; i < RT; ++i) {
        if (wm * RT + i < nu) {
          const int row = m0 + (wm * RT + i) * 16 + fr;
          const uint32_t off = static_cast<uint32_t>(row * N + colx + 32 * q) * 2u;  // past M: zeros
          const auto xv = __builtin_amdgcn_raw_buffer_load_b128(xrsrc, off, 0, 0);
          bf16 xe[8], he[8];
          __builtin_memcpy(xe, &xv, 16);
          float f[8];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            // vector elements are copied out before a bit cast, both ways: __builtin_bit_cast on an ext-vector
            // element reads element 0 (common.h; here it made columns 4c .. 4c + 3 all equal column 4c)
            const float e0 = acc[i][2 * q][r], e1 = acc[i][2 * q + 1][r];
            const auto sw = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, e0),
                                                             __builtin_bit_cast(unsigned, e1), false, false);
            const unsigned r0 = sw[0], r1 = sw[1];
            f[r] = __builtin_bit_cast(float, r0);
            f[4 + r] = __builtin_bit_cast(float, r1);
          }
#pragma unroll
          for (int e = 0; e < 8; ++e) {
            he[e] = static_cast<bf16>(f[e] + bias[e] + static_cast<float>(xe[e]));
            f[e] = static_cast<float>(he[e]);
            s[i] += f[e];
          }
#pragma unroll
          for (int r = 0; r < 4; ++r) acc[i][2 * q][r] = f[r], acc[i][2 * q + 1][r] = f[4 + r];
          if (row < row_end) {
            uint4 hv;
            __builtin_memcpy(&hv, he, 16);
            *reinterpret_cast<uint4*>(p.h + static_cast<int64_t>(row) * N + colx + 32 * q) = hv;
            store_guard();
          }
        }
      }
    }
    // the row's 4 lanes, then the WN waves in wave order (every wave forms the same sum for itself)
    float mean[RT], rstd[RT];
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      s[i] = xor_sum<16>(xor_sum<32>(s[i]));
      if (g == 0) red1[wn * kLnBM + (wm * RT + i) * 16 + fr] = s[i];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      float tot = red1[(wm * RT + i) * 16 + fr];
#pragma unroll
      for (int w = 1; w < WN; ++w) tot += red1[w * kLnBM + (wm * RT + i) * 16 + fr];
      mean[i] = tot * inv_n;
      float qs = 0.f;
#pragma unroll
      for (int j = 0; j < CT; ++j)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const float d = acc[i][j][r] - mean[i];
          qs = fmaf(d, d, qs);
        }
      qs = xor_sum<16>(xor_sum<32>(qs));
      if (g == 0) red2[wn * kLnBM + (wm * RT + i) * 16 + fr] = qs;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < RT; ++i) {
      float tot = red2[(wm * RT + i) * 16 + fr];
#pragma unroll
      for (int w = 1; w < WN; ++w) tot += red2[w * kLnBM + (wm * RT + i) * 16 + fr];
      rstd[i] = rsqrtf(tot * inv_n + p.eps);
      const int row = m0 + (wm * RT + i) * 16 + fr;
      if (wn == 0 && g == 0 && wm * RT + i < nu && row < row_end) {
        p.mean[row] = mean[i];
        p.rstd[row] = rstd[i];
      }
    }
    // pass 3: y
#pragma unroll
    for (int q = 0; q < CT / 2; ++q) {
      float lw[8], lb[8];
      ld8p(p.ln_w, p.ln_f32, colx + 32 * q, lw);
      ld8p(p.ln_b, p.ln_f32, colx + 32 * q, lb);
#pragma unroll
      for (int i = 0; i < RT; ++i) {
        const int row = m0 + (wm * RT + i) * 16 + fr;
        if (wm * RT + i < nu && row < row_end) {
          bf16 ye[8];
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            ye[r] = static_cast<bf16>(fmaf((acc[i][2 * q][r] - mean[i]) * rstd[i], lw[r], lb[r]));
            ye[4 + r] = static_cast<bf16>(fmaf((acc[i][2 * q + 1][r] - mean[i]) * rstd[i], lw[4 + r], lb[4 + r]));
          }
          uint4 yv;
          __builtin_memcpy(&yv, ye, 16);
          *reinterpret_cast<uint4*>(p.y + static_cast<int64_t>(row) * N + colx + 32 * q) = yv;
          store_guard();
        }
      }
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the last two issues (no memory access, but counted)
}

int resident(const void* kernel) {
  return resident_blocks(kernel, kLnThreads, 0);
}

}  // namespace

bool linear_add_ln_supported(int64_t M, int64_t N, int64_t K) { return gemm_ln_shape_ok(M, N, K); }

void linear_add_ln_fwd(const void* a, const void* w, const void* bias, const void* x, void* h, void* y, const void* ln_w,
                       const void* ln_b, float* mean, float* rstd, int64_t M, int64_t N, int64_t K, float eps,
                       int bias_dtype, int ln_wdtype, hipStream_t stream, int max_blocks) {
  if (!gemm_ln_shape_ok(M, N, K))
    throw std::runtime_error("linear_add_ln_fwd: unsupported shape M " + std::to_string(M) + " N " + std::to_string(N) +
                             " K " + std::to_string(K) + " (N is 384 or 768, K a multiple of 64)");
  if (!gemm_ln_aligned16({a, w, bias, x, h, y, ln_w, ln_b}) || mean == nullptr || rstd == nullptr)
    throw std::runtime_error("linear_add_ln_fwd: every tensor must be present and 16-byte aligned");
  for (int dt : {bias_dtype, ln_wdtype})
    if (dt != kBF16 && dt != kF32) throw std::runtime_error("linear_add_ln_fwd: bias and the LayerNorm affine are bf16 or fp32");
  if (max_blocks < 0) throw std::runtime_error("linear_add_ln_fwd: max_blocks must be >= 0 (0: the resident workgroups)");
  GemmLnArgs p{static_cast<const bf16*>(a), static_cast<const bf16*>(w), bias, static_cast<const bf16*>(x),
               static_cast<bf16*>(h), static_cast<bf16*>(y), ln_w, ln_b, mean, rstd, static_cast<int>(M),
               static_cast<int>(K), eps, bias_dtype == kF32, ln_wdtype == kF32};
  auto launch = [&](auto kernel) {
    const int grid = gemm_ln_grid(M, resident(reinterpret_cast<const void*>(kernel)), max_blocks);
    kernel<<<grid, kLnThreads, 0, stream>>>(p);
  };
  if (N == 768) launch(&gemm_ln_kernel<768>);
  else launch(&gemm_ln_kernel<384>);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace fluxmpi
