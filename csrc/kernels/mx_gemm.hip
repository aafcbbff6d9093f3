// MX (block-scaled) fp8 NT GEMM on the scaled 128-deep MFMA — gfx950.
//
//   C[m][n] = bf16( sum over 32-deep K blocks kb of 2^(ea[m][kb] - 127) 2^(eb[n][kb] - 127) (A_blk . B_blk)  (+ bias[n]) )
//
// A [M][K] (e4m3 or e5m2) and B [N][K] (e4m3) are fp8, k-contiguous, each with a scale image of E8M0 bytes,
// one per row and 32 K bytes, rows padded with 127 to a whole dword per 128-byte K tile (mx_host.h).
// v_mfma_scale_f32_16x16x128_f8f6f4 applies both block scales inside the instruction and accumulates in
// fp32; the epilogue only adds the bias and rounds once.
//
// The operand path is gemm_fp8.hip's and is described there: a workgroup of 4 waves (2 x 2) owns 128 x 128
// of C, a wave 4 x 4 MFMA tiles; two register-staged LDS stages of [128 A rows + 128 B rows][128 B] with the
// chunk ^ (row & 7) swizzle; lane l holds row / column l & 15; B is the first operand and the LOADER orders
// B's rows so that a lane ends with 8 consecutive columns of C. One thing differs, and the scales are what
// makes it visible (found on MI355X by moving one scale byte at a time, see below): the instruction's K
// index of lane group g = l >> 4 is NOT 32 g .. 32 g + 31. VGPRs 0 - 3 of an operand are K = 16 g .. 16 g + 15
// and VGPRs 4 - 7 are K = 64 + 16 g .. 64 + 16 g + 15 (two 64-deep halves). The unscaled product does not care
// (gemm_fp8.hip pairs the same bytes of A and B whatever their K index), but scale block kb covers the
// instruction's K = 32 kb .. 32 kb + 31, i.e. the first halves of lane groups 2 kb and 2 kb + 1 (kb < 2) or
// the second halves of lane groups 2 (kb - 2) and 2 (kb - 2) + 1. So a lane reads the 16-byte chunks g and
// 4 + g of the 128-byte tile row (not 2 g and 2 g + 1); then instruction K = memory K and block kb is the
// image's block kb. What is new is the scales' path:
//   * Global -> registers: the K tile of step s needs one scale dword (4 blocks) of each of the 256 tile
//     rows; lane t of the workgroup fetches the dword of LDS row t & 127 of A (t < 128) or of B (t >= 128,
//     the row the loader's order puts there) in issue(), next to its operand chunks, so no global load sits
//     between MFMAs. Rows past M / N are not read and count as 0x7f7f7f7f; the bytes of K blocks past K are
//     forced to 127 whatever the image's padding holds (operand zeros times a stale 255 = NaN would be NaN).
//   * Registers -> LDS: each stage has a 1 KiB scale area behind its operand rows, laid out for the CONSUMER:
//     dword [operand][wave row / column w][K group g][li], its byte i = the scale of (MFMA tile i of wave w,
//     row li, K group g). commit() scatters the lane's four bytes (g = 0 .. 3) to byte (row >> 4) & 3 of the
//     dwords [row >> 6][g][row & 15]: four ds_write_b8.
//   * LDS -> MFMA: a lane reads ONE dword for its four A fragments and one for its four B fragments per K
//     step (the 64 lanes of a wave read 64 consecutive dwords) and the MFMA picks the byte with op_sel =
//     tile index: (fb[j], fa[i], acc, FB, FA, j, sb, i, sa). No byte extraction in VALU.
//   * Scale operand layout, as found: lane l supplies, in the byte op_sel picks, the scale of row l & 15 and
//     of K block l >> 4 of the INSTRUCTION's K order (above), which is not the 32 bytes the lane holds itself:
//     with all scales 127 but one at 128 and K group g of both operands at 2^g, the byte of (row, g) moved
//     exactly that row / column of C, by 16 (1 + 4) for g = 0 and 2 and 16 (16 + 64) for g = 1 and 3 under the
//     2 g, 2 g + 1 chunk order; with the g, 4 + g order it is the block's own 32 products.
// LDS is 2 x (32 KiB + 1 KiB) = 66 KiB, above the 64 KiB static limit, so it is dynamic; two workgroups per
// CU still fit in 160 KiB.
#include <stdexcept>
#include <string>
#include <utility>

#include "../api.h"
#include "c3_frag.h"
#include "common.h"
#include "mx_host.h"

namespace fluxmpi {
namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int kOperands = 2 * kFp8Tile * kFp8TileK;  // bytes of a stage's operand rows: A, then B
constexpr int kScaleArea = kFp8Tile * 4;             // bytes of one operand's scale area: a dword per row
constexpr int kStage = kOperands + 2 * kScaleArea;
constexpr int kSmem = 2 * kStage;
constexpr unsigned kOnes = 0x7f7f7f7fu;              // four E8M0 bytes of 2^0

struct MxGemmArgs {
  const uint8_t* a;   // [M][lda]
  const uint8_t* b;   // [N][ldb]
  bf16* c;            // [M][ldc]
  const void* bias;   // [N] or null
  const uint8_t* sa;  // [M][ldsa]
  const uint8_t* sb;  // [N][ldsb]
  int64_t lda, ldb, ldc, ldsa, ldsb;
  int M, N, K, n_tiles, k_tiles, bias_f32;
};

// byte offset of chunk `c` of row `r` inside an operand's [128][128 B] LDS tile
__device__ __forceinline__ int lds_ofs(int r, int c) { return r * kFp8TileK + ((c ^ (r & 7)) << 4); }

// lane group g's operand registers: K bytes 16 g .. + 15 (VGPRs 0 - 3) and 64 + 16 g .. + 15 (VGPRs 4 - 7)
__device__ __forceinline__ i32x8 read_frag(const uint8_t* tile, int row, int g) {
  const uint4 lo = *reinterpret_cast<const uint4*>(tile + lds_ofs(row, g));
  const uint4 hi = *reinterpret_cast<const uint4*>(tile + lds_ofs(row, g + 4));
  return i32x8{static_cast<int>(lo.x), static_cast<int>(lo.y), static_cast<int>(lo.z), static_cast<int>(lo.w),
               static_cast<int>(hi.x), static_cast<int>(hi.y), static_cast<int>(hi.z), static_cast<int>(hi.w)};
}

// the row of tile `rho` order -> the B row of the tile that the loader puts in LDS row rho (gemm_fp8.hip)
__device__ __forceinline__ int b_row(int rho) {
  return (rho & 64) + 32 * ((rho >> 5) & 1) + 8 * ((rho >> 2) & 3) + 4 * ((rho >> 4) & 1) + (rho & 3);
}

// the 4 MFMAs of A tile I: op_sel must be a constant, so the tile indices are template parameters
template <int FA, int FB, int I, int... J>
__device__ __forceinline__ void mfma_row(f32x4 (&acc)[4], const i32x8 (&fb)[4], const i32x8& fa, int sb, int sa,
                                         std::integer_sequence<int, J...>) {
  ((acc[J] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[J], fa, acc[J], FB, FA, J, sb, I, sa)), ...);
}

template <int FA, int FB>
__global__ __launch_bounds__(kFp8Threads) void mx_gemm_kernel(MxGemmArgs p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int mt = blockIdx.x / p.n_tiles, nt = blockIdx.x - mt * p.n_tiles;
  const int m0 = mt * kFp8Tile, n0 = nt * kFp8Tile;

  // operand loader: chunk t & 7 of the K tile, rows (t >> 3) + 32 u of the A tile and of the B tile
  const int kc = t & 7, lr = t >> 3;
  const uint8_t* arow[4];
  const uint8_t* brow[4];
  bool aok[4], bok[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int rho = lr + 32 * u;  // the LDS row; for B it holds the row the MFMA order wants there
    const int m = m0 + rho, n = n0 + b_row(rho);
    aok[u] = m < p.M, bok[u] = n < p.N;
    arow[u] = p.a + static_cast<int64_t>(aok[u] ? m : 0) * p.lda + kc * 16;
    brow[u] = p.b + static_cast<int64_t>(bok[u] ? n : 0) * p.ldb + kc * 16;
  }
  // scale loader: the dword of LDS row t & 127 of A (waves 0, 1) or of B (waves 2, 3)
  const int srho = t & 127, s_is_b = wave >> 1;
  const int sidx = s_is_b ? n0 + b_row(srho) : m0 + srho;
  const bool sok = sidx < (s_is_b ? p.N : p.M);
  const uint8_t* srow = (s_is_b ? p.sb : p.sa) + static_cast<int64_t>(sok ? sidx : 0) * (s_is_b ? p.ldsb : p.ldsa);
  // where its bytes go: dword [operand][srho >> 6][g][srho & 15], byte (srho >> 4) & 3
  const int sdst = kOperands + s_is_b * kScaleArea + (((srho >> 6) * 4) * 16 + (srho & 15)) * 4 + ((srho >> 4) & 3);
  const int kblocks = p.K / kMxBlock;

  uint4 ra[4], rb[4];
  unsigned rs;
  auto issue = [&](int step) {
    const int k = step * kFp8TileK + kc * 16;
    const bool kin = k < p.K;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      ra[u] = uint4{0u, 0u, 0u, 0u}, rb[u] = uint4{0u, 0u, 0u, 0u};
      if (kin && aok[u]) ra[u] = *reinterpret_cast<const uint4*>(arow[u] + step * kFp8TileK);
      if (kin && bok[u]) rb[u] = *reinterpret_cast<const uint4*>(brow[u] + step * kFp8TileK);
    }
    rs = kOnes;
    if (sok) rs = *reinterpret_cast<const uint32_t*>(srow + 4 * step);
    const int left = kblocks - 4 * step;  // >= 1: blocks of this K tile inside K
    if (left < 4) {
      const unsigned keep = (1u << (8 * left)) - 1u;
      rs = (rs & keep) | (kOnes & ~keep);
    }
  };
  auto commit = [&](int stage) {
    uint8_t* s = lds + stage * kStage;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      *reinterpret_cast<uint4*>(s + lds_ofs(lr + 32 * u, kc)) = ra[u];
      *reinterpret_cast<uint4*>(s + kFp8Tile * kFp8TileK + lds_ofs(lr + 32 * u, kc)) = rb[u];
    }
#pragma unroll
    for (int g = 0; g < 4; ++g) s[sdst + g * 64] = static_cast<uint8_t>(rs >> (8 * g));
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int li = lane & 15, g = lane >> 4;
  const int wm = wave >> 1, wn = wave & 1;
  const int brow0 = 64 * wn + li;
  const int arow0 = 64 * wm + li;
  const int sa_ofs = kOperands + (wm * 64 + lane) * 4, sb_ofs = kOperands + kScaleArea + (wn * 64 + lane) * 4;

  issue(0);
  commit(0);
  __syncthreads();
  for (int s = 0; s < p.k_tiles; ++s) {
    if (s + 1 < p.k_tiles) issue(s + 1);
    const uint8_t* cur = lds + (s & 1) * kStage;
    i32x8 fb[4], fa[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) fb[j] = read_frag(cur + kFp8Tile * kFp8TileK, brow0 + 16 * j, g);
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[i] = read_frag(cur, arow0 + 16 * i, g);
    const int sa = *reinterpret_cast<const int*>(cur + sa_ofs), sb = *reinterpret_cast<const int*>(cur + sb_ofs);
    constexpr std::make_integer_sequence<int, 4> tiles{};
    mfma_row<FA, FB, 0>(acc[0], fb, fa[0], sb, sa, tiles);
    mfma_row<FA, FB, 1>(acc[1], fb, fa[1], sb, sa, tiles);
    mfma_row<FA, FB, 2>(acc[2], fb, fa[2], sb, sa, tiles);
    mfma_row<FA, FB, 3>(acc[3], fb, fa[3], sb, sa, tiles);
    if (s + 1 < p.k_tiles) commit((s + 1) & 1);
    __syncthreads();
  }

  // acc[i][j][r] = C[m0 + 64 wm + 16 i + li][n0 + 64 wn + 32 (j >> 1) + 8 g + 4 (j & 1) + r]
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + 64 * wm + 16 * i + li;
    if (m >= p.M) continue;
    bf16* crow = p.c + static_cast<int64_t>(m) * p.ldc;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int n = n0 + 64 * wn + 32 * jj + 8 * g;
      if (n >= p.N) continue;
      float fbias[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      if (p.bias != nullptr) {
        if (p.bias_f32) {
          load8(static_cast<const float*>(p.bias) + n, fbias);
        } else {
          bf16 tb[8];
          load8(static_cast<const bf16*>(p.bias) + n, tb);
#pragma unroll
          for (int e = 0; e < 8; ++e) fbias[e] = static_cast<float>(tb[e]);
        }
      }
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = static_cast<bf16>(acc[i][2 * jj + (e >> 2)][e & 3] + fbias[e]);
      *reinterpret_cast<bf16x8*>(crow + n) = o;
    }
  }
}

template <int FA>
void launch(const MxGemmArgs& p, unsigned grid, hipStream_t stream) {
  allow_dynamic_lds(reinterpret_cast<const void*>(&mx_gemm_kernel<FA, kFp8E4M3>), kSmem);
  mx_gemm_kernel<FA, kFp8E4M3><<<grid, kFp8Threads, kSmem, stream>>>(p);
}

}  // namespace

void mx_gemm(const void* a, const void* b, void* c, const void* bias, int bias_dtype, const void* sa, const void* sb,
             int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldsa, int64_t ldsb, int fa,
             int fb, hipStream_t stream) {
  const Fp8GemmGeometry g = mx_gemm_check(a, b, c, bias, bias_dtype, sa, sb, M, N, K, lda, ldb, ldc, ldsa, ldsb, fa, fb);
  if (fb == kFp8E2M1)
    return mx4_gemm_launch(a, b, c, bias, bias_dtype == static_cast<int>(kF32), sa, sb, M, N, K, lda, ldb, ldc, ldsa, ldsb,
                           fa, g.n_tiles, g.k_tiles, g.grid, stream);
  if (mx_is_fp6(fb))
    return mx6_gemm_launch(a, b, c, bias, bias_dtype == static_cast<int>(kF32), sa, sb, M, N, K, lda, ldb, ldc, ldsa, ldsb,
                           fa, g.n_tiles, g.k_tiles, g.grid, stream);
  const MxGemmArgs p{static_cast<const uint8_t*>(a), static_cast<const uint8_t*>(b), static_cast<bf16*>(c), bias,
                     static_cast<const uint8_t*>(sa), static_cast<const uint8_t*>(sb), lda, ldb, ldc, ldsa, ldsb,
                     static_cast<int>(M), static_cast<int>(N), static_cast<int>(K), static_cast<int>(g.n_tiles),
                     g.k_tiles, bias_dtype == static_cast<int>(kF32)};
  const unsigned grid = static_cast<unsigned>(g.grid);
  if (fa == kFp8E4M3) launch<kFp8E4M3>(p, grid, stream);
  else launch<kFp8E5M2>(p, grid, stream);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace fluxmpi
