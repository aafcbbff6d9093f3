// fp8 NT GEMM on the 128-deep MFMA — gfx950.
//
//   C[m][n] = bf16( (1 / sa)(1 / sb) sum_k A[m][k] B[n][k]  (+ bias[n]) )
//
// A [M][K] and B [N][K] are fp8, k-contiguous; the formats are template parameters (e4m3 x e4m3 for a
// Linear's forward, e5m2 x e4m3 for its input gradient). Accumulation is fp32 in
// v_mfma_f32_16x16x128_f8f6f4; the two inverse scales (powers of two) are read from the operands' device
// scale blocks in the epilogue, so no scale ever visits the host.
//
//   * Split: a workgroup of 4 waves owns 128 x 128 of C and all of K; the waves are 2 x 2, each owns
//     64 x 64 = 4 x 4 MFMA tiles (64 accumulator VGPRs). The grid is not persistent; the column tiles of
//     one row tile are adjacent workgroups, so the A rows are fetched from HBM once and found in L2 by the
//     others (B, the weight, is L2-resident).
//   * Data movement: register staging, two LDS stages. A K tile is 128 bytes, so a tile row is exactly one
//     128-byte LDS row; per stage [128 A rows + 128 B rows][128 B] = 32 KiB, 64 KiB in all (two workgroups
//     per CU). Per step a lane loads 4 A chunks and 4 B chunks of 16 B for step s + 1 before the MFMAs of
//     step s and writes them to the other stage after them: one barrier per step. Rows past M / N and
//     chunks past K are not loaded and enter LDS as zeros (K % 16 == 0: a chunk is inside or outside as a
//     whole), so partial tiles in every dimension, and a partial last K tile, need no other care.
//   * Swizzle: rows 128 B apart would put the same chunk of every row on the same banks, so chunk c of
//     row r lives at chunk c ^ (r & 7) (as gemm_glds.hip): the 8 chunks that 8 consecutive rows read for one
//     fragment cover all banks once.
//   * Fragments: lane l holds row / column (l & 15) and the 32 K bytes 32 (l >> 4) .. + 31 of the tile: two
//     ds_read_b128 (chunks 2 (l >> 4) and 2 (l >> 4) + 1 before the swizzle), 8 VGPRs per fragment. Both
//     operands are read the same way, so the product depends only on A and B pairing the same K bytes.
//   * The MFMA's first operand is B (rows of the weight = columns of C), its second is A: a lane's 4
//     results are then 4 consecutive COLUMNS of one row of C. B's rows are assigned to first-operand rows
//     so that the tile pair (2 jj, 2 jj + 1) gives a lane 8 consecutive columns (patch_embed.hip's trick):
//     first-operand row li of tile j is B row 32 (j >> 1) + 8 (li >> 2) + 4 (j & 1) + (li & 3) of the wave's
//     64. The LOADER applies that order (LDS row 16 j + li holds that B row; a row is still 128 contiguous
//     bytes of global memory), so both operands' fragments read LDS rows 16 apart with r & 7 = li & 7. The
//     epilogue scales, adds the bias in fp32, rounds once and stores 16 B from registers, with no
//     staging tile. N % 8 == 0: a lane's 8 columns are inside or outside as a whole.
//
// No split-K, no fp32 output. Not tuned: the tile and the two stages were chosen by the arithmetic
// above; profiles/fp8_vit_b16.jsonl has what was measured.
#include <stdexcept>
#include <string>

#include "../api.h"
#include "c3_frag.h"
#include "common.h"
#include "fp8_host.h"

namespace fluxmpi {
namespace {

typedef int i32x8 __attribute__((ext_vector_type(8)));

constexpr int kStage = 2 * kFp8Tile * kFp8TileK;  // bytes of one LDS stage: the A rows, then the B rows

struct GemmArgs {
  const uint8_t* a;   // [M][lda]
  const uint8_t* b;   // [N][ldb]
  bf16* c;            // [M][ldc]
  const void* bias;   // [N] or null
  const float* sa;    // scale blocks: word 1 is the inverse scale
  const float* sb;
  int64_t lda, ldb, ldc;
  int M, N, K, n_tiles, k_tiles, bias_f32;
};

// byte offset of chunk `c` of row `r` inside an operand's [128][128 B] LDS tile
__device__ __forceinline__ int lds_ofs(int r, int c) { return r * kFp8TileK + ((c ^ (r & 7)) << 4); }

__device__ __forceinline__ i32x8 read_frag(const uint8_t* tile, int row, int g) {
  const uint4 lo = *reinterpret_cast<const uint4*>(tile + lds_ofs(row, 2 * g));
  const uint4 hi = *reinterpret_cast<const uint4*>(tile + lds_ofs(row, 2 * g + 1));
  return i32x8{static_cast<int>(lo.x), static_cast<int>(lo.y), static_cast<int>(lo.z), static_cast<int>(lo.w),
               static_cast<int>(hi.x), static_cast<int>(hi.y), static_cast<int>(hi.z), static_cast<int>(hi.w)};
}

template <int FA, int FB>
__global__ __launch_bounds__(kFp8Threads) void gemm_fp8_kernel(GemmArgs p) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[2][kStage];
  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int mt = blockIdx.x / p.n_tiles, nt = blockIdx.x - mt * p.n_tiles;
  const int m0 = mt * kFp8Tile, n0 = nt * kFp8Tile;

  // loader: chunk t & 7 of the K tile, rows (t >> 3) + 32 u of the A tile and of the B tile
  const int kc = t & 7, lr = t >> 3;
  const uint8_t* arow[4];
  const uint8_t* brow[4];
  bool aok[4], bok[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int rho = lr + 32 * u;  // the LDS row; for B it holds the row the MFMA order wants there (header)
    const int m = m0 + rho;
    const int n = n0 + (rho & 64) + 32 * ((rho >> 5) & 1) + 8 * ((rho >> 2) & 3) + 4 * ((rho >> 4) & 1) + (rho & 3);
    aok[u] = m < p.M, bok[u] = n < p.N;
    arow[u] = p.a + static_cast<int64_t>(aok[u] ? m : 0) * p.lda + kc * 16;
    brow[u] = p.b + static_cast<int64_t>(bok[u] ? n : 0) * p.ldb + kc * 16;
  }
  uint4 ra[4], rb[4];
  auto issue = [&](int step) {
    const int k = step * kFp8TileK + kc * 16;
    const bool kin = k < p.K;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      ra[u] = uint4{0u, 0u, 0u, 0u}, rb[u] = uint4{0u, 0u, 0u, 0u};
      if (kin && aok[u]) ra[u] = *reinterpret_cast<const uint4*>(arow[u] + step * kFp8TileK);
      if (kin && bok[u]) rb[u] = *reinterpret_cast<const uint4*>(brow[u] + step * kFp8TileK);
    }
  };
  auto commit = [&](int stage) {
    uint8_t* s = lds[stage];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      *reinterpret_cast<uint4*>(s + lds_ofs(lr + 32 * u, kc)) = ra[u];
      *reinterpret_cast<uint4*>(s + kFp8Tile * kFp8TileK + lds_ofs(lr + 32 * u, kc)) = rb[u];
    }
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

  issue(0);
  commit(0);
  __syncthreads();
  for (int s = 0; s < p.k_tiles; ++s) {
    if (s + 1 < p.k_tiles) issue(s + 1);
    const uint8_t* cur = lds[s & 1];
    i32x8 fb[4], fa[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) fb[j] = read_frag(cur + kFp8Tile * kFp8TileK, brow0 + 16 * j, g);
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[i] = read_frag(cur, arow0 + 16 * i, g);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[j], fa[i], acc[i][j], FB, FA, 0, 0, 0, 0);
    if (s + 1 < p.k_tiles) commit((s + 1) & 1);
    __syncthreads();
  }

  // acc[i][j][r] = C[m0 + 64 wm + 16 i + li][n0 + 64 wn + 32 (j >> 1) + 8 g + 4 (j & 1) + r]
  // applied one after the other: each inverse is within 2^+-126, their product need not be
  const float sa_inv = p.sa[1], sb_inv = p.sb[1];
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
      for (int e = 0; e < 8; ++e) o[e] = static_cast<bf16>(acc[i][2 * jj + (e >> 2)][e & 3] * sa_inv * sb_inv + fbias[e]);
      *reinterpret_cast<bf16x8*>(crow + n) = o;
    }
  }
}

}  // namespace

void fp8_gemm(const void* a, const void* b, void* c, const void* bias, int bias_dtype, const void* sa, const void* sb,
              int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int fa, int fb, hipStream_t stream) {
  const Fp8GemmGeometry g = fp8_gemm_check(a, b, c, bias, bias_dtype, sa, sb, M, N, K, lda, ldb, ldc, fa, fb);
  const GemmArgs p{static_cast<const uint8_t*>(a), static_cast<const uint8_t*>(b), static_cast<bf16*>(c), bias,
                   static_cast<const float*>(sa), static_cast<const float*>(sb), lda, ldb, ldc, static_cast<int>(M),
                   static_cast<int>(N), static_cast<int>(K), static_cast<int>(g.n_tiles), g.k_tiles,
                   bias_dtype == static_cast<int>(kF32)};
  const unsigned grid = static_cast<unsigned>(g.grid);
  if (fa == kFp8E4M3) gemm_fp8_kernel<kFp8E4M3, kFp8E4M3><<<grid, kFp8Threads, 0, stream>>>(p);
  else gemm_fp8_kernel<kFp8E5M2, kFp8E4M3><<<grid, kFp8Threads, 0, stream>>>(p);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace fluxmpi
