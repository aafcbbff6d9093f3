// MX block-scaled NT GEMM with fp4 (e2m1) operands on the scaled 128-deep MFMA — gfx950. Reached through
// mx_gemm(fb = 2).
//
//   C[m][n] = bf16( sum over 32-deep K blocks kb of 2^(ea[m][kb] - 127) 2^(eb[n][kb] - 127) (A_blk . B_blk)  (+ bias[n]) )
//
// B [N][K] is e2m1, two values per byte (element 2 i in the low nibble of byte i), K / 2 bytes a row; A [M][K] is
// e2m1 as well (the forward) or e4m3, one byte per value (the input gradient: dy as it is stored today). Both
// carry mx_host.h's scale image, one E8M0 byte per 32 VALUES. v_mfma_scale_f32_16x16x128_f8f6f4 takes the two
// formats independently (cbsz / blgp = 4 for fp4), applies both block scales and accumulates in fp32; the
// epilogue adds the bias and rounds once.
//
// Operand layout, as found on MI355X with a one-wave probe (one nonzero in each operand, every pair of
// positions; then one lane group's scale byte changed at a time), not taken from the documentation:
//   * an fp4 operand uses 4 VGPRs. Lane l = 16 g + r holds row r and K = 32 g .. 32 g + 31: nibble n of VGPR v is
//     K = 32 g + 8 v + n, the low nibble first. So a lane's 16 bytes are 16 consecutive bytes of the packed row.
//   * lane l supplies, in the byte op_sel picks, the scale of row r and of K block g: for fp4 that is the 32
//     values the lane holds itself.
//   * in the mixed pair the fp4 operand's K above meets the fp8 operand's K of mx_gemm.hip's finding (VGPRs 0 - 3
//     of lane group g are K = 16 g .. + 15, VGPRs 4 - 7 are K = 64 + 16 g .. + 15), and the fp8 operand's scale of
//     lane group g is block g of that order. Nothing else moves.
//   * a scale byte 255 makes the row's / column's result NaN even where the block's values are all zero.
//
// Decisions (an fp4 K tile of 128 values is 64 bytes a row, so the byte budget of mx_gemm.hip buys twice the K):
//   * Tile and stages: 128 x 128 of C per workgroup of 4 waves (2 x 2, 4 x 4 MFMA tiles each), as mx_gemm.hip, and
//     2 LDS stages; but a stage is 256 VALUES deep: one 128-byte LDS row of fp4 carries TWO MFMA K steps, and its
//     two scale dwords travel with it. e2m1 x e2m1 is 2 x (16 + 16 + 2) KiB = 68 KiB, two workgroups per CU in
//     160 KiB like the fp8 kernel, with half as many barriers, global-load rounds and loop trips per MFMA. The
//     larger tile was not taken: 256 x 128 needs 128 accumulator registers and leaves one workgroup per CU.
//   * Mixed pair in step: a stage is 256 values for BOTH operands, so A's rows are 256 bytes (two 128-byte
//     halves, one per MFMA K step) beside B's 128 bytes; K step h reads chunks 8 h + g and 8 h + 4 + g of A and
//     chunk 4 h + g of B. 2 x (32 + 16 + 2) KiB = 100 KiB: one workgroup per CU. The alternative, 128-value
//     stages with 64-byte B rows, halves the stage but brings back a barrier per MFMA K step.
//   * Global -> LDS stays register-staged (not global_load_lds_dwordx4 as mx_wgrad.hip): the ragged edges (rows
//     past M / N, chunks past K) are zero-filled in registers, and with fp4 the staging registers are 32 for 256
//     values of K where mx_gemm.hip holds 32 for 128.
//   * Swizzle: a lane's fragment is ONE 16-byte chunk (c = 4 h + g) of a 128-byte row, stored at chunk
//     c ^ (row & 7). The 16 lanes of a group read rows r .. r + 15 at one c: rows r and r + 8 share a chunk
//     position, 8 rows cover the 8 positions of a 128-byte row, the same spread as gemm_fp8.hip's reads (bank
//     conflicts were not counted on the device); the loader's ds_write_b128 (8 lanes a row, consecutive c) is conflict-free too. A's
//     256-byte rows swizzle the low 3 bits of the chunk index the same way inside each half.
//   * Scales: mx_gemm.hip's path, doubled. Lane t of the workgroup fetches the TWO dwords (8 blocks) of LDS row
//     t & 127 of A (t < 128) or B; blocks past K are forced to 127 (a stale 255 would make a NaN out of zeros).
//     commit() scatters the 8 bytes to a 2 KiB area [operand][h][wave row / column][g][r], byte = MFMA tile; a
//     lane reads one dword per operand and K step and op_sel picks the byte.
// B is the first MFMA operand and the loader orders B's rows so that a lane ends with 8 consecutive columns of
// C, as gemm_fp8.hip describes.
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

constexpr int kHwE4M3 = 0, kHwE2M1 = 4;          // the instruction's format codes (cbsz / blgp)
constexpr int kStages = 2;
constexpr int kBRow = kMx4TileK / 2;             // bytes of a B row of a stage
constexpr int kScales = 2 * 2 * kFp8Tile * 4;    // bytes of a stage's scale area: 2 operands x 2 K steps x a dword per row
constexpr unsigned kOnes = 0x7f7f7f7fu;          // four E8M0 bytes of 2^0

struct Mx4GemmArgs {
  const uint8_t* a;   // [M][lda]
  const uint8_t* b;   // [N][ldb]
  bf16* c;            // [M][ldc]
  const void* bias;   // [N] or null
  const uint8_t* sa;  // [M][ldsa]
  const uint8_t* sb;  // [N][ldsb]
  int64_t lda, ldb, ldc, ldsa, ldsb;
  int M, N, K, n_tiles, k_tiles, bias_f32;
};

// byte offset of 16-byte chunk `c` of row `r` in an LDS tile whose rows are ROW bytes (128 or 256)
template <int ROW>
__device__ __forceinline__ int lds_ofs(int r, int c) { return r * ROW + ((c ^ (r & 7)) << 4); }

// K step h of a stage, lane group g: an fp4 operand is chunk 4 h + g; an fp8 one is chunks 8 h + g, 8 h + 4 + g
template <int HW>
__device__ __forceinline__ i32x8 read_frag(const uint8_t* tile, int row, int g, int h) {
  if constexpr (HW == kHwE2M1) {
    const uint4 lo = *reinterpret_cast<const uint4*>(tile + lds_ofs<128>(row, 4 * h + g));
    return i32x8{static_cast<int>(lo.x), static_cast<int>(lo.y), static_cast<int>(lo.z), static_cast<int>(lo.w), 0, 0, 0, 0};
  } else {
    const uint4 lo = *reinterpret_cast<const uint4*>(tile + lds_ofs<256>(row, 8 * h + g));
    const uint4 hi = *reinterpret_cast<const uint4*>(tile + lds_ofs<256>(row, 8 * h + 4 + g));
    return i32x8{static_cast<int>(lo.x), static_cast<int>(lo.y), static_cast<int>(lo.z), static_cast<int>(lo.w),
                 static_cast<int>(hi.x), static_cast<int>(hi.y), static_cast<int>(hi.z), static_cast<int>(hi.w)};
  }
}

// the row of tile `rho` order -> the B row of the tile that the loader puts in LDS row rho (gemm_fp8.hip)
__device__ __forceinline__ int b_row(int rho) {
  return (rho & 64) + 32 * ((rho >> 5) & 1) + 8 * ((rho >> 2) & 3) + 4 * ((rho >> 4) & 1) + (rho & 3);
}

// the 4 MFMAs of A tile I: op_sel must be a constant, so the tile indices are template parameters
template <int HWA, int I, int... J>
__device__ __forceinline__ void mfma_row(f32x4 (&acc)[4], const i32x8 (&fb)[4], const i32x8& fa, int sb, int sa,
                                         std::integer_sequence<int, J...>) {
  ((acc[J] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[J], fa, acc[J], kHwE2M1, HWA, J, sb, I, sa)), ...);
}

template <int HWA>
struct Shape {
  static constexpr int kARow = HWA == kHwE2M1 ? kMx4TileK / 2 : kMx4TileK;  // bytes of an A row of a stage
  static constexpr int kAChunks = kARow / 128;                              // 16-byte chunks per lane and A row
  static constexpr int kATile = kFp8Tile * kARow, kBTile = kFp8Tile * kBRow;
  static constexpr int kStage = kATile + kBTile + kScales;
  static constexpr int kSmem = kStages * kStage;
};

template <int HWA>
__global__ __launch_bounds__(kFp8Threads) void mx4_gemm_kernel(Mx4GemmArgs p) {
  using S = Shape<HWA>;
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int mt = blockIdx.x / p.n_tiles, nt = blockIdx.x - mt * p.n_tiles;
  const int m0 = mt * kFp8Tile, n0 = nt * kFp8Tile;
  const int a_bytes = HWA == kHwE2M1 ? p.K / 2 : p.K, b_bytes = p.K / 2;  // of a whole row

  // operand loader: chunk t & 7 (+ 8 for the second half of an fp8 A row), rows (t >> 3) + 32 u of each tile
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
  // scale loader: the two dwords of LDS row t & 127 of A (waves 0, 1) or of B (waves 2, 3)
  const int srho = t & 127, s_is_b = wave >> 1;
  const int sidx = s_is_b ? n0 + b_row(srho) : m0 + srho;
  const bool sok = sidx < (s_is_b ? p.N : p.M);
  const uint8_t* srow = (s_is_b ? p.sb : p.sa) + static_cast<int64_t>(sok ? sidx : 0) * (s_is_b ? p.ldsb : p.ldsa);
  // where its bytes go: dword [operand][h][srho >> 6][g][srho & 15], byte (srho >> 4) & 3
  const int sbase = S::kATile + S::kBTile;
  const int sdst = sbase + s_is_b * (kScales / 2) + (srho >> 6) * 256 + (srho & 15) * 4 + ((srho >> 4) & 3);
  const int kblocks = p.K / kMxBlock, sdwords = (kblocks + 3) >> 2;

  uint4 ra[4 * S::kAChunks], rb[4];
  unsigned rs[2];
  auto issue = [&](int step) {
    const int kb_ofs = step * kBRow + kc * 16;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      rb[u] = uint4{0u, 0u, 0u, 0u};
      if (kb_ofs < b_bytes && bok[u]) rb[u] = *reinterpret_cast<const uint4*>(brow[u] + step * kBRow);
#pragma unroll
      for (int e = 0; e < S::kAChunks; ++e) {
        const int ka_ofs = step * S::kARow + e * 128 + kc * 16;
        ra[u * S::kAChunks + e] = uint4{0u, 0u, 0u, 0u};
        if (ka_ofs < a_bytes && aok[u])
          ra[u * S::kAChunks + e] = *reinterpret_cast<const uint4*>(arow[u] + step * S::kARow + e * 128);
      }
    }
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      rs[h] = kOnes;
      if (sok && 2 * step + h < sdwords) rs[h] = *reinterpret_cast<const uint32_t*>(srow + 8 * step + 4 * h);
      const int left = kblocks - 8 * step - 4 * h;  // blocks of this K step inside K
      if (left < 4) {
        const unsigned keep = left <= 0 ? 0u : (1u << (8 * left)) - 1u;
        rs[h] = (rs[h] & keep) | (kOnes & ~keep);
      }
    }
  };
  auto commit = [&](int stage) {
    uint8_t* s = lds + stage * S::kStage;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      *reinterpret_cast<uint4*>(s + S::kATile + lds_ofs<kBRow>(lr + 32 * u, kc)) = rb[u];
#pragma unroll
      for (int e = 0; e < S::kAChunks; ++e)
        *reinterpret_cast<uint4*>(s + lds_ofs<S::kARow>(lr + 32 * u, kc + 8 * e)) = ra[u * S::kAChunks + e];
    }
#pragma unroll
    for (int h = 0; h < 2; ++h)
#pragma unroll
      for (int g = 0; g < 4; ++g) s[sdst + h * 512 + g * 64] = static_cast<uint8_t>(rs[h] >> (8 * g));
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
  const int sa_ofs = sbase + wm * 256 + lane * 4, sb_ofs = sbase + kScales / 2 + wn * 256 + lane * 4;

  issue(0);
  commit(0);
  __syncthreads();
  for (int s = 0; s < p.k_tiles; ++s) {
    if (s + 1 < p.k_tiles) issue(s + 1);
    const uint8_t* cur = lds + (s & 1) * S::kStage;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      i32x8 fb[4], fa[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) fb[j] = read_frag<kHwE2M1>(cur + S::kATile, brow0 + 16 * j, g, h);
#pragma unroll
      for (int i = 0; i < 4; ++i) fa[i] = read_frag<HWA>(cur, arow0 + 16 * i, g, h);
      const int sa = *reinterpret_cast<const int*>(cur + sa_ofs + h * 512);
      const int sb = *reinterpret_cast<const int*>(cur + sb_ofs + h * 512);
      constexpr std::make_integer_sequence<int, 4> tiles{};
      mfma_row<HWA, 0>(acc[0], fb, fa[0], sb, sa, tiles);
      mfma_row<HWA, 1>(acc[1], fb, fa[1], sb, sa, tiles);
      mfma_row<HWA, 2>(acc[2], fb, fa[2], sb, sa, tiles);
      mfma_row<HWA, 3>(acc[3], fb, fa[3], sb, sa, tiles);
    }
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

template <int HWA>
void launch(const Mx4GemmArgs& p, unsigned grid, hipStream_t stream) {
  allow_dynamic_lds(reinterpret_cast<const void*>(&mx4_gemm_kernel<HWA>), Shape<HWA>::kSmem);
  mx4_gemm_kernel<HWA><<<grid, kFp8Threads, Shape<HWA>::kSmem, stream>>>(p);
}

}  // namespace

void mx4_gemm_launch(const void* a, const void* b, void* c, const void* bias, int bias_f32, const void* sa,
                     const void* sb, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldsa,
                     int64_t ldsb, int fa, int64_t n_tiles, int k_tiles, int64_t grid, hipStream_t stream) {
  const Mx4GemmArgs p{static_cast<const uint8_t*>(a), static_cast<const uint8_t*>(b), static_cast<bf16*>(c), bias,
                      static_cast<const uint8_t*>(sa), static_cast<const uint8_t*>(sb), lda, ldb, ldc, ldsa, ldsb,
                      static_cast<int>(M), static_cast<int>(N), static_cast<int>(K), static_cast<int>(n_tiles), k_tiles,
                      bias_f32};
  if (fa == kFp8E2M1) launch<kHwE2M1>(p, static_cast<unsigned>(grid), stream);
  else launch<kHwE4M3>(p, static_cast<unsigned>(grid), stream);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace fluxmpi
