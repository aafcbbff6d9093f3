// MX block-scaled NT GEMM with fp6 operands on the scaled 128-deep MFMA — gfx950. Reached through
// mx_gemm(fb = 3).
//
//   C[m][n] = bf16( sum over 32-deep K blocks kb of 2^(ea[m][kb] - 127) 2^(eb[n][kb] - 127) (A_blk . B_blk)  (+ bias[n]) )
//
// B [N][K] is e2m3; A [M][K] is e2m3 (the forward) or e3m2 (the input gradient: dy). Both are packed four values
// in three bytes (mx_host.h), 3 K / 4 bytes a row, and carry a scale image, one E8M0 byte per 32 VALUES.
// v_mfma_scale_f32_16x16x128_f8f6f4 takes the two formats independently (cbsz / blgp = 2 for e2m3, 3 for e3m2),
// reads six VGPRs per operand, applies both block scales and accumulates in fp32; the epilogue adds the bias and
// rounds once. The pair is homogeneous in both GEMMs of a Linear: the same stage, LDS and occupancy.
//
// Operand layout. The stored image is what the instruction reads, so that nothing is shuffled here:
//   * lane l = 16 g + r holds row r and K = 32 g .. 32 g + 31 in VGPRs 0 - 5: value i of the 32 at bits
//     6 i .. 6 i + 5 of the six VGPRs read as one little-endian 192-bit string (VGPR 0 lowest). A lane's
//     fragment is therefore the 24 consecutive bytes of block g of the packed row;
//   * lane l supplies, in the byte op_sel picks, the scale of row r and of K block g, as for fp4 (mx4_gemm.hip).
//   This is the dense order of the instruction's description; tests/test_mx6_gpu.py::test_mx6_gemm_exact walks one
//   nonzero over every K position below 256 under per-block scales, which fails for any other order or grouping.
//   * a scale byte 255 makes the row's / column's result NaN even where the block's values are all zero, so
//     blocks past K are forced to 127.
//
// Decisions (a 128-value K step is 96 bytes a row; a lane's fragment is 24 bytes at offset 24 g of it: 8-byte
// aligned, not a 16-byte chunk):
//   * Tile: 128 x 128 of C per workgroup of 4 waves (2 x 2, 4 x 4 MFMA tiles each), as the siblings.
//   * Stage depth 128 values, two stages. 256 values (mx4_gemm.hip's choice, half the barriers) would be
//     2 x (2 x 128 x 192 B + 2 KiB) = 100 KiB and one workgroup per CU, the mixed fp4 pair's fate; at 128 values a
//     workgroup holds 58 KiB (below) and two fit the 160 KiB of a CU for BOTH pairs.
//   * Row pitch 112 bytes (96 + 16). The fragment is read as 3 x ds_read_b64 (b128 needs 16-byte alignment, which
//     24 g has for even g only). A b64 read is served 32 lanes at a time: two lane groups x 16 rows. With a bare
//     96-byte pitch row r starts at dword 24 r, a multiple of 8, and rows r and r + 8 fall on the same banks: two-way
//     conflicts throughout. With 112 bytes row r starts at dword 28 r: the 16 rows start at 16 different multiples
//     of 4 (mod 64), lane group g adds 6 g dwords and read j adds 2 j, so in every read the even groups cover banks
//     4 m, 4 m + 1 and the odd groups 4 m + 2, 4 m + 3 (or the reverse): no two lanes of the 32 meet. 16 bytes of
//     padding per row (2 KiB a tile) keep the loader's ds_write_b128 aligned; an XOR swizzle of 16-byte chunks cannot
//     do this, because a fragment straddles chunks. Counted by hand, not with counters on the device.
//   * Global -> LDS register-staged: a tile is 128 rows x 6 chunks of 16 B = 768 chunks, 3 per lane and operand
//     (chunk index t + 256 u: 6 consecutive lanes read one row's 96 contiguous bytes). Rows past M / N and chunks
//     past the row's 3 K / 4 bytes are zero in registers; K % 32 == 0 lets a row end in the middle of a chunk, which
//     is then an 8-byte load. 24 staging VGPRs.
//   * Scales: mx_gemm.hip's path. Lane t of the workgroup fetches the dword (4 blocks) of LDS row t & 127 of A
//     (t < 128) or B; commit() scatters the 4 bytes to a 1 KiB area [operand][wave row / column][g][r],
//     byte = MFMA tile; a lane reads one dword per operand and op_sel picks the byte.
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

constexpr int kHwE2M3 = 2, kHwE3M2 = 3;           // the instruction's format codes (cbsz / blgp)
constexpr int kStages = 2;
constexpr int kPitch = kMx6RowBytes + 16;          // LDS row pitch: 112 bytes = 28 dwords (the header says why)
constexpr int kTile = kFp8Tile * kPitch;           // one operand's tile of a stage
constexpr int kScales = 2 * kFp8Tile * 4;          // bytes of a stage's scale area: 2 operands x a dword per row
constexpr int kStage = 2 * kTile + kScales;
constexpr int kSmem = kStages * kStage;            // 58 KiB
constexpr int kChunks = kMx6RowBytes / 16;         // 16-byte chunks of a row of a stage
constexpr int kLoads = kFp8Tile * kChunks / kFp8Threads;  // chunks per lane and operand
constexpr unsigned kOnes = 0x7f7f7f7fu;            // four E8M0 bytes of 2^0
static_assert(kFp8Tile * kChunks % kFp8Threads == 0 && kPitch % 16 == 0, "the loader's split");

struct Mx6GemmArgs {
  const uint8_t* a;   // [M][lda]
  const uint8_t* b;   // [N][ldb]
  bf16* c;            // [M][ldc]
  const void* bias;   // [N] or null
  const uint8_t* sa;  // [M][ldsa]
  const uint8_t* sb;  // [N][ldsb]
  int64_t lda, ldb, ldc, ldsa, ldsb;
  int M, N, K, n_tiles, k_tiles, bias_f32;
};

// lane group g's 24 bytes of LDS row `row`: three 8-byte reads
__device__ __forceinline__ i32x8 read_frag(const uint8_t* tile, int row, int g) {
  const uint2* p = reinterpret_cast<const uint2*>(tile + row * kPitch + 24 * g);
  const uint2 v0 = p[0], v1 = p[1], v2 = p[2];
  return i32x8{static_cast<int>(v0.x), static_cast<int>(v0.y), static_cast<int>(v1.x), static_cast<int>(v1.y),
               static_cast<int>(v2.x), static_cast<int>(v2.y), 0, 0};
}

// the row of tile `rho` order -> the B row of the tile that the loader puts in LDS row rho (gemm_fp8.hip)
__device__ __forceinline__ int b_row(int rho) {
  return (rho & 64) + 32 * ((rho >> 5) & 1) + 8 * ((rho >> 2) & 3) + 4 * ((rho >> 4) & 1) + (rho & 3);
}

// the 4 MFMAs of A tile I: op_sel must be a constant, so the tile indices are template parameters
template <int HWA, int I, int... J>
__device__ __forceinline__ void mfma_row(f32x4 (&acc)[4], const i32x8 (&fb)[4], const i32x8& fa, int sb, int sa,
                                         std::integer_sequence<int, J...>) {
  ((acc[J] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[J], fa, acc[J], kHwE2M3, HWA, J, sb, I, sa)), ...);
}

template <int HWA>
__global__ __launch_bounds__(kFp8Threads) void mx6_gemm_kernel(Mx6GemmArgs p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int mt = blockIdx.x / p.n_tiles, nt = blockIdx.x - mt * p.n_tiles;
  const int m0 = mt * kFp8Tile, n0 = nt * kFp8Tile;
  const int row_bytes = p.K / 4 * 3;  // of a whole row, either operand

  // operand loader: chunk index t + 256 u = 6 rho + ch of each tile
  const uint8_t* arow[kLoads];
  const uint8_t* brow[kLoads];
  bool aok[kLoads], bok[kLoads];
  int kofs[kLoads], dst[kLoads];
#pragma unroll
  for (int u = 0; u < kLoads; ++u) {
    const int idx = t + kFp8Threads * u, rho = idx / kChunks, ch = idx - rho * kChunks;
    const int m = m0 + rho, n = n0 + b_row(rho);  // the LDS row; for B it holds the row the MFMA order wants there
    aok[u] = m < p.M, bok[u] = n < p.N;
    kofs[u] = ch * 16, dst[u] = rho * kPitch + ch * 16;
    arow[u] = p.a + static_cast<int64_t>(aok[u] ? m : 0) * p.lda + kofs[u];
    brow[u] = p.b + static_cast<int64_t>(bok[u] ? n : 0) * p.ldb + kofs[u];
  }
  // scale loader: the dword of LDS row t & 127 of A (waves 0, 1) or of B (waves 2, 3)
  const int srho = t & 127, s_is_b = wave >> 1;
  const int sidx = s_is_b ? n0 + b_row(srho) : m0 + srho;
  const bool sok = sidx < (s_is_b ? p.N : p.M);
  const uint8_t* srow = (s_is_b ? p.sb : p.sa) + static_cast<int64_t>(sok ? sidx : 0) * (s_is_b ? p.ldsb : p.ldsa);
  // where its bytes go: dword [operand][srho >> 6][g][srho & 15], byte (srho >> 4) & 3
  constexpr int sbase = 2 * kTile;
  const int sdst = sbase + s_is_b * (kScales / 2) + (srho >> 6) * 256 + (srho & 15) * 4 + ((srho >> 4) & 3);
  const int kblocks = p.K / kMxBlock, sdwords = (kblocks + 3) >> 2;

  uint4 ra[kLoads], rb[kLoads];
  unsigned rs;
  // a chunk with `have` bytes of its row left: 16, 8 (K % 32 == 0 ends a row on a multiple of 24) or none
  auto fetch = [](const uint8_t* src, int have, bool ok) {
    uint4 v{0u, 0u, 0u, 0u};
    if (ok && have >= 16) {
      v = *reinterpret_cast<const uint4*>(src);
    } else if (ok && have >= 8) {
      const uint2 h = *reinterpret_cast<const uint2*>(src);
      v.x = h.x, v.y = h.y;
    }
    return v;
  };
  auto issue = [&](int step) {
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
      const int have = row_bytes - step * kMx6RowBytes - kofs[u];
      ra[u] = fetch(arow[u] + step * kMx6RowBytes, have, aok[u]);
      rb[u] = fetch(brow[u] + step * kMx6RowBytes, have, bok[u]);
    }
    rs = kOnes;
    if (sok && step < sdwords) rs = *reinterpret_cast<const uint32_t*>(srow + 4 * step);
    const int left = kblocks - 4 * step;  // blocks of this K step inside K
    if (left < 4) {
      const unsigned keep = left <= 0 ? 0u : (1u << (8 * left)) - 1u;
      rs = (rs & keep) | (kOnes & ~keep);
    }
  };
  auto commit = [&](int stage) {
    uint8_t* s = lds + stage * kStage;
#pragma unroll
    for (int u = 0; u < kLoads; ++u) {
      *reinterpret_cast<uint4*>(s + dst[u]) = ra[u];
      *reinterpret_cast<uint4*>(s + kTile + dst[u]) = rb[u];
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
  const int sa_ofs = sbase + wm * 256 + lane * 4, sb_ofs = sbase + kScales / 2 + wn * 256 + lane * 4;

  issue(0);
  commit(0);
  __syncthreads();
  for (int s = 0; s < p.k_tiles; ++s) {
    if (s + 1 < p.k_tiles) issue(s + 1);
    const uint8_t* cur = lds + (s & 1) * kStage;
    i32x8 fb[4], fa[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) fb[j] = read_frag(cur + kTile, brow0 + 16 * j, g);
#pragma unroll
    for (int i = 0; i < 4; ++i) fa[i] = read_frag(cur, arow0 + 16 * i, g);
    const int sa = *reinterpret_cast<const int*>(cur + sa_ofs);
    const int sb = *reinterpret_cast<const int*>(cur + sb_ofs);
    constexpr std::make_integer_sequence<int, 4> tiles{};
    mfma_row<HWA, 0>(acc[0], fb, fa[0], sb, sa, tiles);
    mfma_row<HWA, 1>(acc[1], fb, fa[1], sb, sa, tiles);
    mfma_row<HWA, 2>(acc[2], fb, fa[2], sb, sa, tiles);
    mfma_row<HWA, 3>(acc[3], fb, fa[3], sb, sa, tiles);
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
void launch(const Mx6GemmArgs& p, unsigned grid, hipStream_t stream) {
  allow_dynamic_lds(reinterpret_cast<const void*>(&mx6_gemm_kernel<HWA>), kSmem);
  mx6_gemm_kernel<HWA><<<grid, kFp8Threads, kSmem, stream>>>(p);
}

}  // namespace

void mx6_gemm_launch(const void* a, const void* b, void* c, const void* bias, int bias_f32, const void* sa,
                     const void* sb, int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldc, int64_t ldsa,
                     int64_t ldsb, int fa, int64_t n_tiles, int k_tiles, int64_t grid, hipStream_t stream) {
  const Mx6GemmArgs p{static_cast<const uint8_t*>(a), static_cast<const uint8_t*>(b), static_cast<bf16*>(c), bias,
                      static_cast<const uint8_t*>(sa), static_cast<const uint8_t*>(sb), lda, ldb, ldc, ldsa, ldsb,
                      static_cast<int>(M), static_cast<int>(N), static_cast<int>(K), static_cast<int>(n_tiles), k_tiles,
                      bias_f32};
  if (fa == kMxE2M3) launch<kHwE2M3>(p, static_cast<unsigned>(grid), stream);
  else launch<kHwE3M2>(p, static_cast<unsigned>(grid), stream);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace fluxmpi
