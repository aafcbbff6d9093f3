// MX (block-scaled) fp8 weight gradient on the scaled 128-deep MFMA, split-K over the reduction — gfx950.
//
//   ws[s][m][n] = sum over the K tiles of split s, over their 32-deep blocks kb, of
//                 2^(ea[m][kb] - 127) 2^(eb[n][kb] - 127) (A_blk . B_blk)                      (fp32)
//
// A [M][K] (e4m3 or e5m2) and B [N][K] (e4m3) are fp8, k-contiguous, with mx_host.h's E8M0 scale images. For a
// Linear A is dy's transposed image (M = n_out), B is x's (N = n_in) and K is the token count: a small output
// and a very long reduction, which mx_gemm.hip's 128 x 128 tile, one workgroup per tile, serves badly (108
// workgroups of four waves for ViT-B/16's qkv, each operand re-read once per 128 columns of the other). Here:
//   * a workgroup of 8 waves (2 in M x 4 in N, 128 x 64 each: 8 x 4 MFMA tiles, 128 accumulator registers) owns
//     256 x 256 of the output and the K tiles of one split; the grid is tiles x splits in wgrad256.hip's
//     XCD-aware order (the workgroups of a split, which read the same K range, share an L2);
//   * operands go global -> LDS with global_load_lds_dwordx4, no staging registers: a wave instruction fills
//     1 KiB = 8 rows of the stage, lane l the 16-byte slot l & 7 of row l >> 3, so the chunk ^ (row & 7)
//     swizzle of mx_gemm.hip is applied to the lane's SOURCE chunk. A chunk past K or a row past M / N reads
//     a zero line. Two stages of [256 A rows + 256 B rows][128 B] + 2 KiB of scales = 132 KiB (dynamic), one
//     workgroup per CU. Step s + 1 is in flight under step s's MFMAs; vmcnt(0) + a barrier publish it;
//   * the instruction, its operand order (B first), the fragment chunks g and 4 + g, the scale operand (lane l:
//     row l & 15, K block l >> 4, op_sel = the tile's byte of a dword) and B's row order in LDS are
//     mx_gemm.hip's, documented there. Scales: lane t of the workgroup fetches the dword (4 K blocks) of LDS
//     row t & 255 of A (waves 0 - 3) or B (waves 4 - 7) and scatters its bytes into the consumer's order,
//     dword [operand][64-row group][K group g][li], byte = the row's 16-row tile within the group; a wave
//     reads two such dwords for its eight A tiles and one for its four B tiles per K step. Rows past M / N
//     count as 127, the bytes of K blocks past K are forced to 127 (the padding may hold anything);
//   * B's four fragments are read once per K step and A's one at a time: 40 fragment registers;
//   * the epilogue writes the fp32 tile with 16-byte stores in the accumulator's own layout (a lane holds 8
//     consecutive columns), masked at the edges. No atomics: gemm_splitk_reduce sums the splits in order.
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

constexpr int kTile = kMxWgTile;
constexpr int kOperand = kTile * kFp8TileK;  // bytes of one operand's rows in a stage
constexpr int kScaleArea = kTile * 4;        // bytes of one operand's scale area: a dword per row
constexpr int kStage = 2 * kOperand + 2 * kScaleArea;
constexpr int kSmem = 2 * kStage;
constexpr int kPieces = kOperand / 1024 / 8;  // 1 KiB DMA pieces per wave, operand and step
constexpr unsigned kOnes = 0x7f7f7f7fu;       // four E8M0 bytes of 2^0

__device__ __attribute__((aligned(16))) uint4 g_mx_zero[1];  // source of masked chunks

struct MxWgradArgs {
  const uint8_t* a;   // [M][lda]
  const uint8_t* b;   // [N][ldb]
  float* ws;          // [splits][M][N]
  const uint8_t* sa;  // [M][ldsa]
  const uint8_t* sb;  // [N][ldsb]
  int64_t lda, ldb, ldsa, ldsb;
  int M, N, K, n_tiles, tiles, k_tiles, splits;
};

// byte offset of chunk `c` of row `r` inside an operand's [256][128 B] LDS tile
__device__ __forceinline__ int lds_ofs(int r, int c) { return r * kFp8TileK + ((c ^ (r & 7)) << 4); }

// lane group g's operand registers: K bytes 16 g .. + 15 (VGPRs 0 - 3) and 64 + 16 g .. + 15 (VGPRs 4 - 7).
// __restrict__: the reads get an alias scope of their own, without which the waitcnt pass takes them to
// read what the DMA just issued writes and drains it before the MFMAs
__device__ __forceinline__ i32x8 read_frag(const uint8_t* __restrict__ tile, int ofs_lo, int ofs_hi) {
  const uint4 lo = *reinterpret_cast<const uint4*>(tile + ofs_lo);
  const uint4 hi = *reinterpret_cast<const uint4*>(tile + ofs_hi);
  return i32x8{static_cast<int>(lo.x), static_cast<int>(lo.y), static_cast<int>(lo.z), static_cast<int>(lo.w),
               static_cast<int>(hi.x), static_cast<int>(hi.y), static_cast<int>(hi.z), static_cast<int>(hi.w)};
}

// LDS row rho of the B tile -> the B row the MFMA order wants there (mx_gemm.hip's b_row over 256 rows)
__device__ __forceinline__ int b_row(int rho) {
  return (rho & 192) + 32 * ((rho >> 5) & 1) + 8 * ((rho >> 2) & 3) + 4 * ((rho >> 4) & 1) + (rho & 3);
}

// the 4 MFMAs of A tile I: op_sel must be a constant, so the tile indices are template parameters
template <int FA, int FB, int I, int... J>
__device__ __forceinline__ void mfma_row(f32x4 (&acc)[4], const i32x8 (&fb)[4], const i32x8& fa, int sb, int sa,
                                         std::integer_sequence<int, J...>) {
  ((acc[J] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fb[J], fa, acc[J], FB, FA, J, sb, I & 3, sa)), ...);
}

template <int FA, int FB>
__global__ __launch_bounds__(kMxWgThreads) void mx_wgrad_kernel(MxWgradArgs p) {
  extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  // wgrad256.hip's bijective XCD-aware order: an XCD gets a contiguous (split-major) range of ids
  const int total = static_cast<int>(gridDim.x);
  int lid = blockIdx.x;
  if (total >= 8) {
    const int q = total / 8, r = total % 8, xcd = lid % 8, pos = lid / 8;
    lid = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + pos;
  }
  const int split = lid / p.tiles, tile = lid - split * p.tiles;
  const int mt = tile / p.n_tiles, nt = tile - mt * p.n_tiles;
  const int m0 = mt * kTile, n0 = nt * kTile;
  const int kt0 = mx_wgrad_first_tile(p.k_tiles, p.splits, split);
  const int nk = mx_wgrad_first_tile(p.k_tiles, p.splits, split + 1) - kt0;  // >= 1

  // operand DMA: piece j of this wave = LDS rows 32 wave + 8 j + (lane >> 3); the lane's slot lane & 7 of its
  // row holds chunk (lane & 7) ^ (row & 7), and row & 7 = lane >> 3
  const int kc = (lane & 7) ^ (lane >> 3);
  // addresses as integers and the masked source chosen by a select: one load per piece whatever the mask. B's
  // rows of pieces j = 0 .. 3 are b_row(rho0 + 8 j) = b_row(rho0) + 16 (j & 1) + 4 (j >> 1)
  const int rho0 = 32 * wave + (lane >> 3);
  const int am = m0 + rho0, bn = n0 + b_row(rho0);
  const uint64_t zero_line = reinterpret_cast<uint64_t>(g_mx_zero);
  const uint64_t a_base = reinterpret_cast<uint64_t>(p.a) + static_cast<uint64_t>(am) * p.lda + kc * 16;
  const uint64_t b_base = reinterpret_cast<uint64_t>(p.b) + static_cast<uint64_t>(bn) * p.ldb + kc * 16;
  // scale loader: the dword of LDS row t & 255 of A (waves 0 - 3) or of B (waves 4 - 7)
  const int srho = t & 255, s_is_b = wave >> 2;
  const int sidx = s_is_b ? n0 + b_row(srho) : m0 + srho;
  const bool sok = sidx < (s_is_b ? p.N : p.M);
  const uint8_t* srow = (s_is_b ? p.sb : p.sa) + static_cast<int64_t>(sok ? sidx : 0) * (s_is_b ? p.ldsb : p.ldsa);
  // where its bytes go: dword [operand][srho >> 6][g][srho & 15], byte (srho >> 4) & 3
  const int sdst = 2 * kOperand + s_is_b * kScaleArea + (((srho >> 6) * 4) * 16 + (srho & 15)) * 4 + ((srho >> 4) & 3);
  const int kblocks = p.K / kMxBlock;

  typedef __attribute__((address_space(3))) char lds_char;
  typedef __attribute__((address_space(1))) void gl_void;
  unsigned rs, rs_keep;
  // step: the K tile's index in the whole reduction; `live` false (the step behind the split's last) moves
  // nothing but zero lines, so the loop body has no branch and the compiler's schedule stays as written. The
  // scale dword goes first, so that nothing but it is waited for when commit() needs it; rows past M / N
  // read row 0's dword and drop it, and the bytes of K blocks past K are replaced in commit()
  auto issue = [&](int step, int stage, bool live) {
    uint8_t* s = lds + stage * kStage;
    step = live ? step : kt0;
    rs = *reinterpret_cast<const uint32_t*>(srow + 4 * static_cast<int64_t>(step));
    const int left = kblocks - 4 * step;  // >= 1: blocks of this K tile inside K
    rs_keep = !sok ? 0u : left < 4 ? (1u << (8 * left)) - 1u : 0xffffffffu;
    const uint64_t kofs = static_cast<uint64_t>(step) * kFp8TileK;
    const bool kin = live & (step * kFp8TileK + kc * 16 < p.K);
#pragma unroll
    for (int j = 0; j < kPieces; ++j) {
      const uint64_t src =
          (kin & (am + 8 * j < p.M)) ? a_base + kofs + static_cast<uint64_t>(8 * j) * p.lda : zero_line;
      __builtin_amdgcn_global_load_lds(reinterpret_cast<gl_void*>(src), (lds_char*)(s + (wave * kPieces + j) * 1024),
                                       16, 0, 0);
    }
#pragma unroll
    for (int j = 0; j < kPieces; ++j) {
      const int dn = 16 * (j & 1) + 4 * (j >> 1);
      const uint64_t src = (kin & (bn + dn < p.N)) ? b_base + kofs + static_cast<uint64_t>(dn) * p.ldb : zero_line;
      __builtin_amdgcn_global_load_lds(reinterpret_cast<gl_void*>(src),
                                       (lds_char*)(s + kOperand + (wave * kPieces + j) * 1024), 16, 0, 0);
    }
  };
  auto commit = [&](int stage) {
    uint8_t* s = lds + stage * kStage;
    const unsigned v = (rs & rs_keep) | (kOnes & ~rs_keep);
#pragma unroll
    for (int g = 0; g < 4; ++g) s[sdst + g * 64] = static_cast<uint8_t>(v >> (8 * g));
  };
  // every DMA and LDS access of this wave has landed, then every wave's. The scheduling barriers keep the
  // step's MFMAs in front of the wait: behind it they would start only once the next step's operands are in
  auto publish = [&]() {
    __builtin_amdgcn_sched_barrier(0);
    __builtin_amdgcn_s_waitcnt(0);
    __syncthreads();
    __builtin_amdgcn_sched_barrier(0);
  };

  f32x4 acc[8][4];
#pragma unroll
  for (int i = 0; i < 8; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int li = lane & 15, g = lane >> 4;
  const int wm = wave >> 2, wn = wave & 3;
  // fragment offsets inside an operand's tile: rows 16 apart share row & 7, so a tile is + 16 * 128 bytes
  const int a_lo = lds_ofs(128 * wm + li, g), a_hi = lds_ofs(128 * wm + li, g + 4);
  const int b_lo = kOperand + lds_ofs(64 * wn + li, g), b_hi = kOperand + lds_ofs(64 * wn + li, g + 4);
  const int sa_ofs = 2 * kOperand + (2 * wm * 64 + lane) * 4, sb_ofs = 2 * kOperand + kScaleArea + (wn * 64 + lane) * 4;
  constexpr int kTileRows = 16 * kFp8TileK;  // bytes from one MFMA tile's rows to the next

  issue(kt0, 0, true);
  commit(0);
  publish();
  for (int s = 0; s < nk; ++s) {
    // stage (s + 1) & 1 was last read in step s - 1, which every wave left behind at the barrier
    issue(kt0 + s + 1, (s + 1) & 1, s + 1 < nk);
    const uint8_t* cur = lds + (s & 1) * kStage;
    i32x8 fb[4], fa[2];
#pragma unroll
    for (int j = 0; j < 4; ++j) fb[j] = read_frag(cur, b_lo + j * kTileRows, b_hi + j * kTileRows);
    const int sb = *reinterpret_cast<const int*>(cur + sb_ofs);
    const int sa0 = *reinterpret_cast<const int*>(cur + sa_ofs), sa1 = *reinterpret_cast<const int*>(cur + sa_ofs + 256);
    fa[0] = read_frag(cur, a_lo, a_hi);
    constexpr std::make_integer_sequence<int, 4> tiles{};
    // A tile I's MFMAs run under the read of tile I + 1; the scheduling barrier keeps the compiler from
    // reading all eight first (96 fragment registers, and spills)
#define FLUXMPI_MX_WGRAD_ROW(I, SA)                                                                            \
  if ((I) < 7) fa[((I) + 1) & 1] = read_frag(cur, a_lo + ((I) + 1) * kTileRows, a_hi + ((I) + 1) * kTileRows); \
  mfma_row<FA, FB, (I)>(acc[(I)], fb, fa[(I) & 1], sb, (SA), tiles);                                           \
  __builtin_amdgcn_sched_barrier(0);
    FLUXMPI_MX_WGRAD_ROW(0, sa0)
    FLUXMPI_MX_WGRAD_ROW(1, sa0)
    FLUXMPI_MX_WGRAD_ROW(2, sa0)
    FLUXMPI_MX_WGRAD_ROW(3, sa0)
    FLUXMPI_MX_WGRAD_ROW(4, sa1)
    FLUXMPI_MX_WGRAD_ROW(5, sa1)
    FLUXMPI_MX_WGRAD_ROW(6, sa1)
    FLUXMPI_MX_WGRAD_ROW(7, sa1)
#undef FLUXMPI_MX_WGRAD_ROW
    commit((s + 1) & 1);
    publish();
  }

  // acc[i][j][r] = ws[split][m0 + 128 wm + 16 i + li][n0 + 64 wn + 32 (j >> 1) + 8 g + 4 (j & 1) + r]
  float* out = p.ws + static_cast<int64_t>(split) * p.M * p.N;
#pragma unroll
  for (int i = 0; i < 8; ++i) {
    const int m = m0 + 128 * wm + 16 * i + li;
    if (m >= p.M) continue;
    float* crow = out + static_cast<int64_t>(m) * p.N;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int n = n0 + 64 * wn + 32 * jj + 8 * g;
      if (n >= p.N) continue;  // N % 8 == 0: the 8 columns are inside N together
      *reinterpret_cast<f32x4*>(crow + n) = acc[i][2 * jj];
      *reinterpret_cast<f32x4*>(crow + n + 4) = acc[i][2 * jj + 1];
    }
  }
}

template <int FA>
void launch(const MxWgradArgs& p, unsigned grid, hipStream_t stream) {
  allow_dynamic_lds(reinterpret_cast<const void*>(&mx_wgrad_kernel<FA, kFp8E4M3>), kSmem);
  mx_wgrad_kernel<FA, kFp8E4M3><<<grid, kMxWgThreads, kSmem, stream>>>(p);
}

}  // namespace

void mx_wgrad(const void* a, const void* b, float* ws, const void* sa, const void* sb, int64_t M, int64_t N, int64_t K,
              int64_t lda, int64_t ldb, int64_t ldsa, int64_t ldsb, int fa, int fb, int splits, hipStream_t stream) {
  const MxWgradGeometry g = mx_wgrad_check(a, b, ws, sa, sb, M, N, K, lda, ldb, ldsa, ldsb, fa, fb, splits);
  const MxWgradArgs p{static_cast<const uint8_t*>(a), static_cast<const uint8_t*>(b), ws,
                      static_cast<const uint8_t*>(sa), static_cast<const uint8_t*>(sb), lda, ldb, ldsa, ldsb,
                      static_cast<int>(M), static_cast<int>(N), static_cast<int>(K), static_cast<int>(g.n_tiles),
                      static_cast<int>(g.tiles), g.k_tiles, g.splits};
  const unsigned grid = static_cast<unsigned>(g.grid);
  if (fa == kFp8E4M3) launch<kFp8E4M3>(p, grid, stream);
  else launch<kFp8E5M2>(p, grid, stream);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace fluxmpi
