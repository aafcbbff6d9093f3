// Host side of the fp8 entries (fp8_quant.hip, gemm_fp8.hip) without the launches: the argument checks
// and the launch geometry, plain C++ so that a stand-alone program can walk them under a sanitizer
// (scripts/fp8_host_check.cpp).
//
// Formats: 0 = e4m3 (OCP e4m3fn: no inf, FMAX 448), 1 = e5m2 (FMAX 57344). A scale block is 8 words on
// the device: {scale (fp32), 1 / scale (fp32), amax (the fp32 bits of max |x|, an integer max), the amax
// the last fp8_scale_update consumed, 4 spare}.
//   quantise: a workgroup owns a kFp8QTile x kFp8QTile tile of x; the grid is col_tiles x row_tiles with the
//             column tiles of one row tile adjacent. The transposed image has R' = R rounded up to 16 rows
//             per column, rows R .. R' zero.
//   GEMM:     a workgroup owns kFp8Tile x kFp8Tile of C and walks K in tiles of kFp8TileK bytes; the grid is
//             n_tiles x m_tiles with the column tiles of one row tile adjacent (they share the A rows in L2).
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

namespace fluxmpi {

constexpr int kFp8E4M3 = 0, kFp8E5M2 = 1;
constexpr int kFp8E2M1 = 2;  // fp4 (two values per byte): the MX entries only (mx_host.h); fp8_format_check rejects it
constexpr int kFp8BlockWords = 8;
constexpr int kFp8Threads = 256;
constexpr int kFp8QTile = 64;    // quantise tile: rows and columns
constexpr int kFp8Tile = 128;    // GEMM tile: rows and columns of C
constexpr int kFp8TileK = 128;   // GEMM: K bytes per step (one LDS row)
constexpr int64_t kFp8MaxDim = (1LL << 31) - 256;

struct Fp8QuantGeometry {
  int64_t col_tiles, row_tiles, grid;
  int64_t rpad;  // R rounded up to 16: the transposed image's row length
};

struct Fp8GemmGeometry {
  int64_t m_tiles, n_tiles, grid;
  int k_tiles;
};

[[noreturn]] inline void fp8_fail(const char* entry, const std::string& m) {
  throw std::runtime_error(std::string(entry) + ": " + m);
}

inline bool fp8_aligned16(const void* p) { return reinterpret_cast<uintptr_t>(p) % 16 == 0; }

inline void fp8_block_check(const char* entry, const void* block) {
  if (block == nullptr) fp8_fail(entry, "null scale block");
  if (reinterpret_cast<uintptr_t>(block) % 4 != 0) fp8_fail(entry, "the scale block must be 4-byte aligned");
}

inline void fp8_format_check(const char* entry, int fmt) {
  if (fmt != kFp8E4M3 && fmt != kFp8E5M2) fp8_fail(entry, "the format is 0 (e4m3) or 1 (e5m2)");
}

// x bf16 [R][C] with row stride ld (elements), C % 8 == 0; q fp8 [R][C'] with row stride ldq (C' = C rounded up
// to 16, columns C .. C' written as zero), qt fp8 [C][R'] with row stride ldt (bytes); q and qt may each be
// null (both null: the amax pass alone)
inline Fp8QuantGeometry fp8_quant_check(const void* x, int64_t R, int64_t C, int64_t ld, const void* block, int fmt,
                                        const void* q, int64_t ldq, const void* qt, int64_t ldt, bool want_amax) {
  const char* e = "fp8_quantize";
  fp8_format_check(e, fmt);
  fp8_block_check(e, block);
  if (R < 1 || R > kFp8MaxDim) fp8_fail(e, "R must lie in 1 .. 2^31 - 256");
  if (C < 8 || C % 8 != 0 || C > kFp8MaxDim) fp8_fail(e, "C must be a positive multiple of 8 below 2^31 - 256");
  if (ld < C || ld % 8 != 0) fp8_fail(e, "the input's row stride must be >= C and a multiple of 8 elements");
  if (x == nullptr) fp8_fail(e, "null input");
  if (!fp8_aligned16(x)) fp8_fail(e, "the input must be 16-byte aligned");
  Fp8QuantGeometry g{};
  g.rpad = (R + 15) / 16 * 16;
  if (q != nullptr) {
    if (!fp8_aligned16(q)) fp8_fail(e, "the output must be 16-byte aligned");
    if (ldq < (C + 15) / 16 * 16 || ldq % 16 != 0)
      fp8_fail(e, "the output's row stride must be >= C rounded up to 16 and a multiple of 16");
  }
  if (qt != nullptr) {
    if (!fp8_aligned16(qt)) fp8_fail(e, "the transposed output must be 16-byte aligned");
    if (ldt < g.rpad || ldt % 16 != 0)
      fp8_fail(e, "the transposed output's row stride must be >= R rounded up to 16 and a multiple of 16");
  }
  if (q == nullptr && qt == nullptr && !want_amax) fp8_fail(e, "nothing to do: no output and no amax");
  g.col_tiles = (C + kFp8QTile - 1) / kFp8QTile;
  g.row_tiles = (R + kFp8QTile - 1) / kFp8QTile;
  g.grid = g.col_tiles * g.row_tiles;
  if (g.grid > 0x7fffffffLL) fp8_fail(e, "too many workgroups for one launch");
  return g;
}

// C bf16 [M][N] (row stride ldc elements) = A fp8 [M][K] (lda bytes) x B fp8 [N][K] (ldb bytes); bias [N]
// bf16 (9) or fp32 (7) or null
inline Fp8GemmGeometry fp8_gemm_check(const void* a, const void* b, const void* c, const void* bias, int bias_dtype,
                                      const void* sa, const void* sb, int64_t M, int64_t N, int64_t K, int64_t lda,
                                      int64_t ldb, int64_t ldc, int fa, int fb) {
  const char* e = "fp8_gemm";
  fp8_format_check(e, fa);
  fp8_format_check(e, fb);
  if (fb != kFp8E4M3) fp8_fail(e, "the B operand is e4m3 (e4m3 x e4m3 and e5m2 x e4m3 are built)");
  fp8_block_check(e, sa);
  fp8_block_check(e, sb);
  if (M < 1 || M > kFp8MaxDim) fp8_fail(e, "M must lie in 1 .. 2^31 - 256");
  if (N < 8 || N % 8 != 0 || N > kFp8MaxDim) fp8_fail(e, "N must be a positive multiple of 8 below 2^31 - 256");
  if (K < 16 || K % 16 != 0 || K > kFp8MaxDim) fp8_fail(e, "K must be a positive multiple of 16 below 2^31 - 256");
  if (lda < K || lda % 16 != 0 || ldb < K || ldb % 16 != 0)
    fp8_fail(e, "the operands' row strides must be >= K and multiples of 16 bytes");
  if (ldc < N || ldc % 8 != 0) fp8_fail(e, "the output's row stride must be >= N and a multiple of 8 elements");
  if (a == nullptr || b == nullptr || c == nullptr) fp8_fail(e, "null tensor");
  if (!fp8_aligned16(a) || !fp8_aligned16(b) || !fp8_aligned16(c) || !fp8_aligned16(bias))
    fp8_fail(e, "every tensor must be 16-byte aligned");
  if (bias != nullptr && bias_dtype != 9 && bias_dtype != 7) fp8_fail(e, "the bias is bf16 or fp32");
  Fp8GemmGeometry g{};
  g.m_tiles = (M + kFp8Tile - 1) / kFp8Tile;
  g.n_tiles = (N + kFp8Tile - 1) / kFp8Tile;
  g.grid = g.m_tiles * g.n_tiles;
  if (g.grid > 0x7fffffffLL) fp8_fail(e, "too many workgroups for one launch");
  g.k_tiles = static_cast<int>((K + kFp8TileK - 1) / kFp8TileK);
  return g;
}

}  // namespace fluxmpi
