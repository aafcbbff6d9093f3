// Host side of the MX (block-scaled fp8) entries (mx_quant.hip, mx_gemm.hip, mx_wgrad.hip) without the launches: the
// argument checks and the launch geometry, plain C++ as fp8_host.h (scripts/mx_host_check.cpp walks them
// under a sanitizer).
//
// The format: a block is kMxBlock = 32 consecutive elements along the reduction axis of the GEMM that reads
// the image. Its elements are fp8 (fp8_host.h's formats) of x * s with s = 2^floor(log2(FMAX / block amax)),
// exponent kept in -126 .. 126, 1 for an amax of 0, inf or NaN; what is stored per block is the E8M0 byte of
// 1 / s, b = 127 - log2(s) in 1 .. 253. A scale image has one row per image row: the row's block bytes in
// order, then 127 (= 2^0) up to 4 ceil(blocks / 4), so that one aligned dword holds the four blocks of one
// 128-byte K tile (mx_scale_row).
//   quantise: a workgroup owns a kMxQTile x kMxQTile tile of x, i.e. whole scale dwords of both images; the
//             grid is col_tiles x row_tiles with the column tiles of one row tile adjacent.
//   GEMM:     fp8_host.h's geometry (128 x 128 of C per workgroup, K in tiles of 128 bytes).
//   fp4:      format 2 (e2m1: +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}, no inf / NaN) is packed two values per byte, element
//             2 i in the low nibble of byte i, so an image row of k values is k / 2 bytes and its strides are in
//             bytes. The scale images are the same (a byte per 32 VALUES). Its scale is 2^floor(log2(FMAX /
//             amax)) too, with the format's top significand 1.5; a block with an inf or NaN is all zero with the
//             byte 255. mx_quantize and mx_gemm take it (mx4_quant.hip, mx4_gemm.hip: K in tiles of 256 values),
//             mx_wgrad does not.
//   fp6:      formats 3 (e2m3: bias 1, subnormal step 0.125, max 7.5 = 1.875 * 2^2) and 4 (e3m2: bias 3, subnormal
//             step 0.0625, max 28 = 1.75 * 2^4), OCP FP6 without inf / NaN, are packed four values in three bytes:
//             value i of a 32-value block sits at bits 6 i .. 6 i + 5 of the block's 24 bytes read as one
//             little-endian bit string, so a row of k values is 3 k / 4 bytes (a multiple of 24, not always of 16:
//             the strides are still multiples of 16 bytes and the callers pad). Scale rule, scale images and the
//             byte 255 of a non-finite block as fp4. mx_quantize and mx_gemm take them (mx6_quant.hip,
//             mx6_gemm.hip: e2m3 x e2m3 and e3m2 x e2m3, K in tiles of 128 values = 96 bytes), mx_wgrad does not.
//   wgrad:    256 x 256 of the output per workgroup, the K tiles split over workgroups (below).
#pragma once
#include "fp8_host.h"

namespace fluxmpi {

constexpr int kMxBlock = 32;
constexpr int kMxQTile = 128;       // quantise tile: rows and columns (4 blocks = one scale dword each way)
constexpr unsigned kMxOne = 127;    // the E8M0 byte of 2^0: padding, empty and non-finite blocks

struct MxQuantGeometry {
  int64_t col_tiles, row_tiles, grid;
};

// bytes of a scale row for a reduction length k: one dword per 128-byte K tile
inline int64_t mx_scale_row(int64_t k) { return 4 * ((k + 127) / 128); }

constexpr int kMxE2M3 = 3, kMxE3M2 = 4;  // fp6, four values in three bytes
inline bool mx_is_fp6(int fmt) { return fmt == kMxE2M3 || fmt == kMxE3M2; }

// the MX entries that have fp4 and fp6 kernels take formats 2 .. 4 as well
inline void mx_format_check(const char* entry, int fmt) {
  if (fmt != kFp8E4M3 && fmt != kFp8E5M2 && fmt != kFp8E2M1 && !mx_is_fp6(fmt))
    fp8_fail(entry, "the format is 0 (e4m3), 1 (e5m2), 2 (e2m1, packed fp4), 3 (e2m3) or 4 (e3m2, packed fp6)");
}

// bytes of k values of a format (k % 32 == 0)
inline int64_t mx_row_bytes(int64_t k, int fmt) { return fmt == kFp8E2M1 ? k / 2 : (mx_is_fp6(fmt) ? k / 4 * 3 : k); }

constexpr int kMx6TileK = 128;                   // mx6_gemm.hip: K VALUES per step
constexpr int kMx6RowBytes = kMx6TileK / 4 * 3;  // ... which are 96 bytes of a row: six 16-byte chunks

constexpr int kMx4TileK = 256;  // mx4_gemm.hip: K VALUES per step (a 128-byte LDS row of fp4)

inline void mx_scale_check(const char* e, const void* s, int64_t lds, int64_t k, const char* what) {
  if (s == nullptr) fp8_fail(e, std::string("null ") + what);
  if (reinterpret_cast<uintptr_t>(s) % 4 != 0) fp8_fail(e, std::string(what) + " must be 4-byte aligned");
  if (lds < mx_scale_row(k) || lds % 4 != 0)
    fp8_fail(e, std::string(what) + ": the row stride must be >= 4 ceil(K / 128) and a multiple of 4");
}

// x bf16 [R][C] (row stride ld elements), C % 32 == 0. Row-wise image: q [R][ldq] with s [R][lds], both or
// neither. Transposed image (blocks along R, so R % 32 == 0): qt [C][ldt] with st [C][ldst], both or neither.
// ldq / ldt are bytes: >= C / R for fp8, >= C / 2 and R / 2 for fp4, >= 3 C / 4 and 3 R / 4 for fp6.
inline MxQuantGeometry mx_quant_check(const void* x, int64_t R, int64_t C, int64_t ld, int fmt, const void* q,
                                      int64_t ldq, const void* s, int64_t lds, const void* qt, int64_t ldt,
                                      const void* st, int64_t ldst) {
  const char* e = "mx_quantize";
  mx_format_check(e, fmt);
  if (R < 1 || R > kFp8MaxDim) fp8_fail(e, "R must lie in 1 .. 2^31 - 256");
  if (C < kMxBlock || C % kMxBlock != 0 || C > kFp8MaxDim)
    fp8_fail(e, "C must be a positive multiple of 32 below 2^31 - 256");
  if (ld < C || ld % 8 != 0) fp8_fail(e, "the input's row stride must be >= C and a multiple of 8 elements");
  if (x == nullptr) fp8_fail(e, "null input");
  if (!fp8_aligned16(x)) fp8_fail(e, "the input must be 16-byte aligned");
  if ((q == nullptr) != (s == nullptr)) fp8_fail(e, "the row-wise image and its scales come together");
  if ((qt == nullptr) != (st == nullptr)) fp8_fail(e, "the transposed image and its scales come together");
  if (q == nullptr && qt == nullptr) fp8_fail(e, "nothing to do: no output");
  if (q != nullptr) {
    if (!fp8_aligned16(q)) fp8_fail(e, "the output must be 16-byte aligned");
    if (ldq < mx_row_bytes(C, fmt) || ldq % 16 != 0)
      fp8_fail(e, "the output's row stride must be >= C (fp4: C / 2, fp6: 3 C / 4) bytes and a multiple of 16");
    mx_scale_check(e, s, lds, C, "the scale image");
  }
  if (qt != nullptr) {
    if (R % kMxBlock != 0) fp8_fail(e, "the transposed image needs R % 32 == 0 (its blocks run along R)");
    if (!fp8_aligned16(qt)) fp8_fail(e, "the transposed output must be 16-byte aligned");
    if (ldt < mx_row_bytes(R, fmt) || ldt % 16 != 0)
      fp8_fail(e, "the transposed output's row stride must be >= R (fp4: R / 2, fp6: 3 R / 4) bytes and a multiple of 16");
    mx_scale_check(e, st, ldst, R, "the transposed scale image");
  }
  MxQuantGeometry g{};
  g.col_tiles = (C + kMxQTile - 1) / kMxQTile;
  g.row_tiles = (R + kMxQTile - 1) / kMxQTile;
  g.grid = g.col_tiles * g.row_tiles;
  if (g.grid > 0x7fffffffLL) fp8_fail(e, "too many workgroups for one launch");
  return g;
}

// C bf16 [M][ldc] = A fp8 [M][K] (lda bytes, scales sa [M][ldsa]) x B fp8 [N][K] (ldb, sb [N][ldsb]); bias [N]
// bf16 (9) or fp32 (7) or null. K counts values: an fp4 operand's row is K / 2 bytes, an fp6 one's 3 K / 4
inline Fp8GemmGeometry mx_gemm_check(const void* a, const void* b, const void* c, const void* bias, int bias_dtype,
                                     const void* sa, const void* sb, int64_t M, int64_t N, int64_t K, int64_t lda,
                                     int64_t ldb, int64_t ldc, int64_t ldsa, int64_t ldsb, int fa, int fb) {
  const char* e = "mx_gemm";
  mx_format_check(e, fa);
  mx_format_check(e, fb);
  if (mx_is_fp6(fa) || mx_is_fp6(fb)) {
    if (fb != kMxE2M3 || !mx_is_fp6(fa))
      fp8_fail(e, "an fp6 operand: A x B is e2m3 x e2m3 or e3m2 x e2m3 (no other pair with an fp6 side is built)");
  } else if (!(fb == kFp8E4M3 && fa != kFp8E2M1) && !(fb == kFp8E2M1 && fa != kFp8E5M2)) {
    fp8_fail(e, "A x B is e4m3 x e4m3, e5m2 x e4m3, e2m1 x e2m1 or e4m3 x e2m1 (no other pair is built)");
  }
  if (M < 1 || M > kFp8MaxDim) fp8_fail(e, "M must lie in 1 .. 2^31 - 256");
  if (N < 8 || N % 8 != 0 || N > kFp8MaxDim) fp8_fail(e, "N must be a positive multiple of 8 below 2^31 - 256");
  if (K < kMxBlock || K % kMxBlock != 0 || K > kFp8MaxDim)
    fp8_fail(e, "K must be a positive multiple of 32 below 2^31 - 256");
  if (lda < mx_row_bytes(K, fa) || lda % 16 != 0 || ldb < mx_row_bytes(K, fb) || ldb % 16 != 0)
    fp8_fail(e, "the operands' row strides must be >= K (fp4: K / 2, fp6: 3 K / 4) bytes and multiples of 16");
  if (ldc < N || ldc % 8 != 0) fp8_fail(e, "the output's row stride must be >= N and a multiple of 8 elements");
  if (a == nullptr || b == nullptr || c == nullptr) fp8_fail(e, "null tensor");
  if (!fp8_aligned16(a) || !fp8_aligned16(b) || !fp8_aligned16(c) || !fp8_aligned16(bias))
    fp8_fail(e, "every tensor must be 16-byte aligned");
  if (bias != nullptr && bias_dtype != 9 && bias_dtype != 7) fp8_fail(e, "the bias is bf16 or fp32");
  mx_scale_check(e, sa, ldsa, K, "A's scale image");
  mx_scale_check(e, sb, ldsb, K, "B's scale image");
  Fp8GemmGeometry g{};
  g.m_tiles = (M + kFp8Tile - 1) / kFp8Tile;
  g.n_tiles = (N + kFp8Tile - 1) / kFp8Tile;
  g.grid = g.m_tiles * g.n_tiles;
  if (g.grid > 0x7fffffffLL) fp8_fail(e, "too many workgroups for one launch");
  const int tile_k = fb == kFp8E2M1 ? kMx4TileK : kFp8TileK;
  g.k_tiles = static_cast<int>((K + tile_k - 1) / tile_k);
  return g;
}

// ---- the weight gradient (mx_wgrad.hip): ws fp32 [splits][M][N], split s = the K tiles of its range ----
constexpr int kMxWgTile = 256;     // rows and columns of the output per workgroup
constexpr int kMxWgThreads = 512;  // 8 waves: 2 (M) x 4 (N), 128 x 64 each
constexpr int kMxWgPerCu = 1;      // workgroups resident per CU (132 KiB of LDS each)

struct MxWgradGeometry {
  int64_t m_tiles, n_tiles, tiles, grid;
  int k_tiles, splits;
};

// K tiles of split s out of `splits` over `k_tiles`: contiguous, sizes differing by at most one, none empty
// (splits <= k_tiles): the first k_tiles % splits ranges hold one tile more. constexpr: the kernel calls it too
constexpr int mx_wgrad_first_tile(int k_tiles, int splits, int s) {
  const int base = k_tiles / splits, rem = k_tiles % splits;
  return s * base + (s < rem ? s : rem);
}

// the split count a launch uses for `wanted`: 1 .. the number of 128-byte K tiles (wanted < 1 counts as 1)
inline int mx_wgrad_splits(int64_t K, int64_t wanted) {
  const char* e = "mx_wgrad_splits";
  if (K < kMxBlock || K % kMxBlock != 0 || K > kFp8MaxDim)
    fp8_fail(e, "K must be a positive multiple of 32 below 2^31 - 256");
  const int64_t k_tiles = (K + kFp8TileK - 1) / kFp8TileK;
  return static_cast<int>(wanted < 1 ? 1 : (wanted < k_tiles ? wanted : k_tiles));
}

// ws fp32 [splits][M][N] (dense) from A fp8 [M][K] (lda bytes, scales sa [M][ldsa]) and B fp8 [N][K] (ldb,
// sb [N][ldsb]); `splits` must be mx_wgrad_splits(K, .) of itself: the caller sized ws from it
inline MxWgradGeometry mx_wgrad_check(const void* a, const void* b, const void* ws, const void* sa, const void* sb,
                                      int64_t M, int64_t N, int64_t K, int64_t lda, int64_t ldb, int64_t ldsa,
                                      int64_t ldsb, int fa, int fb, int64_t splits) {
  const char* e = "mx_wgrad";
  fp8_format_check(e, fa);
  fp8_format_check(e, fb);
  if (fb != kFp8E4M3) fp8_fail(e, "the B operand is e4m3 (e4m3 x e4m3 and e5m2 x e4m3 are built)");
  if (M < 1 || M > kFp8MaxDim) fp8_fail(e, "M must lie in 1 .. 2^31 - 256");
  if (N < 8 || N % 8 != 0 || N > kFp8MaxDim) fp8_fail(e, "N must be a positive multiple of 8 below 2^31 - 256");
  if (K < kMxBlock || K % kMxBlock != 0 || K > kFp8MaxDim)
    fp8_fail(e, "K must be a positive multiple of 32 below 2^31 - 256");
  if (lda < K || lda % 16 != 0 || ldb < K || ldb % 16 != 0)
    fp8_fail(e, "the operands' row strides must be >= K and multiples of 16 bytes");
  if (a == nullptr || b == nullptr || ws == nullptr) fp8_fail(e, "null tensor");
  if (!fp8_aligned16(a) || !fp8_aligned16(b) || !fp8_aligned16(ws))
    fp8_fail(e, "every tensor must be 16-byte aligned");
  mx_scale_check(e, sa, ldsa, K, "A's scale image");
  mx_scale_check(e, sb, ldsb, K, "B's scale image");
  if (splits < 1 || splits != mx_wgrad_splits(K, splits))
    fp8_fail(e, "the split count must be mx_wgrad_splits(K, wanted): 1 .. the number of 128-byte K tiles");
  MxWgradGeometry g{};
  g.m_tiles = (M + kMxWgTile - 1) / kMxWgTile;
  g.n_tiles = (N + kMxWgTile - 1) / kMxWgTile;
  g.tiles = g.m_tiles * g.n_tiles;
  g.grid = g.tiles * splits;
  if (g.tiles > 0x7fffffffLL || g.grid > 0x7fffffffLL) fp8_fail(e, "too many workgroups for one launch");
  g.k_tiles = static_cast<int>((K + kFp8TileK - 1) / kFp8TileK);
  g.splits = static_cast<int>(splits);
  return g;
}

}  // namespace fluxmpi
