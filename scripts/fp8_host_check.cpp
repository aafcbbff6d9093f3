// Stand-alone walk of the fp8 entries' host code (csrc/kernels/fp8_host.h: the argument checks and the launch
// geometry) for a sanitizer run on the CPU; no GPU, no Python:
//
//   amdclang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I csrc scripts/fp8_host_check.cpp -o build/fp8_host_check && build/fp8_host_check
//
// It walks the shapes of tests/test_fp8_gpu.py, the ViT-B/16 shapes at 50432 tokens, R = 1 and M = 1, the largest
// sizes that fit and the first that do not, and every rejected argument, and verifies the geometry: the quantise
// grid covers every 64 x 64 tile once, the transposed image's padded row length is R rounded up to 16, every
// 16-byte access a lane makes (input, both outputs; A, B, C and the bias of the GEMM) lies inside its row, and
// the GEMM's loader permutation of B rows is a permutation of the tile that the epilogue's column formula
// inverts. Exit status 0 and "ok" when all hold.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels/fp8_host.h"

using namespace fluxmpi;

static int failures = 0;
#define EXPECT(cond)                                                         \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                            \
    }                                                                        \
  } while (0)

alignas(16) static unsigned char mem[64];
static const void* const X = mem;
static void* const Q = mem + 16;
static void* const QT = mem + 32;
static void* const BLK = mem + 48;

static void walk_quant(int64_t R, int64_t C, int64_t ld) {
  const int64_t rp = (R + 15) / 16 * 16;
  for (int fmt : {kFp8E4M3, kFp8E5M2}) {
    const int64_t cp = (C + 15) / 16 * 16;
    const Fp8QuantGeometry g = fp8_quant_check(X, R, C, ld, BLK, fmt, Q, cp, QT, rp, true);
    EXPECT(g.rpad == rp && g.rpad >= R && g.rpad - R < 16);
    EXPECT(g.col_tiles * kFp8QTile >= C && (g.col_tiles - 1) * kFp8QTile < C);
    EXPECT(g.row_tiles * kFp8QTile >= R && (g.row_tiles - 1) * kFp8QTile < R);
    EXPECT(g.grid == g.col_tiles * g.row_tiles && g.grid <= 0x7fffffffLL);
    // the last tile's lanes: each half of a lane's 16 columns, and its 16 transposed rows, are inside or outside
    // as a whole
    const int64_t r0 = (g.row_tiles - 1) * kFp8QTile, c0 = (g.col_tiles - 1) * kFp8QTile;
    for (int t = 0; t < kFp8Threads; ++t) {
      const int64_t r = r0 + (t >> 2), c = c0 + (t & 3) * 16;
      if (r < R && c < C) EXPECT(c + 8 <= C && c + 8 <= ld && c + 16 <= cp);  // the half loaded, the 16 B stored
      if (r < R && c + 8 < C) EXPECT(c + 16 <= C && c + 16 <= ld);
      const int64_t tc = c0 + (t >> 2), tr = r0 + (t & 3) * 16;
      if (tc < C && tr < g.rpad) EXPECT(tr + 16 <= g.rpad);
    }
  }
  fp8_quant_check(X, R, C, ld, BLK, kFp8E4M3, nullptr, 0, nullptr, 0, true);  // the amax pass alone
}

static void walk_gemm(int64_t M, int64_t N, int64_t K) {
  for (int fa : {kFp8E4M3, kFp8E5M2})
    for (int bt : {0, 7, 9}) {
      const Fp8GemmGeometry g =
          fp8_gemm_check(X, Q, QT, bt != 0 ? X : nullptr, bt, BLK, BLK, M, N, K, K, (K + 15) / 16 * 16, N + 8, fa, kFp8E4M3);
      EXPECT(g.m_tiles * kFp8Tile >= M && (g.m_tiles - 1) * kFp8Tile < M);
      EXPECT(g.n_tiles * kFp8Tile >= N && (g.n_tiles - 1) * kFp8Tile < N);
      EXPECT(static_cast<int64_t>(g.k_tiles) * kFp8TileK >= K && static_cast<int64_t>(g.k_tiles - 1) * kFp8TileK < K);
      EXPECT(g.grid == g.m_tiles * g.n_tiles);
      // the last K tile: a lane's 16-byte chunk is inside K or outside as a whole
      for (int kc = 0; kc < 8; ++kc) {
        const int64_t k = static_cast<int64_t>(g.k_tiles - 1) * kFp8TileK + kc * 16;
        if (k < K) EXPECT(k + 16 <= K);
      }
      // the last column tile: a lane's 8 columns (the store, the bias load)
      for (int n8 = 0; n8 < kFp8Tile; n8 += 8) {
        const int64_t n = (g.n_tiles - 1) * kFp8Tile + n8;
        if (n < N) EXPECT(n + 8 <= N);
      }
    }
}

// the loader's order of B rows (gemm_fp8.hip): LDS row rho holds tile row src(rho); first-operand row 4 g + r of
// MFMA tile j of wave column wn must be column 64 wn + 32 (j >> 1) + 8 g + 4 (j & 1) + r of the epilogue
static void walk_permutation() {
  std::vector<int> seen(kFp8Tile, 0);
  for (int rho = 0; rho < kFp8Tile; ++rho) {
    const int src = (rho & 64) + 32 * ((rho >> 5) & 1) + 8 * ((rho >> 2) & 3) + 4 * ((rho >> 4) & 1) + (rho & 3);
    EXPECT(src >= 0 && src < kFp8Tile);
    if (src >= 0 && src < kFp8Tile) ++seen[src];
    const int wn = rho >> 6, j = (rho >> 4) & 3, row = rho & 15, g = row >> 2, r = row & 3;
    EXPECT(src == 64 * wn + 32 * (j >> 1) + 8 * g + 4 * (j & 1) + r);
  }
  for (int v : seen) EXPECT(v == 1);
}

template <typename F> static void rejects(const char* what, F&& f) {
  try {
    f();
  } catch (const std::runtime_error& e) {
    if (std::string(e.what()).rfind("fp8_", 0) != 0) {
      std::fprintf(stderr, "the error does not name its entry: %s\n", e.what());
      ++failures;
    }
    return;
  }
  std::fprintf(stderr, "not rejected: %s\n", what);
  ++failures;
}

int main() {
  int shapes = 0;
  for (auto [r, c, ld] : std::vector<std::array<int64_t, 3>>{{1, 16, 16}, {17, 48, 48}, {130, 144, 144}, {300, 400, 400},
                                                           {130, 144, 152}, {130, 136, 136}, {9, 8, 8}, {50432, 768, 768}, {2304, 768, 768},
                                                           {50432, 2304, 2304}, {kFp8MaxDim, 16, 16}, {16, kFp8MaxDim - 240, kFp8MaxDim - 240}})
    walk_quant(r, c, ld), ++shapes;
  for (int64_t m : {1, 127, 129, 300})
    for (int64_t n : {8, 136})
      for (int64_t k : {16, 128, 144, 400}) walk_gemm(m, n, k), ++shapes;
  for (auto [m, n, k] : std::vector<std::array<int64_t, 3>>{{256, 256, 256}, {50432, 2304, 768}, {50432, 768, 2304},
                                                          {50432, 3072, 768}, {50432, 768, 3072}, {kFp8MaxDim, 8, 16},
                                                          {1, kFp8MaxDim - 248, 16}, {1, 8, kFp8MaxDim - 240}})
    walk_gemm(m, n, k), ++shapes;
  walk_permutation();

  const auto quant = [&](int64_t R, int64_t C, int64_t ld, const void* x = X, void* blk = BLK, int fmt = 0, void* q = Q,
                         int64_t ldq = -1, void* qt = QT, int64_t ldt = -1, bool amax = true) {
    fp8_quant_check(x, R, C, ld, blk, fmt, q, ldq < 0 ? (C + 15) / 16 * 16 : ldq, qt, ldt < 0 ? (R + 15) / 16 * 16 : ldt, amax);
  };
  quant(17, 48, 48);
  rejects("R = 0", [&] { quant(0, 48, 48); });
  rejects("R too large", [&] { quant(kFp8MaxDim + 1, 16, 16); });
  rejects("C = 0", [&] { quant(17, 0, 48); });
  quant(17, 40, 40);
  rejects("C % 8", [&] { quant(17, 44, 48); });
  rejects("ldq below C rounded up to 16", [&] { quant(17, 40, 40, X, BLK, 0, Q, 32); });
  rejects("C too large", [&] { quant(1, kFp8MaxDim + 240, kFp8MaxDim + 240); });
  rejects("ld < C", [&] { quant(17, 48, 40); });
  rejects("ld % 8", [&] { quant(17, 48, 52); });
  rejects("null input", [&] { quant(17, 48, 48, nullptr); });
  rejects("unaligned input", [&] { quant(17, 48, 48, mem + 2); });
  rejects("null block", [&] { quant(17, 48, 48, X, nullptr); });
  rejects("unaligned block", [&] { quant(17, 48, 48, X, mem + 2); });
  rejects("format 2", [&] { quant(17, 48, 48, X, BLK, 2); });
  rejects("unaligned q", [&] { quant(17, 48, 48, X, BLK, 0, mem + 8); });
  rejects("ldq < C", [&] { quant(17, 48, 48, X, BLK, 0, Q, 32); });
  rejects("ldq % 16", [&] { quant(17, 48, 48, X, BLK, 0, Q, 56); });
  rejects("unaligned qt", [&] { quant(17, 48, 48, X, BLK, 0, Q, 48, mem + 8); });
  rejects("ldt < R'", [&] { quant(17, 48, 48, X, BLK, 0, Q, 48, QT, 16); });
  rejects("ldt % 16", [&] { quant(17, 48, 48, X, BLK, 0, Q, 48, QT, 40); });
  rejects("nothing to do", [&] { quant(17, 48, 48, X, BLK, 0, nullptr, 0, nullptr, 0, false); });
  rejects("too many workgroups", [&] { quant(kFp8MaxDim, kFp8MaxDim - 240, kFp8MaxDim - 240); });
  rejects("update: format", [&] { fp8_format_check("fp8_scale_update", -1); });
  rejects("update: block", [&] { fp8_block_check("fp8_scale_update", nullptr); });

  const auto gemm = [&](int64_t M, int64_t N, int64_t K, int64_t lda = -1, int64_t ldb = -1, int64_t ldc = -1,
                        const void* a = X, const void* b = Q, const void* c = QT, const void* bias = nullptr, int bt = 0,
                        const void* sa = BLK, const void* sb = BLK, int fa = 0, int fb = 0) {
    fp8_gemm_check(a, b, c, bias, bt, sa, sb, M, N, K, lda < 0 ? K : lda, ldb < 0 ? K : ldb, ldc < 0 ? N : ldc, fa, fb);
  };
  gemm(130, 136, 144);
  rejects("M = 0", [&] { gemm(0, 136, 144); });
  rejects("M too large", [&] { gemm(kFp8MaxDim + 1, 8, 16); });
  rejects("N = 0", [&] { gemm(130, 0, 144); });
  rejects("N % 8", [&] { gemm(130, 132, 144); });
  rejects("N too large", [&] { gemm(1, kFp8MaxDim + 8, 16); });
  rejects("K = 0", [&] { gemm(130, 136, 0); });
  rejects("K % 16", [&] { gemm(130, 136, 136); });
  rejects("K too large", [&] { gemm(1, 8, kFp8MaxDim + 240); });
  rejects("lda < K", [&] { gemm(130, 136, 144, 128); });
  rejects("lda % 16", [&] { gemm(130, 136, 144, 152); });
  rejects("ldb < K", [&] { gemm(130, 136, 144, 144, 128); });
  rejects("ldb % 16", [&] { gemm(130, 136, 144, 144, 152); });
  rejects("ldc < N", [&] { gemm(130, 136, 144, 144, 144, 128); });
  rejects("ldc % 8", [&] { gemm(130, 136, 144, 144, 144, 140); });
  rejects("null a", [&] { gemm(130, 136, 144, -1, -1, -1, nullptr); });
  rejects("null b", [&] { gemm(130, 136, 144, -1, -1, -1, X, nullptr); });
  rejects("null c", [&] { gemm(130, 136, 144, -1, -1, -1, X, Q, nullptr); });
  rejects("unaligned a", [&] { gemm(130, 136, 144, -1, -1, -1, mem + 4); });
  rejects("unaligned bias", [&] { gemm(130, 136, 144, -1, -1, -1, X, Q, QT, mem + 4, 9); });
  rejects("fp16 bias", [&] { gemm(130, 136, 144, -1, -1, -1, X, Q, QT, X, 6); });
  rejects("null scale block", [&] { gemm(130, 136, 144, -1, -1, -1, X, Q, QT, nullptr, 0, nullptr); });
  rejects("unaligned scale block", [&] { gemm(130, 136, 144, -1, -1, -1, X, Q, QT, nullptr, 0, BLK, mem + 1); });
  rejects("format of a", [&] { gemm(130, 136, 144, -1, -1, -1, X, Q, QT, nullptr, 0, BLK, BLK, 2); });
  rejects("e5m2 b", [&] { gemm(130, 136, 144, -1, -1, -1, X, Q, QT, nullptr, 0, BLK, BLK, 0, 1); });
  rejects("too many workgroups", [&] { gemm(kFp8MaxDim, kFp8MaxDim - 248, 16); });

  if (failures != 0) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("fp8_host_check: ok (%d shapes)\n", shapes);
  return 0;
}
