// Stand-alone walk of the MX entries' host code (csrc/kernels/mx_host.h: the argument checks and the launch
// geometry) for a sanitizer run on the CPU; no GPU, no Python:
//
//   amdclang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I csrc scripts/mx_host_check.cpp -o build/mx_host_check && build/mx_host_check
//
// It walks the shapes of tests/test_mx_gpu.py, the ViT-B/16 shapes at 50432 tokens, R = 1 and M = 1, the largest
// sizes that fit and the first that do not, and every rejected argument, and verifies the geometry: the quantise
// grid covers every 128 x 128 tile once, every 16-byte access of a lane (input, both images) and every scale dword
// (both scale images; the GEMM's loader) lies inside its row, no two tiles share a scale dword, and the GEMM's
// scale scatter fills each operand's area exactly once with the dword order its reader expects. For the weight
// gradient (mx_wgrad_check, mx_wgrad_splits): the shapes and split counts of tests/test_mx_wgrad_gpu.py and the
// ViT-B/16 ones, wanted counts of 0, 1 and above the tile count, the split ranges (contiguous, none empty, within one
// tile of each other) and the kernel's LDS row and scale-area maps over 256 rows. For fp6 (formats 3 and 4): row bytes
// 3 k / 4, strides padded to 16, every store of mx6_quant.hip's quads and columns and every chunk of mx6_gemm.hip's
// loader inside its row, the loader's chunk map covering the LDS tile once, and the refused pairs. Exit status 0 and
// "ok" when all hold.
#include <array>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels/mx_host.h"

using namespace fluxmpi;

static int failures = 0;
#define EXPECT(cond)                                                         \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                            \
    }                                                                        \
  } while (0)

alignas(16) static unsigned char mem[80];
static const void* const X = mem;
static void* const Q = mem + 16;
static void* const QT = mem + 32;
static void* const S = mem + 48;
static void* const ST = mem + 64;

static void walk_quant(int64_t R, int64_t C, int64_t ld) {
  const bool t = R % kMxBlock == 0;
  const int64_t lds = mx_scale_row(C), ldst = mx_scale_row(R);
  for (int fmt : {kFp8E4M3, kFp8E5M2}) {
    const MxQuantGeometry g = mx_quant_check(X, R, C, ld, fmt, Q, C, S, lds, t ? QT : nullptr, R, t ? ST : nullptr, ldst);
    EXPECT(g.col_tiles * kMxQTile >= C && (g.col_tiles - 1) * kMxQTile < C);
    EXPECT(g.row_tiles * kMxQTile >= R && (g.row_tiles - 1) * kMxQTile < R);
    EXPECT(g.grid == g.col_tiles * g.row_tiles && g.grid <= 0x7fffffffLL);
    // a tile's scale dwords: 4 ct of a row, 4 rt of a column: distinct per tile, inside the scale rows
    EXPECT(4 * (g.col_tiles - 1) + 4 <= lds && 4 * (g.row_tiles - 1) + 4 <= ldst);
    EXPECT(lds >= (C + kMxBlock - 1) / kMxBlock && ldst >= (R + kMxBlock - 1) / kMxBlock);
    // the last tile's lanes: 16 columns of a row, and two columns x 32 rows of the transposed image
    const int64_t r0 = (g.row_tiles - 1) * kMxQTile, c0 = (g.col_tiles - 1) * kMxQTile;
    for (int lane = 0; lane < kFp8Threads; ++lane) {
      for (int pass = 0; pass < 4; ++pass) {
        const int64_t r = r0 + (lane >> 3) + 32 * pass, c = c0 + (lane & 7) * 16;
        if (r < R && c < C) EXPECT(c + 16 <= C && c + 16 <= ld);
      }
      const int64_t col = c0 + 2 * (lane & 63), rb = r0 + 32 * (lane >> 6);
      if (t && col < C && rb < R) EXPECT(col + 2 <= C && rb + 32 <= R);
    }
  }
  mx_quant_check(X, R, C, ld, kFp8E4M3, Q, C, S, lds, nullptr, 0, nullptr, 0);  // the row-wise image alone
  if (t) mx_quant_check(X, R, C, ld, kFp8E4M3, nullptr, 0, nullptr, 0, QT, R, ST, ldst);
}

static void walk_gemm(int64_t M, int64_t N, int64_t K) {
  for (int fa : {kFp8E4M3, kFp8E5M2})
    for (int bt : {0, 7, 9}) {
      const int64_t lds = mx_scale_row(K);
      const Fp8GemmGeometry g = mx_gemm_check(X, Q, QT, bt != 0 ? X : nullptr, bt, S, ST, M, N, K, K, (K + 15) / 16 * 16,
                                              N + 8, lds, lds + 4, fa, kFp8E4M3);
      EXPECT(g.m_tiles * kFp8Tile >= M && (g.m_tiles - 1) * kFp8Tile < M);
      EXPECT(g.n_tiles * kFp8Tile >= N && (g.n_tiles - 1) * kFp8Tile < N);
      EXPECT(static_cast<int64_t>(g.k_tiles) * kFp8TileK >= K && static_cast<int64_t>(g.k_tiles - 1) * kFp8TileK < K);
      EXPECT(g.grid == g.m_tiles * g.n_tiles);
      EXPECT(4 * static_cast<int64_t>(g.k_tiles) <= lds);  // the last step's scale dword
      const int64_t left = K / kMxBlock - 4 * static_cast<int64_t>(g.k_tiles - 1);
      EXPECT(left >= 1 && left <= 4);  // blocks of the last K tile inside K: the rest are forced to 127
      for (int kc = 0; kc < 8; ++kc) {
        const int64_t k = static_cast<int64_t>(g.k_tiles - 1) * kFp8TileK + kc * 16;
        if (k < K) EXPECT(k + 16 <= K);
      }
      for (int n8 = 0; n8 < kFp8Tile; n8 += 8) {
        const int64_t n = (g.n_tiles - 1) * kFp8Tile + n8;
        if (n < N) EXPECT(n + 8 <= N);
      }
    }
}

// fp6: mx6_quant.hip's stores (a quad's 48 bytes of a row in chunks of 16 or a last 8; a lane's 48 bytes of a column)
// and mx6_gemm.hip's loader (chunk t + 256 u = 6 rho + ch; 16 bytes, a last 8, or nothing) stay inside rows of
// 3 k / 4 bytes, and the padded strides are what the checks ask for
static void walk_fp6(int64_t R, int64_t C) {
  const auto pad16 = [](int64_t n) { return (n + 15) / 16 * 16; };
  const bool t = R % kMxBlock == 0;
  for (int fmt : {kMxE2M3, kMxE3M2}) {
    const int64_t qb = mx_row_bytes(C, fmt), tb = mx_row_bytes(R, fmt);
    EXPECT(qb * 4 == C * 3 && qb % 24 == 0 && pad16(qb) - qb < 16 && pad16(qb) % 16 == 0);
    const MxQuantGeometry g = mx_quant_check(X, R, C, C, fmt, Q, pad16(qb), S, mx_scale_row(C), t ? QT : nullptr, pad16(tb),
                                             t ? ST : nullptr, mx_scale_row(R));
    for (int64_t ct = 0; ct < g.col_tiles; ct += (g.col_tiles > 2 ? g.col_tiles - 1 : 1))
      for (int quad = 0; quad < 2; ++quad) {
        const int64_t left = C - (ct * kMxQTile + 64 * quad), bytes = left >= 64 ? 48 : (left >= 32 ? 24 : 0);
        int64_t written = 0;
        for (int j = 0; j < 3; ++j) {
          const int64_t ofs = 96 * ct + 48 * quad + 16 * j, n = 16 * j + 16 <= bytes ? 16 : (16 * j + 8 <= bytes ? 8 : 0);
          EXPECT(ofs % 16 == 0 && (n == 0 || ofs + n <= qb));
          written += n;
        }
        EXPECT(written == bytes);
      }
    if (t)
      for (int half = 0; half < 2; ++half) {
        const int64_t rt = g.row_tiles - 1, left = R - (rt * kMxQTile + 64 * half), bytes = left >= 64 ? 48 : (left >= 32 ? 24 : 0);
        for (int k = 0; k < 3; ++k) {
          const int64_t n = 16 * k + 16 <= bytes ? 16 : (16 * k + 8 <= bytes ? 8 : 0);
          EXPECT(n == 0 || 96 * rt + 48 * half + 16 * k + n <= tb);
        }
      }
    // the GEMM with K = C: e2m3 B, this format as A
    const Fp8GemmGeometry gg = mx_gemm_check(X, Q, QT, nullptr, 0, S, ST, R, 8, C, pad16(qb), pad16(qb), 8, mx_scale_row(C),
                                             mx_scale_row(C), fmt, kMxE2M3);
    EXPECT(static_cast<int64_t>(gg.k_tiles) * kMx6TileK >= C && static_cast<int64_t>(gg.k_tiles - 1) * kMx6TileK < C);
    int64_t covered = 0;
    for (int step = 0; step < gg.k_tiles; ++step)
      for (int ch = 0; ch < kMx6RowBytes / 16; ++ch) {
        const int64_t have = qb - step * kMx6RowBytes - ch * 16, n = have >= 16 ? 16 : (have >= 8 ? 8 : 0);
        EXPECT(n == 0 || step * kMx6RowBytes + ch * 16 + n <= qb);
        covered += n;
      }
    EXPECT(covered == qb);
  }
  std::vector<int> seen(kFp8Tile * (kMx6RowBytes / 16), 0);
  for (int u = 0; u < 3; ++u)
    for (int lane = 0; lane < kFp8Threads; ++lane) {
      const int idx = lane + kFp8Threads * u, rho = idx / 6, ch = idx - 6 * rho;
      EXPECT(rho < kFp8Tile && ch < 6);
      if (rho < kFp8Tile) ++seen[rho * 6 + ch];
    }
  for (int v : seen) EXPECT(v == 1);
}

// mx_gemm.hip's scale area: the loader lane of LDS row rho writes byte (rho >> 4) & 3 of the dwords
// [rho >> 6][g][rho & 15]; the reader of wave row / column w, lane l reads dword w * 64 + l and wants in byte i
// the scale of (tile i, row l & 15, K group l >> 4)
static void walk_scale_area() {
  std::vector<int> seen(kFp8Tile * 4, 0);
  for (int rho = 0; rho < kFp8Tile; ++rho)
    for (int g = 0; g < 4; ++g) {
      const int ofs = (((rho >> 6) * 4) * 16 + (rho & 15)) * 4 + ((rho >> 4) & 3) + g * 64;
      EXPECT(ofs >= 0 && ofs < kFp8Tile * 4);
      if (ofs >= 0 && ofs < kFp8Tile * 4) ++seen[ofs];
      const int w = rho >> 6, tile = (rho >> 4) & 3, lane = 16 * g + (rho & 15);
      EXPECT(ofs == (w * 64 + lane) * 4 + tile);
    }
  for (int v : seen) EXPECT(v == 1);
}

// mx_wgrad.hip: the tiles cover M x N once, the splits partition the K tiles (contiguous, none empty, sizes within
// one of each other), every operand chunk and scale dword a workgroup reads and every 8-column store lies inside
static void walk_wgrad(int64_t M, int64_t N, int64_t K, int64_t wanted) {
  const int splits = mx_wgrad_splits(K, wanted);
  const int64_t k_tiles = (K + kFp8TileK - 1) / kFp8TileK, lds = mx_scale_row(K);
  EXPECT(splits >= 1 && splits <= k_tiles && (wanted < 1 || splits <= wanted));
  EXPECT(splits == wanted || wanted < 1 || wanted > k_tiles);
  EXPECT(mx_wgrad_splits(K, splits) == splits);
  for (int fa : {kFp8E4M3, kFp8E5M2}) {
    const MxWgradGeometry g = mx_wgrad_check(X, Q, QT, S, ST, M, N, K, K, (K + 15) / 16 * 16, lds, lds + 4, fa, kFp8E4M3, splits);
    EXPECT(g.m_tiles * kMxWgTile >= M && (g.m_tiles - 1) * kMxWgTile < M);
    EXPECT(g.n_tiles * kMxWgTile >= N && (g.n_tiles - 1) * kMxWgTile < N);
    EXPECT(g.tiles == g.m_tiles * g.n_tiles && g.grid == g.tiles * splits && g.splits == splits && g.k_tiles == k_tiles);
    EXPECT(mx_wgrad_first_tile(g.k_tiles, splits, 0) == 0 && mx_wgrad_first_tile(g.k_tiles, splits, splits) == g.k_tiles);
    int lo = g.k_tiles, hi = 0;
    for (int s = 0; s < splits; ++s) {
      const int n = mx_wgrad_first_tile(g.k_tiles, splits, s + 1) - mx_wgrad_first_tile(g.k_tiles, splits, s);
      lo = n < lo ? n : lo, hi = n > hi ? n : hi;
    }
    EXPECT(lo >= 1 && hi - lo <= 1);
    EXPECT(4 * static_cast<int64_t>(g.k_tiles) <= lds);  // the last K tile's scale dword
    for (int kc = 0; kc < 8; ++kc) {
      const int64_t k = static_cast<int64_t>(g.k_tiles - 1) * kFp8TileK + kc * 16;
      if (k < K) EXPECT(k + 16 <= K);
    }
    for (int n8 = 0; n8 < kMxWgTile; n8 += 8) {
      const int64_t n = (g.n_tiles - 1) * kMxWgTile + n8;
      if (n < N) EXPECT(n + 8 <= N);
    }
  }
}

// mx_wgrad.hip's LDS rows: wave w's DMA piece j holds rows 32 w + 8 j .. + 7, and B's row of LDS row rho0 + 8 j is
// b_row(rho0) + 16 (j & 1) + 4 (j >> 1); b_row is a permutation of each 64-row group. Its scale area is
// walk_scale_area's over 256 rows: wave row wm reads groups 2 wm and 2 wm + 1, wave column wn group wn
static void walk_wgrad_lds() {
  const auto b_row = [](int rho) {
    return (rho & 192) + 32 * ((rho >> 5) & 1) + 8 * ((rho >> 2) & 3) + 4 * ((rho >> 4) & 1) + (rho & 3);
  };
  std::vector<int> rows(kMxWgTile, 0), brows(kMxWgTile, 0), seen(kMxWgTile * 4, 0);
  for (int w = 0; w < kMxWgThreads / 64; ++w)
    for (int j = 0; j < 4; ++j)
      for (int r = 0; r < 8; ++r) {
        const int rho = 32 * w + 8 * j + r;
        EXPECT(rho < kMxWgTile && b_row(rho) == b_row(32 * w + r) + 16 * (j & 1) + 4 * (j >> 1));
        EXPECT((b_row(rho) & 192) == (rho & 192));
        if (rho < kMxWgTile) ++rows[rho], ++brows[b_row(rho)];
      }
  for (int v : rows) EXPECT(v == 1);
  for (int v : brows) EXPECT(v == 1);
  for (int rho = 0; rho < kMxWgTile; ++rho)
    for (int g = 0; g < 4; ++g) {
      const int ofs = (((rho >> 6) * 4) * 16 + (rho & 15)) * 4 + ((rho >> 4) & 3) + g * 64;
      EXPECT(ofs >= 0 && ofs < kMxWgTile * 4);
      if (ofs >= 0 && ofs < kMxWgTile * 4) ++seen[ofs];
      EXPECT(ofs == ((rho >> 6) * 64 + 16 * g + (rho & 15)) * 4 + ((rho >> 4) & 3));
    }
  for (int v : seen) EXPECT(v == 1);
}

template <typename F> static void rejects(const char* what, F&& f) {
  try {
    f();
  } catch (const std::runtime_error& e) {
    if (std::string(e.what()).rfind("mx_", 0) != 0) {
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
  for (auto [r, c, ld] : std::vector<std::array<int64_t, 3>>{
           {1, 32, 32}, {17, 96, 96}, {130, 160, 168}, {300, 416, 416}, {32, 32, 32}, {160, 96, 104}, {288, 416, 416},
           {50432, 768, 768}, {2304, 768, 768}, {50432, 2304, 2304}, {kFp8MaxDim, 32, 32},
           {32, kFp8MaxDim - 224, kFp8MaxDim - 224}})
    walk_quant(r, c, ld), ++shapes;
  for (int64_t m : {1, 127, 129, 300})
    for (int64_t n : {8, 136})
      for (int64_t k : {32, 128, 160, 416}) walk_gemm(m, n, k), ++shapes;
  for (auto [m, n, k] : std::vector<std::array<int64_t, 3>>{{256, 256, 256}, {50432, 2304, 768}, {50432, 768, 2304},
                                                          {50432, 3072, 768}, {50432, 768, 3072}, {kFp8MaxDim, 8, 32},
                                                          {1, kFp8MaxDim - 248, 32}, {1, 8, kFp8MaxDim - 224}})
    walk_gemm(m, n, k), ++shapes;
  walk_scale_area();
  for (auto [r, c] : std::vector<std::array<int64_t, 2>>{{32, 32}, {128, 128}, {160, 416}, {32, 544}, {130, 160}, {1, 32},
                                                         {50432, 768}, {2304, 768}, {50432, 2304}, {kFp8MaxDim, 32}})
    walk_fp6(r, c), ++shapes;
  for (int64_t m : {1, 129, 300})
    for (int64_t n : {8, 264})
      for (auto [k, wanted] : std::vector<std::array<int64_t, 2>>{{32, 1}, {160, 2}, {416, 3}, {1312, 4}, {1312, 64}, {1312, 0}})
        walk_wgrad(m, n, k, wanted), ++shapes;
  for (auto [m, n, k, wanted] : std::vector<std::array<int64_t, 4>>{{2304, 768, 50432, 9}, {768, 768, 50432, 28},
                                                                  {3072, 768, 50432, 7}, {768, 3072, 50432, 1},
                                                                  {160, 96, 160, -5}, {kFp8MaxDim, 8, 32, 1},
                                                                  {1, 8, kFp8MaxDim - 224, 1 << 30}})
    walk_wgrad(m, n, k, wanted), ++shapes;
  walk_wgrad_lds();

  const auto quant = [&](int64_t R, int64_t C, int64_t ld, const void* x = X, int fmt = 0, void* q = Q, int64_t ldq = -1,
                         void* s = S, int64_t lds = -1, void* qt = QT, int64_t ldt = -1, void* st = ST, int64_t ldst = -1) {
    mx_quant_check(x, R, C, ld, fmt, q, ldq < 0 ? C : ldq, s, lds < 0 ? mx_scale_row(C) : lds, qt, ldt < 0 ? R : ldt, st,
                   ldst < 0 ? mx_scale_row(R) : ldst);
  };
  quant(160, 96, 96);
  rejects("R = 0", [&] { quant(0, 96, 96); });
  rejects("R too large", [&] { quant(kFp8MaxDim + 32, 32, 32, X, 0, Q, -1, S, -1, nullptr, 0, nullptr, 0); });
  rejects("C = 0", [&] { quant(160, 0, 96); });
  rejects("C % 32", [&] { quant(160, 80, 96); });
  rejects("C too large", [&] { quant(32, kFp8MaxDim + 224, kFp8MaxDim + 224); });
  rejects("ld < C", [&] { quant(160, 96, 64); });
  rejects("ld % 8", [&] { quant(160, 96, 100); });
  rejects("null input", [&] { quant(160, 96, 96, nullptr); });
  rejects("unaligned input", [&] { quant(160, 96, 96, mem + 2); });
  quant(160, 96, 96, X, 2);  // e2m1: rows of C / 2 bytes fit the same strides
  quant(160, 96, 96, X, 3), quant(160, 96, 96, X, 4);  // fp6: rows of 72 and 120 bytes in strides of 96 and 160
  rejects("format 5", [&] { quant(160, 96, 96, X, 5); });
  rejects("fp6 ldq < 3 C / 4", [&] { quant(160, 96, 96, X, 3, Q, 64); });
  rejects("fp6 ldq % 16", [&] { quant(160, 96, 96, X, 3, Q, 72); });
  rejects("fp6 ldt < 3 R / 4", [&] { quant(160, 96, 96, X, 4, Q, -1, S, -1, QT, 112); });
  rejects("q without scales", [&] { quant(160, 96, 96, X, 0, Q, -1, nullptr); });
  rejects("scales without q", [&] { quant(160, 96, 96, X, 0, nullptr); });
  rejects("qt without scales", [&] { quant(160, 96, 96, X, 0, Q, -1, S, -1, QT, -1, nullptr); });
  rejects("nothing to do", [&] { quant(160, 96, 96, X, 0, nullptr, 0, nullptr, 0, nullptr, 0, nullptr, 0); });
  rejects("unaligned q", [&] { quant(160, 96, 96, X, 0, mem + 8); });
  rejects("ldq < C", [&] { quant(160, 96, 96, X, 0, Q, 80); });
  rejects("ldq % 16", [&] { quant(160, 96, 96, X, 0, Q, 104); });
  rejects("unaligned scales", [&] { quant(160, 96, 96, X, 0, Q, -1, mem + 2); });
  rejects("lds < 4 ceil(C / 128)", [&] { quant(160, 160, 160, X, 0, Q, -1, S, 4); });
  rejects("lds % 4", [&] { quant(160, 96, 96, X, 0, Q, -1, S, 6); });
  rejects("R % 32 with the transposed image", [&] { quant(130, 96, 96); });
  rejects("unaligned qt", [&] { quant(160, 96, 96, X, 0, Q, -1, S, -1, mem + 8); });
  rejects("ldt < R", [&] { quant(160, 96, 96, X, 0, Q, -1, S, -1, QT, 128); });
  rejects("ldt % 16", [&] { quant(160, 96, 96, X, 0, Q, -1, S, -1, QT, 168); });
  rejects("ldst < 4 ceil(R / 128)", [&] { quant(160, 96, 96, X, 0, Q, -1, S, -1, QT, -1, ST, 4); });
  rejects("too many workgroups", [&] { quant(kFp8MaxDim - 224, kFp8MaxDim - 224, kFp8MaxDim - 224); });

  const auto gemm = [&](int64_t M, int64_t N, int64_t K, int64_t lda = -1, int64_t ldb = -1, int64_t ldc = -1,
                        const void* a = X, const void* b = Q, const void* c = QT, const void* bias = nullptr, int bt = 0,
                        const void* sa = S, const void* sb = ST, int64_t ldsa = -1, int64_t ldsb = -1, int fa = 0,
                        int fb = 0) {
    mx_gemm_check(a, b, c, bias, bt, sa, sb, M, N, K, lda < 0 ? K : lda, ldb < 0 ? K : ldb, ldc < 0 ? N : ldc,
                  ldsa < 0 ? mx_scale_row(K) : ldsa, ldsb < 0 ? mx_scale_row(K) : ldsb, fa, fb);
  };
  gemm(130, 136, 160);
  rejects("M = 0", [&] { gemm(0, 136, 160); });
  rejects("M too large", [&] { gemm(kFp8MaxDim + 1, 8, 32); });
  rejects("N = 0", [&] { gemm(130, 0, 160); });
  rejects("N % 8", [&] { gemm(130, 132, 160); });
  rejects("N too large", [&] { gemm(1, kFp8MaxDim + 8, 32); });
  rejects("K = 0", [&] { gemm(130, 136, 0); });
  rejects("K % 32", [&] { gemm(130, 136, 144); });
  rejects("K too large", [&] { gemm(1, 8, kFp8MaxDim + 224); });
  rejects("lda < K", [&] { gemm(130, 136, 160, 128); });
  rejects("lda % 16", [&] { gemm(130, 136, 160, 168); });
  rejects("ldb < K", [&] { gemm(130, 136, 160, 160, 128); });
  rejects("ldc < N", [&] { gemm(130, 136, 160, 160, 160, 128); });
  rejects("ldc % 8", [&] { gemm(130, 136, 160, 160, 160, 140); });
  rejects("null a", [&] { gemm(130, 136, 160, -1, -1, -1, nullptr); });
  rejects("null c", [&] { gemm(130, 136, 160, -1, -1, -1, X, Q, nullptr); });
  rejects("unaligned b", [&] { gemm(130, 136, 160, -1, -1, -1, X, mem + 4); });
  rejects("unaligned bias", [&] { gemm(130, 136, 160, -1, -1, -1, X, Q, QT, mem + 4, 9); });
  rejects("fp16 bias", [&] { gemm(130, 136, 160, -1, -1, -1, X, Q, QT, X, 6); });
  rejects("null scale image", [&] { gemm(130, 136, 160, -1, -1, -1, X, Q, QT, nullptr, 0, nullptr); });
  rejects("unaligned scale image", [&] { gemm(130, 136, 160, -1, -1, -1, X, Q, QT, nullptr, 0, S, mem + 1); });
  rejects("ldsa < 4 ceil(K / 128)", [&] { gemm(130, 136, 160, -1, -1, -1, X, Q, QT, nullptr, 0, S, ST, 4); });
  rejects("ldsb % 4", [&] { gemm(130, 136, 160, -1, -1, -1, X, Q, QT, nullptr, 0, S, ST, 8, 10); });
  rejects("format of a", [&] { gemm(130, 136, 160, -1, -1, -1, X, Q, QT, nullptr, 0, S, ST, -1, -1, 2); });
  rejects("e5m2 b", [&] { gemm(130, 136, 160, -1, -1, -1, X, Q, QT, nullptr, 0, S, ST, -1, -1, 0, 1); });
  rejects("too many workgroups", [&] { gemm(kFp8MaxDim, kFp8MaxDim - 248, 32); });
  gemm(130, 136, 160, -1, -1, -1, X, Q, QT, nullptr, 0, S, ST, -1, -1, 3, 3);  // fp6 rows of 120 bytes in strides of 160
  gemm(130, 136, 160, 128, 128, -1, X, Q, QT, nullptr, 0, S, ST, -1, -1, 4, 3);
  for (auto [fa, fb] : std::vector<std::array<int, 2>>{{3, 4}, {4, 4}, {0, 3}, {1, 3}, {2, 3}, {3, 0}, {4, 0}, {3, 2}, {4, 2}, {5, 3}})
    rejects("a pair with an fp6 side that is not built",
            [&, fa = fa, fb = fb] { gemm(130, 136, 160, -1, -1, -1, X, Q, QT, nullptr, 0, S, ST, -1, -1, fa, fb); });
  rejects("fp6 lda < 3 K / 4", [&] { gemm(130, 136, 160, 112, -1, -1, X, Q, QT, nullptr, 0, S, ST, -1, -1, 3, 3); });
  rejects("fp6 ldb % 16", [&] { gemm(130, 136, 160, -1, 120, -1, X, Q, QT, nullptr, 0, S, ST, -1, -1, 3, 3); });

  const auto wgrad = [&](int64_t M, int64_t N, int64_t K, int64_t splits = 1, int64_t lda = -1, int64_t ldb = -1,
                         const void* a = X, const void* b = Q, const void* ws = QT, const void* sa = S,
                         const void* sb = ST, int64_t ldsa = -1, int64_t ldsb = -1, int fa = 0, int fb = 0) {
    mx_wgrad_check(a, b, ws, sa, sb, M, N, K, lda < 0 ? K : lda, ldb < 0 ? K : ldb, ldsa < 0 ? mx_scale_row(K) : ldsa,
                   ldsb < 0 ? mx_scale_row(K) : ldsb, fa, fb, splits);
  };
  wgrad(300, 264, 416, 3);
  rejects("M = 0", [&] { wgrad(0, 264, 416); });
  rejects("M too large", [&] { wgrad(kFp8MaxDim + 1, 8, 32); });
  rejects("N = 0", [&] { wgrad(300, 0, 416); });
  rejects("N % 8", [&] { wgrad(300, 260, 416); });
  rejects("K = 0", [&] { wgrad(300, 264, 0); });
  rejects("K % 32", [&] { wgrad(300, 264, 400); });
  rejects("K too large", [&] { wgrad(1, 8, kFp8MaxDim + 224); });
  rejects("splits = 0", [&] { wgrad(300, 264, 416, 0); });
  rejects("splits above the K tiles", [&] { wgrad(300, 264, 416, 5); });
  rejects("lda < K", [&] { wgrad(300, 264, 416, 1, 384); });
  rejects("lda % 16", [&] { wgrad(300, 264, 416, 1, 424); });
  rejects("ldb < K", [&] { wgrad(300, 264, 416, 1, 416, 384); });
  rejects("ldb % 16", [&] { wgrad(300, 264, 416, 1, 416, 424); });
  rejects("null a", [&] { wgrad(300, 264, 416, 1, -1, -1, nullptr); });
  rejects("null ws", [&] { wgrad(300, 264, 416, 1, -1, -1, X, Q, nullptr); });
  rejects("unaligned b", [&] { wgrad(300, 264, 416, 1, -1, -1, X, mem + 4); });
  rejects("unaligned ws", [&] { wgrad(300, 264, 416, 1, -1, -1, X, Q, mem + 8); });
  rejects("null scale image", [&] { wgrad(300, 264, 416, 1, -1, -1, X, Q, QT, nullptr); });
  rejects("unaligned scale image", [&] { wgrad(300, 264, 416, 1, -1, -1, X, Q, QT, S, mem + 1); });
  rejects("ldsa < 4 ceil(K / 128)", [&] { wgrad(300, 264, 416, 1, -1, -1, X, Q, QT, S, ST, 12); });
  rejects("ldsb % 4", [&] { wgrad(300, 264, 416, 1, -1, -1, X, Q, QT, S, ST, 16, 18); });
  rejects("format of a", [&] { wgrad(300, 264, 416, 1, -1, -1, X, Q, QT, S, ST, -1, -1, 2); });
  rejects("e5m2 b", [&] { wgrad(300, 264, 416, 1, -1, -1, X, Q, QT, S, ST, -1, -1, 0, 1); });
  rejects("fp6 a", [&] { wgrad(300, 264, 416, 1, -1, -1, X, Q, QT, S, ST, -1, -1, 4, 0); });
  rejects("fp6 b", [&] { wgrad(300, 264, 416, 1, -1, -1, X, Q, QT, S, ST, -1, -1, 0, 3); });
  rejects("too many workgroups", [&] { wgrad(kFp8MaxDim, kFp8MaxDim - 248, 32); });
  rejects("mx_wgrad_splits: K = 0", [&] { mx_wgrad_splits(0, 1); });
  rejects("mx_wgrad_splits: K % 32", [&] { mx_wgrad_splits(144, 2); });
  rejects("mx_wgrad_splits: K too large", [&] { mx_wgrad_splits(kFp8MaxDim + 224, 2); });

  if (failures != 0) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("mx_host_check: ok (%d shapes)\n", shapes);
  return 0;
}
