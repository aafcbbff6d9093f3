// Stand-alone walk of the host code of the Linear + add + LayerNorm forward (csrc/kernels/gemm_ln_host.h: the
// shape and alignment checks and the split of the rows over the persistent grid) for a sanitizer run on the CPU;
// no GPU, no Python:
//
//   amdclang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I csrc scripts/gemm_ln_host_check.cpp -o build/gemm_ln_host_check && build/gemm_ln_host_check
//
// For a sweep of (M, resident workgroups, max_blocks) it marks every 16-row unit a workgroup's tiles visit and
// verifies: the grid is 1 .. the cap and never leaves a workgroup without a unit; the ranges are contiguous,
// cover [0, units) once (cover and disjointness) and their lengths differ by at most one unit; a tile holds 1 .. 4
// units; the rows a workgroup stores ([first row, min(range end, M))) cover [0, M) once; and every row a tile may
// touch (64 from its first) keeps its byte offsets below 2^31 for the shapes the check accepts. Then the accepted
// and rejected shapes and pointers. Exit status 0 and "ok" when all hold.
#include <cstdio>
#include <vector>

#include "kernels/gemm_ln_host.h"

using namespace fluxmpi;

static int failures = 0;
#define EXPECT(cond)                                                         \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                            \
    }                                                                        \
  } while (0)

static void walk(int64_t M, int resident, int max_blocks) {
  const int64_t units = gemm_ln_units(M);
  const int G = gemm_ln_grid(M, resident, max_blocks);
  const int64_t cap = max_blocks > 0 ? max_blocks : resident;
  EXPECT(G >= 1 && G <= cap && G <= units);
  EXPECT(gemm_ln_range_start(units, G, 0) == 0 && gemm_ln_range_start(units, G, G) == units);
  std::vector<unsigned char> seen(static_cast<size_t>(units), 0);
  std::vector<unsigned char> rows(static_cast<size_t>(M), 0);
  int64_t lo = units, hi = 0;
  for (int b = 0; b < G; ++b) {
    const int64_t u0 = gemm_ln_range_start(units, G, b), u1 = gemm_ln_range_start(units, G, b + 1);
    EXPECT(u1 > u0);
    lo = u1 - u0 < lo ? u1 - u0 : lo;
    hi = u1 - u0 > hi ? u1 - u0 : hi;
    const int64_t ntiles = (u1 - u0 + 3) / 4;
    const int64_t row_end = u1 * kLnUnit < M ? u1 * kLnUnit : M;
    for (int64_t tt = 0; tt < ntiles; ++tt) {
      const int64_t left = u1 - u0 - 4 * tt, nu = left < 4 ? left : 4;
      EXPECT(nu >= 1 && nu <= 4);
      for (int64_t u = 0; u < nu; ++u) {
        const int64_t unit = u0 + 4 * tt + u;
        EXPECT(unit < units);
        if (unit < units) ++seen[static_cast<size_t>(unit)];
        for (int64_t r = unit * kLnUnit; r < (unit + 1) * kLnUnit && r < row_end; ++r) ++rows[static_cast<size_t>(r)];
      }
    }
  }
  EXPECT(hi - lo <= 1);
  for (unsigned char s : seen) EXPECT(s == 1);
  for (unsigned char s : rows) EXPECT(s == 1);
}

int main() {
  int walks = 0;
  for (int64_t M : {1, 15, 16, 17, 63, 64, 65, 77, 200, 333, 1023, 1024, 4097, 50432, 50433})
    for (int resident : {1, 2, 3, 7, 64, 256, 304})
      for (int max_blocks : {0, 1, 2, 5, 255, 1 << 20}) walk(M, resident, max_blocks), ++walks;

  for (int64_t N : {384, 768})
    for (int64_t K : {64, 128, 768, 3072}) {
      EXPECT(gemm_ln_shape_ok(1, N, K) && gemm_ln_shape_ok(50432, N, K));
      // the largest M taken: every byte offset of the 64 rows from a tile's first row stays below 2^31
      const int64_t widest = K > N ? K : N, top = (1LL << 31) / (2 * widest) - kLnBM;
      EXPECT(gemm_ln_shape_ok(top, N, K) && !gemm_ln_shape_ok(top + 1, N, K));
      EXPECT((top + kLnBM) * widest * 2 <= (1LL << 31));
    }
  EXPECT(!gemm_ln_shape_ok(0, 768, 768) && !gemm_ln_shape_ok(-3, 768, 768));
  EXPECT(!gemm_ln_shape_ok(200, 1032, 96) && !gemm_ln_shape_ok(200, 512, 128) && !gemm_ln_shape_ok(200, 0, 128));
  EXPECT(!gemm_ln_shape_ok(200, 768, 96) && !gemm_ln_shape_ok(200, 768, 32) && !gemm_ln_shape_ok(200, 768, 0));
  EXPECT(!gemm_ln_shape_ok(200, 768, (1 << 20) + 64));

  alignas(16) static unsigned char buf[64];
  EXPECT(gemm_ln_aligned16({buf, buf + 16, buf + 48}));
  EXPECT(!gemm_ln_aligned16({buf, buf + 8}) && !gemm_ln_aligned16({buf, nullptr}) && !gemm_ln_aligned16({buf + 2}));

  if (failures != 0) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("gemm_ln_host_check: ok (%d walks)\n", walks);
  return 0;
}
