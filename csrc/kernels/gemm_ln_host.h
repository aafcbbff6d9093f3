// Host side of the Linear + residual add + LayerNorm forward (gemm_ln.hip) without the launch: the shape and
// alignment checks and the split of the rows over the persistent grid, plain C++ so that a stand-alone program
// can walk them under a sanitizer (scripts/gemm_ln_host_check.cpp). The kernel calls the split's functions too.
//
// Geometry. A workgroup owns whole output rows (all N columns), kLnBM = 64 at a time. The M rows are cut into
// units of kLnUnit = 16 (one MFMA row tile); the ceil(M / 16) units are dealt to the G workgroups as contiguous
// ranges [start(b), start(b + 1)), start(b) = floor(units b / G): the ranges cover the units, are disjoint and
// their lengths differ by at most one unit. A workgroup walks its range in tiles of 4 units; the last tile of a
// range may hold 1 .. 3 units, and the last unit of all may hold fewer than 16 rows. G = min(cap, ceil(units /
// 4)), cap = max_blocks when > 0, else the resident workgroups: no range is empty and, while there is work for
// it, every workgroup has about a tile.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>

namespace fluxmpi {

constexpr int kLnBM = 64;       // rows of a tile
constexpr int kLnUnit = 16;     // rows of a unit (an MFMA row tile)
constexpr int kLnBK = 32;       // K elements per pipeline stage
constexpr int kLnThreads = 512;
constexpr int kLnStages = 3;

// N in {384, 768}; K a multiple of 64, at least 64; M >= 1; every byte offset into a, x, h, y of a row the
// kernel may touch (up to 63 rows past M, masked or read as zeros through a buffer resource) below 2^31
constexpr bool gemm_ln_shape_ok(int64_t M, int64_t N, int64_t K) {
  if (N != 384 && N != 768) return false;
  if (K < 64 || K % 64 != 0) return false;
  if (M < 1) return false;
  const int64_t widest = K > N ? K : N;
  return K <= (1 << 20) && M <= (1LL << 31) / (2 * widest) - kLnBM;
}

inline bool gemm_ln_aligned16(std::initializer_list<const void*> ptrs) {
  for (const void* q : ptrs)
    if (q == nullptr || reinterpret_cast<uintptr_t>(q) % 16 != 0) return false;
  return true;
}

constexpr int64_t gemm_ln_units(int64_t M) { return (M + kLnUnit - 1) / kLnUnit; }

// the persistent grid: resident = the workgroups one round keeps on the device (>= 1), max_blocks >= 0
constexpr int gemm_ln_grid(int64_t M, int resident, int max_blocks) {
  const int64_t tiles = (gemm_ln_units(M) + 3) / 4;
  const int64_t cap = max_blocks > 0 ? max_blocks : (resident > 0 ? resident : 1);
  return static_cast<int>(tiles < cap ? tiles : cap);
}

// first unit of workgroup b's range (b = G: one past the last unit)
constexpr int64_t gemm_ln_range_start(int64_t units, int G, int b) { return units * b / G; }

}  // namespace fluxmpi
