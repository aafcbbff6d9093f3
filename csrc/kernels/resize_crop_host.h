// Host side of resized_crop_batch (resize_crop.hip) without the launch: the argument checks and the
// launch geometry, plain C++ so that a stand-alone program can walk them under a sanitizer
// (scripts/resize_host_check.cpp).
//
// Geometry. A workgroup owns `rows` consecutive output rows of one sample: grid = B * row_blocks. It
// stages source rows of the sample's box (3 * bw bytes from byte 3 * left of an image row, at most W
// pixels, starting at an arbitrary byte) into `slots` = 2 * rows LDS rows per set by aligned 16-byte
// chunks: `chunks` of them cover 3 * W bytes from any of the 16 misalignments; an LDS row is 16 * chunks
// bytes plus 16 of slack (a lane reads 3 aligned dwords around its 6 bytes). `sets`: 2 when the
// partner's rows are staged too (a mixing mode, or a device block that may select one). In front of
// the staged rows the LDS holds three tables per set: the row terms (kRrcMaxRows words), the source
// row of each slot (2 * kRrcMaxRows words) and the column terms (w rounded up to 8 words). The 256
// lanes walk rows x (a power of two of lanes along the row), for the staging and for the output alike.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "../api.h"

namespace fluxmpi {

constexpr int kRrcThreads = 256;
constexpr int kRrcMaxRows = 8;
constexpr int kRrcMaxSide = 16384;        // every index product then fits 32 bits
constexpr int kRrcLdsBudget = 32 * 1024;  // bytes of LDS a workgroup aims to stay within
constexpr int kRrcLdsLimit = 64 * 1024;   // and may not exceed

struct RrcGeometry {
  int chunks;      // 16-byte chunks per staged row at most
  int row_bytes;   // LDS bytes per staged row
  int sets;        // 1: the sample's rows, 2: the partner's too
  int rows;        // output rows per workgroup
  int slots;       // staged rows per set: 2 * rows
  int row_blocks;  // workgroups per sample
  int64_t grid;    // workgroups (0: nothing to launch)
  int wpad;        // words of one set's column table
  // byte offsets into the LDS: row terms [sets][kRrcMaxRows], slot sources [sets][2 kRrcMaxRows],
  // column terms [sets][wpad], staged rows [sets][slots][row_bytes]
  int row_tab, slot_tab, col_tab, stage;
  // the lanes of a workgroup as (rows in flight) x (2^shift lanes along a row): no division in the kernel
  int stage_shift;  // staging: lanes along a row's chunks
  int item_shift;   // output: lanes along a row's items (w / 8 vector groups + w % 8 tail pixels)
  size_t lds_bytes;
};

inline void rrc_check(const void* in, const void* out, const void* boxes, int64_t B, int H, int W, int h, int w, int C,
                      bool dtype_ok, const AugHyper& a) {
  const auto fail = [](const std::string& m) { throw std::runtime_error("resized_crop_batch: " + m); };
  if (B < 0) fail("negative batch");
  if (B > 0x7fffffffLL) fail("batch above 2^31 - 1");
  if (H < 1 || W < 1 || h < 1 || w < 1) fail("image and output sizes must be positive");
  if (H > kRrcMaxSide || W > kRrcMaxSide || h > kRrcMaxSide || w > kRrcMaxSide) fail("sides above 16384");
  if (C != 3 && C != 4) fail("channels must be 3 or 4");
  if (!dtype_ok) fail("the output is bf16 or fp16");
  if (a.pad != 0 || a.fill != 0) fail("a box lies inside the image: pad and fill must be 0");
  if (a.dev_block == nullptr) {
    if (a.mode < 0 || a.mode > 2) fail("mode must be 0, 1 or 2");
    if (a.mode == 2 && !(0 <= a.y0 && a.y0 <= a.y1 && a.y1 <= h && 0 <= a.x0 && a.x0 <= a.x1 && a.x1 <= w))
      fail("the cutmix box must lie inside the output");
  } else if (reinterpret_cast<uintptr_t>(a.dev_block) % 4 != 0) {
    fail("the device block must be 4-byte aligned");
  }
  if (B > 0 && (in == nullptr || out == nullptr || boxes == nullptr)) fail("null tensor");
  if (reinterpret_cast<uintptr_t>(out) % 16 != 0) fail("the output must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(boxes) % 4 != 0) fail("the box table must be 4-byte aligned");
}

#if defined(__HIPCC__)
#define FLUXMPI_RRC_HD __host__ __device__ __forceinline__
#else
#define FLUXMPI_RRC_HD inline
#endif

// Output index i of n_out over n_src source pixels (half-pixel centres): the pair (p0, p1) and the
// weight f of p1 in 1/2048, rounded. The kernel's own arithmetic, here so that the host check walks it:
// 0 <= p0 <= p1 <= n_src - 1, p1 - p0 <= 1, f <= 2048; sides <= kRrcMaxSide keep every product in 32 bits.
struct RrcTerm {
  int p0, p1;
  uint32_t f;
};

FLUXMPI_RRC_HD RrcTerm rrc_term(int i, int n_src, int n_out) {
  const int num = (2 * i + 1) * n_src - n_out;  // below 2^30
  RrcTerm t{0, 0, 0u};
  if (num >= 0) {
    const uint32_t den = 2u * static_cast<uint32_t>(n_out);
    const uint32_t q = static_cast<uint32_t>(num) / den;
    const uint32_t rem = static_cast<uint32_t>(num) - q * den;
    t.p0 = static_cast<int>(q);
    t.f = (rem * 2048u + static_cast<uint32_t>(n_out)) / den;
  }
  t.p1 = t.p0 + 1 < n_src ? t.p0 + 1 : n_src - 1;
  return t;
}

// log2 of the smallest power of two >= n, at most log2(kRrcThreads)
inline int rrc_lane_shift(int n) {
  int s = 0;
  while ((1 << s) < n && (1 << s) < kRrcThreads) ++s;
  return s;
}

inline RrcGeometry rrc_geometry(int64_t B, int W, int h, int w, bool partner) {
  RrcGeometry g{};
  // 3 * W bytes from a misalignment of up to 15: ceil((15 + 3 W) / 16) chunks
  g.chunks = (3 * W + 15 + 15) / 16;
  g.row_bytes = 16 * g.chunks + 16;  // 16 of slack: a lane reads 3 aligned dwords around its 6 bytes
  g.sets = partner ? 2 : 1;
  g.wpad = (w + 7) & ~7;
  g.row_tab = 0;
  g.slot_tab = g.row_tab + 4 * kRrcMaxRows * g.sets;
  g.col_tab = g.slot_tab + 4 * 2 * kRrcMaxRows * g.sets;
  g.stage = g.col_tab + 4 * g.wpad * g.sets;
  const int per_row = 2 * g.row_bytes * g.sets;  // an output row's pair of source rows
  if (g.stage + per_row > kRrcLdsLimit)
    throw std::runtime_error("resized_crop_batch: the image or the output is too wide to stage one output row's pair of source rows");
  int rows = (kRrcLdsBudget - g.stage) / per_row;
  if (rows < 1) rows = 1;
  if (rows > kRrcMaxRows) rows = kRrcMaxRows;
  if (rows > h) rows = h;
  g.rows = rows;
  g.slots = 2 * rows;
  g.row_blocks = (h + rows - 1) / rows;
  g.grid = B * g.row_blocks;
  if (g.grid > 0x7fffffffLL) throw std::runtime_error("resized_crop_batch: too many workgroups for one launch");
  g.lds_bytes = static_cast<size_t>(g.stage) + static_cast<size_t>(per_row) * rows;
  g.stage_shift = rrc_lane_shift(g.chunks);
  g.item_shift = rrc_lane_shift((w >> 3) + (w & 7));
  return g;
}

}  // namespace fluxmpi
