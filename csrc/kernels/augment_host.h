// Host side of augment_batch (augment.hip) without the launch: the argument checks and the launch
// geometry, plain C++ so that a stand-alone program can walk them under a sanitizer
// (scripts/augment_host_check.cpp).
//
// Geometry. A workgroup owns `rows` consecutive output rows of one sample: grid = B * row_blocks.
// A row's source span (the columns of the crop that lie inside the image, at most min(w, W) pixels
// of 3 bytes, starting at an arbitrary byte) is staged into LDS by aligned 16-byte chunks: `chunks`
// of them cover 3 * span bytes from any of the 16 misalignments. An LDS row is 16 * chunks bytes plus
// 16 of slack (a lane reads 7 aligned dwords around its 24 bytes). `sets`: 2 when the partner's
// rows are staged too (a mixing mode, or a device block that may select one). The 256 lanes walk
// rows x (a power of two of lanes along the row), for the staging and for the output alike.
#pragma once
#include <cstddef>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "../api.h"

namespace fluxmpi {

constexpr int kAugThreads = 256;
constexpr int kAugMaxRows = 8;
constexpr int kAugLdsBudget = 32 * 1024;  // bytes of LDS a workgroup may stage into

struct AugGeometry {
  int span;        // staged pixels per row at most
  int chunks;      // 16-byte chunks per staged row at most
  int row_bytes;   // LDS bytes per staged row
  int sets;        // 1: the sample's rows, 2: the partner's too
  int rows;        // output rows per workgroup
  int row_blocks;  // workgroups per sample
  int64_t grid;    // workgroups (0: nothing to launch)
  // the lanes of a workgroup as (rows in flight) x (2^shift lanes along a row): no division in the kernel
  int stage_shift;  // staging: lanes along a row's chunks
  int item_shift;   // output: lanes along a row's items (w / 8 vector groups + w % 8 tail pixels)
  size_t lds_bytes;
};

inline void aug_check(const void* in, const void* out, int64_t B, int H, int W, int h, int w, int C, bool dtype_ok,
                      const AugHyper& a) {
  const auto fail = [](const std::string& m) { throw std::runtime_error("augment_batch: " + m); };
  if (B < 0) fail("negative batch");
  if (H < 1 || W < 1 || h < 1 || w < 1) fail("image and output sizes must be positive");
  if (C != 3 && C != 4) fail("channels must be 3 or 4");
  if (!dtype_ok) fail("the output is bf16 or fp16");
  if (a.pad < 0 || a.pad > (1 << 20)) fail("pad out of range");
  if (H > (1 << 24) || W > (1 << 24) || h > (1 << 24) || w > (1 << 24)) fail("sizes above 2^24");
  if (static_cast<int64_t>(h) > static_cast<int64_t>(H) + 2 * a.pad ||
      static_cast<int64_t>(w) > static_cast<int64_t>(W) + 2 * a.pad)
    fail("the output is larger than the padded image");
  if (a.fill < 0 || a.fill > 255) fail("fill is a byte");
  if (a.stream >= (1u << 30)) fail("the stream id must be below 2^30");
  if (a.sample_offset < 0) fail("sample_offset is not negative");
  if (a.dev_block == nullptr) {
    if (a.mode < 0 || a.mode > 2) fail("mode must be 0, 1 or 2");
    if (a.mode == 2 && !(0 <= a.y0 && a.y0 <= a.y1 && a.y1 <= h && 0 <= a.x0 && a.x0 <= a.x1 && a.x1 <= w))
      fail("the cutmix box must lie inside the output");
  } else if (reinterpret_cast<uintptr_t>(a.dev_block) % 4 != 0) {
    fail("the device block must be 4-byte aligned");
  }
  if (B > 0 && (in == nullptr || out == nullptr)) fail("null tensor");
  if (reinterpret_cast<uintptr_t>(out) % 16 != 0) fail("the output must be 16-byte aligned");
}

// log2 of the smallest power of two >= n, at most log2(kAugThreads)
inline int aug_lane_shift(int n) {
  int s = 0;
  while ((1 << s) < n && (1 << s) < kAugThreads) ++s;
  return s;
}

inline AugGeometry aug_geometry(int64_t B, int W, int h, int w, bool partner) {
  AugGeometry g{};
  g.span = w < W ? w : W;
  // 3 * span bytes from a misalignment of up to 15: ceil((15 + 3 span) / 16) chunks
  g.chunks = (3 * g.span + 15 + 15) / 16;
  g.row_bytes = 16 * g.chunks + 16;
  g.sets = partner ? 2 : 1;
  const int per_row = g.row_bytes * g.sets;
  if (per_row > 2 * kAugLdsBudget) throw std::runtime_error("augment_batch: the output is too wide to stage a row");
  int rows = kAugLdsBudget / per_row;
  if (rows < 1) rows = 1;
  if (rows > kAugMaxRows) rows = kAugMaxRows;
  if (rows > h) rows = h;
  g.rows = rows;
  g.row_blocks = (h + rows - 1) / rows;
  g.grid = B * g.row_blocks;
  if (g.grid > 0x7fffffffLL) throw std::runtime_error("augment_batch: too many workgroups for one launch");
  g.lds_bytes = static_cast<size_t>(per_row) * rows;
  g.stage_shift = aug_lane_shift(g.chunks);
  g.item_shift = aug_lane_shift((w >> 3) + (w & 7));
  return g;
}

}  // namespace fluxmpi
