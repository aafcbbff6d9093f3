// Stand-alone walk of resized_crop_batch's host code (csrc/kernels/resize_crop_host.h: the argument
// checks, the launch geometry and the resampling terms the kernel shares with it) for a sanitizer run
// on the CPU; no GPU, no Python:
//
//   amdclang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -D__HIP_PLATFORM_AMD__=1 -I csrc -I $ROCM_PATH/include scripts/resize_host_check.cpp \
//       -o build/resize_host_check && build/resize_host_check
//
// It walks the shapes of tests/test_resize_crop_gpu.py, B = 0, the widest image that fits with one and
// with two sets, the first that does not, and the extremes of every checked range, and verifies the
// geometry's invariants: the workgroups cover every output row once; a staged row holds 3 * W bytes
// from any of the 16 misalignments plus the 3-dword read around a lane's 6 bytes; the tables and the staged rows do not overlap and stay within
// 64 KiB; a term's pair lies inside the box and its weight within 2048; and for a box of at most twice
// the output's height the source rows of a workgroup fit its slots (the union path). Exit status 0 and
// "ok" when all hold.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels/resize_crop_host.h"

using namespace fluxmpi;

static int failures = 0;
#define EXPECT(cond)                                                         \
  do {                                                                       \
    if (!(cond)) {                                                           \
      std::fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); \
      ++failures;                                                            \
    }                                                                        \
  } while (0)

struct Shape {
  int64_t B;
  int H, W, h, w;
};

static AugHyper hyper() {
  AugHyper a{};
  a.a[0] = a.a[1] = a.a[2] = 1.f;
  return a;
}

// every output index of n_out over boxes of n_src pixels: the pair, the weight, and monotony
static void walk_terms(int n_src, int n_out) {
  int prev = 0;
  for (int i = 0; i < n_out; ++i) {
    const RrcTerm t = rrc_term(i, n_src, n_out);
    EXPECT(t.p0 >= 0 && t.p0 <= t.p1 && t.p1 <= n_src - 1 && t.p1 - t.p0 <= 1);
    EXPECT(t.f <= 2048u);
    EXPECT(t.p0 >= prev);
    prev = t.p0;
    if (n_src == n_out) EXPECT(t.p0 == i && t.f == 0u);  // the identity scale is the plain crop
  }
}

static void walk(const Shape& s) {
  alignas(16) static unsigned char in[64], out[64];
  alignas(16) static int32_t boxes[16];
  for (int C : {3, 4}) {
    for (int mode : {0, 1, 2}) {
      AugHyper a = hyper();
      a.mode = mode;
      if (mode == 2) a.y0 = 0, a.x0 = 0, a.y1 = s.h, a.x1 = s.w;
      for (int off = 0; off < 4; ++off) rrc_check(in + off, out, boxes, s.B, s.H, s.W, s.h, s.w, C, true, a);
      const RrcGeometry g = rrc_geometry(s.B, s.W, s.h, s.w, mode != 0);
      EXPECT(g.rows >= 1 && g.rows <= kRrcMaxRows && g.rows <= s.h);
      EXPECT(g.slots == 2 * g.rows);
      EXPECT(static_cast<int64_t>(g.rows) * g.row_blocks >= s.h);
      EXPECT(static_cast<int64_t>(g.rows) * (g.row_blocks - 1) < s.h);
      EXPECT(g.grid == s.B * g.row_blocks);
      EXPECT(g.sets == (mode != 0 ? 2 : 1));
      for (int mis = 0; mis < 16; ++mis) {
        const int nch = (mis + 3 * s.W + 15) >> 4;  // the kernel's chunk count of the widest box
        EXPECT(nch <= g.chunks);
        // the last lane's 3 aligned dwords, around the 6 bytes from the last pixel on, end inside the row
        EXPECT(((mis + 3 * (s.W - 1)) & ~3) + 12 <= g.row_bytes);
      }
      EXPECT(g.row_bytes % 16 == 0 && g.row_bytes >= 16 * g.chunks + 16);
      // the tables, in order, without overlap, the staged rows 16-byte aligned
      EXPECT(g.wpad >= s.w && g.wpad % 8 == 0);
      EXPECT(g.row_tab == 0 && g.slot_tab >= g.row_tab + 4 * kRrcMaxRows * g.sets);
      EXPECT(g.col_tab >= g.slot_tab + 4 * 2 * kRrcMaxRows * g.sets);
      EXPECT(g.stage >= g.col_tab + 4 * g.wpad * g.sets && g.stage % 16 == 0);
      EXPECT(g.lds_bytes == static_cast<size_t>(g.stage) + static_cast<size_t>(g.row_bytes) * g.sets * g.slots);
      EXPECT(g.lds_bytes <= static_cast<size_t>(kRrcLdsLimit));
      const int items = (s.w >> 3) + (s.w & 7);
      for (const int* p : {&g.stage_shift, &g.item_shift}) {
        const int n = p == &g.stage_shift ? g.chunks : items;
        EXPECT(*p >= 0 && (1 << *p) <= kRrcThreads);
        EXPECT((1 << *p) >= n || (1 << *p) == kRrcThreads);  // a row in one pass, or every lane on it
        EXPECT(*p == 0 || (1 << (*p - 1)) < n);               // and no wider than that
      }
      // the union path: a box of at most twice the output's height never needs more rows than the slots
      for (int bh : {1, 2, s.h / 2 > 0 ? s.h / 2 : 1, s.h, s.h + 1, 2 * s.h - 1, 2 * s.h}) {
        if (bh > s.H || s.h > 4096) continue;
        for (int i0 = 0; i0 < s.h; i0 += g.rows) {
          const int last = i0 + g.rows <= s.h ? i0 + g.rows - 1 : s.h - 1;
          EXPECT(rrc_term(last, bh, s.h).p1 - rrc_term(i0, bh, s.h).p0 + 1 <= g.slots);
        }
      }
    }
  }
  if (s.h <= 4096 && s.w <= 4096)
    for (int n_src : {1, 2, 3, s.H, s.W}) {
      walk_terms(n_src, s.h);
      walk_terms(n_src, s.w);
    }
}

template <typename F> static void rejects(const char* what, F&& f) {
  try {
    f();
  } catch (const std::runtime_error&) {
    return;
  }
  std::fprintf(stderr, "not rejected: %s\n", what);
  ++failures;
}

int main() {
  // the widest images that fit: stage + 2 * sets * row_bytes <= 64 KiB (w = 8)
  int widest[2] = {0, 0};
  for (int sets = 1; sets <= 2; ++sets)
    for (int W = 1; W <= kRrcMaxSide; ++W) {
      try {
        rrc_geometry(1, W, 8, 8, sets == 2);
      } catch (const std::runtime_error&) {
        break;
      }
      widest[sets - 1] = W;
    }
  EXPECT(widest[0] > widest[1] && widest[1] >= 4096 && widest[0] < kRrcMaxSide);

  const std::vector<Shape> shapes = {
      {5, 37, 41, 32, 36},  {5, 37, 41, 32, 8},    {5, 37, 41, 32, 5},        {5, 37, 41, 3, 36},
      {5, 37, 41, 75, 50},  {1, 37, 41, 32, 36},   {0, 37, 41, 32, 36},       {4, 256, 256, 224, 224},
      {256, 256, 256, 224, 224}, {11, 16384, 4096, 8, 24}, {1, 1, 1, 1, 1},   {1, 1, 1, 16384, 4096},
      {2, 16384, 1, 1, 4096},   {1, 8, widest[1], 8, 8},  {3, 16384, widest[1], 16384, 8},
      {(1LL << 31) / 4 - 1, 32, 32, 32, 32},
  };
  for (const Shape& s : shapes) walk(s);
  rrc_geometry(1, widest[0], 8, 8, false);  // fits with one set ...
  rejects("two sets at the widest one-set image", [&] { rrc_geometry(1, widest[0], 8, 8, true); });
  rejects("first image too wide, one set", [&] { rrc_geometry(1, widest[0] + 1, 8, 8, false); });
  rejects("first image too wide, two sets", [&] { rrc_geometry(1, widest[1] + 1, 8, 8, true); });
  rejects("the widest side", [&] { rrc_geometry(1, kRrcMaxSide, 8, 8, false); });
  rejects("the widest output (its column table)", [&] { rrc_geometry(1, 1, 1, kRrcMaxSide, true); });
  rejects("grid", [&] { rrc_geometry(1LL << 31, 41, 32, 36, false); });
  // the largest products of a term: the extremes of every side
  for (int n_src : {1, kRrcMaxSide})
    for (int n_out : {1, kRrcMaxSide})
      for (int i : {0, n_out / 2, n_out - 1}) {
        const RrcTerm t = rrc_term(i, n_src, n_out);
        EXPECT(t.p0 >= 0 && t.p1 <= n_src - 1 && t.p0 <= t.p1 && t.f <= 2048u);
      }
  EXPECT(rrc_term(1, 2, 4).p0 == 0 && rrc_term(1, 2, 4).f == 512u && rrc_term(3, 2, 4).p0 == 1);

  alignas(16) static unsigned char in[64], out[64];
  alignas(16) static int32_t boxes[16];
  const AugHyper ok = hyper();
  rrc_check(nullptr, nullptr, nullptr, 0, 37, 41, 32, 36, 3, true, ok);  // an empty batch has no tensors
  rrc_check(in, out, boxes, 5, kRrcMaxSide, kRrcMaxSide, kRrcMaxSide, kRrcMaxSide, 4, true, ok);
  rejects("negative batch", [&] { rrc_check(in, out, boxes, -1, 37, 41, 32, 36, 3, true, ok); });
  rejects("huge batch", [&] { rrc_check(in, out, boxes, 1LL << 31, 37, 41, 32, 36, 3, true, ok); });
  rejects("null input", [&] { rrc_check(nullptr, out, boxes, 5, 37, 41, 32, 36, 3, true, ok); });
  rejects("null table", [&] { rrc_check(in, out, nullptr, 5, 37, 41, 32, 36, 3, true, ok); });
  rejects("unaligned table", [&] {
    rrc_check(in, out, reinterpret_cast<unsigned char*>(boxes) + 2, 5, 37, 41, 32, 36, 3, true, ok);
  });
  rejects("unaligned output", [&] { rrc_check(in, out + 2, boxes, 5, 37, 41, 32, 36, 3, true, ok); });
  rejects("channels", [&] { rrc_check(in, out, boxes, 5, 37, 41, 32, 36, 5, true, ok); });
  rejects("dtype", [&] { rrc_check(in, out, boxes, 5, 37, 41, 32, 36, 3, false, ok); });
  rejects("zero size", [&] { rrc_check(in, out, boxes, 5, 37, 41, 0, 36, 3, true, ok); });
  rejects("zero image", [&] { rrc_check(in, out, boxes, 5, 0, 41, 32, 36, 3, true, ok); });
  rejects("huge H", [&] { rrc_check(in, out, boxes, 1, kRrcMaxSide + 1, 1, 1, 1, 3, true, ok); });
  rejects("huge W", [&] { rrc_check(in, out, boxes, 1, 1, kRrcMaxSide + 1, 1, 1, 3, true, ok); });
  rejects("huge h", [&] { rrc_check(in, out, boxes, 1, 1, 1, kRrcMaxSide + 1, 1, 3, true, ok); });
  rejects("huge w", [&] { rrc_check(in, out, boxes, 1, 1, 1, 1, kRrcMaxSide + 1, 3, true, ok); });
  {
    AugHyper a = ok;
    a.pad = 1;
    rejects("pad", [&] { rrc_check(in, out, boxes, 5, 37, 41, 32, 36, 3, true, a); });
    a = ok, a.fill = 1;
    rejects("fill", [&] { rrc_check(in, out, boxes, 5, 37, 41, 32, 36, 3, true, a); });
    a = ok, a.mode = 3;
    rejects("mode", [&] { rrc_check(in, out, boxes, 5, 37, 41, 32, 36, 3, true, a); });
    a = ok, a.mode = -1;
    rejects("negative mode", [&] { rrc_check(in, out, boxes, 5, 37, 41, 32, 36, 3, true, a); });
    a = ok, a.mode = 2, a.y0 = 0, a.x0 = 0, a.y1 = 33, a.x1 = 36;
    rejects("box", [&] { rrc_check(in, out, boxes, 5, 37, 41, 32, 36, 3, true, a); });
    a = ok, a.dev_block = reinterpret_cast<const uint32_t*>(in + 2);
    rejects("block alignment", [&] { rrc_check(in, out, boxes, 5, 37, 41, 32, 36, 3, true, a); });
    a = ok, a.dev_block = reinterpret_cast<const uint32_t*>(in), a.mode = 77;  // the block supplies the mode
    rrc_check(in, out, boxes, 5, 37, 41, 32, 36, 3, true, a);
  }

  if (failures != 0) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("resize_host_check: ok (widest image: %d pixels with one set, %d with two)\n", widest[0], widest[1]);
  return 0;
}
