// Stand-alone walk of augment_batch's host code (csrc/kernels/augment_host.h: the argument checks and
// the launch geometry) for a sanitizer run on the CPU; no GPU, no Python:
//
//   amdclang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -D__HIP_PLATFORM_AMD__=1 -I csrc -I $ROCM_PATH/include scripts/augment_host_check.cpp \
//       -o build/augment_host_check && build/augment_host_check
//
// It walks the shapes of tests/test_augment_gpu.py, B = 0, the widest row that fits and the extremes
// of every checked range, and verifies the geometry's invariants: the workgroups cover every output row
// once, a staged row holds 3 * span bytes from any of the 16 misalignments plus the 7-dword read
// around a lane's 24 bytes, and the LDS stays within 64 KiB. Exit status 0 and "ok" when all hold.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels/augment_host.h"

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
  int H, W, h, w, pad;
};

static AugHyper hyper(int pad) {
  AugHyper a{};
  a.pad = pad;
  a.a[0] = a.a[1] = a.a[2] = 1.f;
  return a;
}

static void walk(const Shape& s) {
  alignas(16) static unsigned char in[64], out[64];
  for (int C : {3, 4}) {
    for (int mode : {0, 1, 2}) {
      AugHyper a = hyper(s.pad);
      a.mode = mode;
      if (mode == 2) a.y0 = 0, a.x0 = 0, a.y1 = s.h, a.x1 = s.w;
      for (int off = 0; off < 4; ++off) aug_check(in + off, out, s.B, s.H, s.W, s.h, s.w, C, true, a);
      const AugGeometry g = aug_geometry(s.B, s.W, s.h, s.w, mode != 0);
      EXPECT(g.rows >= 1 && g.rows <= kAugMaxRows && g.rows <= s.h);
      EXPECT(static_cast<int64_t>(g.rows) * g.row_blocks >= s.h);
      EXPECT(static_cast<int64_t>(g.rows) * (g.row_blocks - 1) < s.h);
      EXPECT(g.grid == s.B * g.row_blocks);
      EXPECT(g.sets == (mode != 0 ? 2 : 1));
      EXPECT(g.span == (s.w < s.W ? s.w : s.W));
      for (int mis = 0; mis < 16; ++mis) {
        const int nch = (mis + 3 * g.span + 15) >> 4;  // the kernel's chunk count of a full span
        EXPECT(nch <= g.chunks);
        // the last lane's 7 aligned dwords end inside the row
        if (g.span >= 8) EXPECT(((mis + 3 * (g.span - 8)) & ~3) + 28 <= g.row_bytes);
      }
      EXPECT(g.row_bytes % 16 == 0 && g.row_bytes >= 16 * g.chunks + 16);
      EXPECT(g.lds_bytes == static_cast<size_t>(g.row_bytes) * g.sets * g.rows);
      EXPECT(g.lds_bytes <= 64 * 1024);
      const int items = (s.w >> 3) + (s.w & 7);
      for (const int* p : {&g.stage_shift, &g.item_shift}) {
        const int n = p == &g.stage_shift ? g.chunks : items;
        EXPECT(*p >= 0 && (1 << *p) <= kAugThreads);
        EXPECT((1 << *p) >= n || (1 << *p) == kAugThreads);  // a row in one pass, or every lane on it
        EXPECT(*p == 0 || (1 << (*p - 1)) < n);               // and no wider than that
      }
    }
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
  const std::vector<Shape> shapes = {
      {5, 37, 41, 32, 36, 4},   {5, 37, 41, 37, 41, 0},  {5, 37, 41, 32, 8, 4},  {5, 37, 41, 32, 7, 4},
      {5, 37, 41, 1, 36, 4},    {5, 37, 41, 45, 57, 10}, {1, 37, 41, 32, 36, 4}, {0, 37, 41, 32, 36, 4},
      {2, 256, 256, 224, 224, 0}, {256, 256, 256, 224, 224, 0}, {4, 16384, 16384, 8, 24, 0},
      {1, 1, 1, 1, 1, 0},       {1, 1, 1, 3, 3, 1},      {3, 8, 10000, 8, 10000, 0}, {1, 1 << 24, 1, 1 << 24, 1, 0},
      {(1LL << 31) / 32 - 1, 32, 32, 32, 32, 4},
  };
  for (const Shape& s : shapes) walk(s);

  alignas(16) static unsigned char in[64], out[64];
  const AugHyper ok = hyper(4);
  aug_check(nullptr, nullptr, 0, 37, 41, 32, 36, 3, true, ok);  // an empty batch has no tensors
  rejects("negative batch", [&] { aug_check(in, out, -1, 37, 41, 32, 36, 3, true, ok); });
  rejects("null input", [&] { aug_check(nullptr, out, 5, 37, 41, 32, 36, 3, true, ok); });
  rejects("unaligned output", [&] { aug_check(in, out + 2, 5, 37, 41, 32, 36, 3, true, ok); });
  rejects("channels", [&] { aug_check(in, out, 5, 37, 41, 32, 36, 5, true, ok); });
  rejects("dtype", [&] { aug_check(in, out, 5, 37, 41, 32, 36, 3, false, ok); });
  rejects("zero size", [&] { aug_check(in, out, 5, 37, 41, 0, 36, 3, true, ok); });
  rejects("too tall", [&] { aug_check(in, out, 5, 37, 41, 46, 36, 3, true, ok); });
  rejects("too wide", [&] { aug_check(in, out, 5, 37, 41, 32, 50, 3, true, ok); });
  rejects("huge side", [&] { aug_check(in, out, 1, (1 << 24) + 1, 1, 1, 1, 3, true, ok); });
  {
    AugHyper a = ok;
    a.pad = -1;
    rejects("negative pad", [&] { aug_check(in, out, 5, 37, 41, 32, 36, 3, true, a); });
    a.pad = 0x7fffffff;  // 2 * pad would overflow an int: refused before it is formed
    rejects("huge pad", [&] { aug_check(in, out, 5, 37, 41, 32, 36, 3, true, a); });
    a = ok, a.fill = 256;
    rejects("fill", [&] { aug_check(in, out, 5, 37, 41, 32, 36, 3, true, a); });
    a = ok, a.stream = 1u << 30;
    rejects("stream", [&] { aug_check(in, out, 5, 37, 41, 32, 36, 3, true, a); });
    a = ok, a.sample_offset = -1;
    rejects("sample_offset", [&] { aug_check(in, out, 5, 37, 41, 32, 36, 3, true, a); });
    a = ok, a.mode = 3;
    rejects("mode", [&] { aug_check(in, out, 5, 37, 41, 32, 36, 3, true, a); });
    a = ok, a.mode = 2, a.y0 = 0, a.x0 = 0, a.y1 = 33, a.x1 = 36;
    rejects("box", [&] { aug_check(in, out, 5, 37, 41, 32, 36, 3, true, a); });
    a = ok, a.dev_block = reinterpret_cast<const uint32_t*>(in + 2);
    rejects("block alignment", [&] { aug_check(in, out, 5, 37, 41, 32, 36, 3, true, a); });
    a = ok, a.dev_block = reinterpret_cast<const uint32_t*>(in), a.mode = 77;  // the block supplies the mode
    aug_check(in, out, 5, 37, 41, 32, 36, 3, true, a);
  }
  rejects("row too wide for the LDS", [&] { aug_geometry(1, 1 << 24, 8, 1 << 24, true); });
  rejects("grid", [&] { aug_geometry(1LL << 31, 41, 32, 36, false); });

  if (failures != 0) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::puts("augment_host_check: ok");
  return 0;
}
