// Stand-alone walk of the patch-embedding entries' host code (csrc/kernels/patch_embed_host.h: the
// argument checks and the launch geometry) for a sanitizer run on the CPU; no GPU, no Python:
//
//   amdclang++ -std=c++17 -g -O1 -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -I csrc scripts/patch_embed_host_check.cpp -o build/patch_embed_host_check && build/patch_embed_host_check
//
// It walks the shapes of tests/test_patch_embed_gpu.py, ViT-B/16 at batch 256, B = 1, the largest
// sample that fits and the first that does not, and every rejected argument (the image's limits, the other
// tensors' pointers, the forward's row stride and parameter types, the split count), and verifies the geometry's
// invariants: the forward grid covers every token tile and column tile once; every chunk of every
// token of the first and last sample lies inside its sample, 16-byte aligned; the token ranges of the
// weight gradient are whole steps, cover [0, M) and none is empty; and the loaders' division-free
// walks (the forward's chunk walk, the weight gradient's token walk) land where the divisions say.
// Exit status 0 and "ok" when all hold.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "kernels/patch_embed_host.h"

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
  int H, W, C, p, D;
};

alignas(16) static unsigned char image[64];

static void walk(const Shape& s, int want_splits) {
  for (const char* e : {"patch_embed_fwd", "patch_embed_wgrad"}) patch_check(e, image, true, s.B, s.H, s.W, s.C, s.p, s.D);
  patch_check("patch_weight_pack", nullptr, false, 0, 0, 0, s.C, s.p, s.D);
  const PatchGeometry g = patch_geometry(s.B, s.H, s.W, s.C, s.p, s.D, want_splits);
  EXPECT(g.n == (s.H / s.p) * (s.W / s.p) && g.M == s.B * g.n);
  EXPECT(g.cpr * 8 == s.p * s.C && g.kp == g.cpr * 8 * s.p && g.kp % kPeFwdK == 0 && g.kp % kPeWgK == 0);
  EXPECT(g.sample * 2 < (1LL << 31) && g.sample % 8 == 0 && g.row_pitch % 8 == 0 && g.patch_pitch % 8 == 0);
  // forward: tiles
  const int64_t mt = (g.M + kPeFwdTok - 1) / kPeFwdTok;
  EXPECT(g.fwd_grid == mt * (s.D / kPeFwdDim) && mt * kPeFwdTok >= g.M && (mt - 1) * kPeFwdTok < g.M);
  // every chunk of the first and the last token of a sample: inside the sample, and the forward's walk
  // (4 chunks per step from chunk kc, compare-and-wrap) agrees with q / cpr, q % cpr
  for (int tk : {0, g.n - 1}) {
    const int pi = tk / g.gw, pj = tk % g.gw;
    const int64_t base = static_cast<int64_t>(pi) * s.p * g.row_pitch + static_cast<int64_t>(pj) * g.patch_pitch;
    for (int kc = 0; kc < 4; ++kc) {
      int qr = kc, qoff = 0;
      while (qr >= g.cpr) qr -= g.cpr, qoff += g.row_pitch;
      for (int step = 0; step < g.kp / kPeFwdK; ++step) {
        const int q = 4 * step + kc;
        EXPECT(qr == q % g.cpr && qoff == (q / g.cpr) * g.row_pitch);
        const int64_t off = base + qoff + qr * 8;
        EXPECT(off >= 0 && off + 8 <= g.sample && off % 8 == 0);
        qr += 4;
        while (qr >= g.cpr) qr -= g.cpr, qoff += g.row_pitch;
      }
    }
  }
  // weight gradient: the ranges
  EXPECT(g.splits >= 1 && g.splits <= (want_splits < 1 ? 1 : want_splits) && g.splits <= kPeMaxSplits);
  EXPECT(g.split_tokens % kPeWgTok == 0 && g.split_tokens * g.splits >= g.M && g.split_tokens * (g.splits - 1) < g.M);
  EXPECT(patch_wgrad_splits(g.M, g.splits) == g.splits);  // what the entry requires of its caller
  EXPECT(g.step_b * g.n + g.step_pi * g.gw + g.step_pj == kPeWgTok && g.step_pj < g.gw && g.step_pi < g.gh);
  // the token walk of a lane from the start of each range (a few ranges, at most 4096 steps each)
  for (int z : {0, g.splits / 2, g.splits - 1}) {
    for (int tg : {0, 7, 15}) {
      int64_t m = z * g.split_tokens + 4 * tg;
      if (m >= g.M) continue;
      int b = static_cast<int>(m / g.n), pi = static_cast<int>(m % g.n) / g.gw, pj = static_cast<int>(m % g.n) % g.gw;
      for (int step = 0; step < 4096 && m < g.M; ++step) {
        int bb = b, ii = pi, jj = pj;  // the lane's 4 tokens
        for (int u = 0; u < 4 && m + u < g.M; ++u) {
          const int64_t mm = m + u;
          EXPECT(bb == mm / g.n && ii == (mm % g.n) / g.gw && jj == (mm % g.n) % g.gw);
          if (++jj == g.gw) {
            jj = 0;
            if (++ii == g.gh) ii = 0, ++bb;
          }
        }
        m += kPeWgTok;
        pj += g.step_pj;
        if (pj >= g.gw) pj -= g.gw, ++pi;
        pi += g.step_pi;
        if (pi >= g.gh) pi -= g.gh, ++b;
        b += g.step_b;
      }
    }
  }
}

template <typename F> static void rejects(const char* what, F&& f) {
  try {
    f();
  } catch (const std::runtime_error& e) {
    if (std::string(e.what()).rfind("patch_", 0) != 0) {
      std::fprintf(stderr, "the error does not name its entry: %s\n", e.what());
      ++failures;
    }
    return;
  }
  std::fprintf(stderr, "not rejected: %s\n", what);
  ++failures;
}

int main() {
  std::vector<Shape> shapes;
  for (int C : {3, 4})
    for (int p : {16, 8})
      for (int D : {64, 192})
        for (int64_t B : {1, 3, 43}) shapes.push_back({B, 2 * p, 3 * p, C, p, D});
  for (int C : {3, 4}) {
    shapes.push_back({256, 224, 224, C, 16, 768});
    shapes.push_back({1, 224, 224, C, 16, 768});
    shapes.push_back({5, 32, 32, C, 8, 64});
    shapes.push_back({7, 4, 8, 4, 4, 64});  // cpr = 2: the chunk walk wraps twice per step
  }
  // the largest sample that fits (H W C 2 < 2^31) and the first that does not
  const int side = 16 * 1024;
  shapes.push_back({1, side, side - 16, 4, 16, 64});
  for (const Shape& s : shapes)
    for (int want : {0, 1, 5, 8, 1 << 20}) walk(s, want);
  rejects("first sample too large", [&] { patch_check("patch_embed_fwd", image, true, 1, side, side, 4, 16, 64); });
  patch_check("patch_embed_fwd", image, true, 1, 16368, 21840, 3, 16, 64);  // 2^31 - 2752 bytes at C = 3
  rejects("too large at C = 3", [&] { patch_check("patch_embed_fwd", image, true, 1, 16384, 21856, 3, 16, 64); });

  const auto chk = [&](int64_t B, int H, int W, int C, int p, int D, const void* x = image) {
    patch_check("patch_embed_wgrad", x, true, B, H, W, C, p, D);
  };
  chk(3, 32, 48, 3, 16, 64);
  rejects("channels 2", [&] { chk(3, 32, 48, 2, 16, 64); });
  rejects("channels 5", [&] { chk(3, 32, 48, 5, 16, 64); });
  rejects("p = 14 at C = 3", [&] { chk(3, 28, 42, 3, 14, 64); });
  rejects("p = 2 at C = 4 (K' = 16)", [&] { chk(3, 32, 48, 4, 2, 64); });
  rejects("p = 0", [&] { chk(3, 32, 48, 4, 0, 64); });
  rejects("p = 1024", [&] { chk(1, 1024, 1024, 4, 1024, 64); });
  rejects("H % p", [&] { chk(3, 40, 48, 3, 16, 64); });
  rejects("W % p", [&] { chk(3, 32, 40, 3, 16, 64); });
  rejects("H < p", [&] { chk(3, 0, 48, 3, 16, 64); });
  rejects("D = 96", [&] { chk(3, 32, 48, 3, 16, 96); });
  rejects("D = 0", [&] { chk(3, 32, 48, 3, 16, 0); });
  rejects("empty batch", [&] { chk(0, 32, 48, 3, 16, 64); });
  rejects("negative batch", [&] { chk(-1, 32, 48, 3, 16, 64); });
  rejects("null image", [&] { chk(3, 32, 48, 3, 16, 64, nullptr); });
  rejects("unaligned image", [&] { chk(3, 32, 48, 3, 16, 64, image + 2); });
  rejects("too many tokens", [&] { chk((1LL << 31) / 7, 32, 48, 3, 16, 64); });
  chk(((1LL << 31) - 1024) / 7, 32, 48, 3, 16, 64);
  rejects("no tokens", [&] { patch_wgrad_splits(0, 4); });
  // the other tensors, the forward's stride and types, the weight gradient's split count
  patch_need16("patch_embed_fwd", {image, image + 16});
  rejects("null tensor", [&] { patch_need16("patch_embed_fwd", {image, nullptr}); });
  rejects("unaligned tensor", [&] { patch_need16("patch_embed_wgrad", {image, image + 8}); });
  for (int bt : {7, 9})
    for (int ct : {7, 9})
      for (int pt : {7, 9}) patch_fwd_check(64, 72, bt, ct, pt);
  patch_fwd_check(192, 192, 9, 9, 9);
  rejects("row stride below D", [&] { patch_fwd_check(192, 184, 9, 9, 9); });
  rejects("row stride % 8", [&] { patch_fwd_check(64, 68, 9, 9, 9); });
  rejects("fp16 bias", [&] { patch_fwd_check(64, 64, 6, 9, 9); });
  rejects("fp16 cls", [&] { patch_fwd_check(64, 64, 9, 6, 9); });
  rejects("fp64 pos", [&] { patch_fwd_check(64, 64, 9, 9, 8); });
  patch_wgrad_check(258, 5);
  patch_wgrad_check(258, 1);
  rejects("a split count that leaves empty ranges", [&] { patch_wgrad_check(258, 6); });
  rejects("zero splits", [&] { patch_wgrad_check(258, 0); });
  rejects("pack: D", [&] { patch_check("patch_weight_pack", nullptr, false, 0, 0, 0, 3, 16, 100); });

  if (failures != 0) {
    std::fprintf(stderr, "%d check(s) failed\n", failures);
    return 1;
  }
  std::printf("patch_embed_host_check: ok (%zu shapes)\n", shapes.size());
  return 0;
}
