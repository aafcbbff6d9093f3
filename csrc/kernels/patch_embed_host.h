// Host side of the patch-embedding entries (patch_embed.hip) without the launches: the argument
// checks and the launch geometry, plain C++ so that a stand-alone program can walk them under a
// sanitizer (scripts/patch_embed_host_check.cpp).
//
// Geometry. The image is NHWC bf16 [B][H][W][C], cut into gh x gw patches of p x p pixels; token
// m = (b, pi, pj), n = gh gw tokens per sample, M = B n. The K axis of the implicit GEMM is
// k' = (i, j, c): a patch row is p C contiguous elements = cpr 16-byte chunks, chunk q of a token
// lies (q / cpr) image rows down and (q % cpr) chunks along. All offsets inside a sample are below
// 2^30 elements (a sample is below 2^31 bytes); the sample's base is 64-bit.
//   forward: a workgroup owns kPeFwdTok tokens x kPeFwdDim output columns, the grid is
//            (D / kPeFwdDim) x ceil(M / kPeFwdTok) with the column tiles of one token tile adjacent;
//   weight gradient: a workgroup owns kPeWgDim x kPeWgK of dW' and one of `splits` token ranges of
//            split_tokens tokens (a multiple of the kPeWgTok tokens of a step; no range is empty).
//            A step's advance of kPeWgTok tokens is (step_b, step_pi, step_pj) in (sample, patch row,
//            patch column), so the loader walks tokens with compare-and-wrap, without a division.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#include <stdexcept>
#include <string>

namespace fluxmpi {

constexpr int kPeThreads = 256;
constexpr int kPeFwdTok = 256;  // forward tile: tokens
constexpr int kPeFwdDim = 64;   // forward tile: output columns
constexpr int kPeFwdK = 32;     // forward: K elements per step (4 chunks)
constexpr int kPeWgDim = 64;    // weight gradient tile: rows of dW' (d)
constexpr int kPeWgK = 64;      // weight gradient tile: columns of dW' (k')
constexpr int kPeWgTok = 64;    // weight gradient: tokens per step
constexpr int kPeMaxSplits = 1024;

struct PatchGeometry {
  int gh, gw, n;      // patch grid, tokens per sample
  int cpr;            // 16-byte chunks per patch row
  int kp;             // K' = p p C
  int kw;             // the parameter's row length, 3 p p
  int row_pitch;      // elements per image row, W C
  int patch_pitch;    // elements from a patch to its right neighbour, p C
  int64_t sample;     // elements per sample, H W C
  int64_t M;          // tokens
  int64_t fwd_grid;   // forward workgroups
  int splits;         // weight gradient: token ranges (grid z)
  int64_t split_tokens;
  int step_b, step_pi, step_pj;  // kPeWgTok tokens as sample / patch-row / patch-column steps
};

// The limits every entry shares; `entry` names the caller in the error. `x` may be null where an
// entry has no image (the pack).
inline void patch_check(const char* entry, const void* x, bool has_x, int64_t B, int H, int W, int C, int p, int D) {
  const auto fail = [entry](const std::string& m) { throw std::runtime_error(std::string(entry) + ": " + m); };
  if (C != 3 && C != 4) fail("channels must be 3 or 4");
  if (p < 1 || p > 512) fail("the patch size must lie in 1..512");
  if ((p * C) % 8 != 0) fail("p * C must be a multiple of 8 (a patch row in whole 16-byte chunks)");
  if ((p * p * C) % 64 != 0) fail("p * p * C must be a multiple of 64 (the K tiles)");
  if (D < 64 || D % 64 != 0 || D > (1 << 20)) fail("D must be a positive multiple of 64");
  if (!has_x) return;
  if (B < 1) fail("the batch must not be empty");
  if (H < p || W < p || H % p != 0 || W % p != 0) fail("H and W must be positive multiples of the patch size");
  if (static_cast<int64_t>(H) * W * C * 2 >= (1LL << 31)) fail("one sample must be below 2^31 bytes");
  if (x == nullptr) fail("null image");
  if (reinterpret_cast<uintptr_t>(x) % 16 != 0) fail("the image must be 16-byte aligned");
  const int64_t n = static_cast<int64_t>(H / p) * (W / p);
  if (B > ((1LL << 31) - 1024) / (n + 1)) fail("B * (n + 1) must stay below 2^31 - 1024");
}

// every tensor an entry reads or writes beside the image: not null, 16-byte aligned
inline void patch_need16(const char* entry, std::initializer_list<const void*> ptrs) {
  for (const void* q : ptrs) {
    if (q == nullptr) throw std::runtime_error(std::string(entry) + ": null tensor");
    if (reinterpret_cast<uintptr_t>(q) % 16 != 0)
      throw std::runtime_error(std::string(entry) + ": every tensor must be 16-byte aligned");
  }
}

// the forward's own arguments: the output's row stride, and the types of bias / cls / pos (each bf16 = 9
// or fp32 = 7, the codes of common.h's DType)
inline void patch_fwd_check(int D, int64_t ldo, int bias_dtype, int cls_dtype, int pos_dtype) {
  if (ldo < D || ldo % 8 != 0)
    throw std::runtime_error("patch_embed_fwd: the output's row stride must be >= D and a multiple of 8");
  for (int dt : {bias_dtype, cls_dtype, pos_dtype})
    if (dt != 9 && dt != 7) throw std::runtime_error("patch_embed_fwd: bias, cls and pos are bf16 or fp32");
}

// the token ranges `splits` asks for: ranges of whole steps, none empty
inline int patch_wgrad_splits(int64_t M, int splits) {
  if (M < 1) throw std::runtime_error("patch_embed_wgrad: no tokens");
  if (splits < 1) splits = 1;
  if (splits > kPeMaxSplits) splits = kPeMaxSplits;
  const int64_t per = (M + splits - 1) / splits;
  const int64_t len = (per + kPeWgTok - 1) / kPeWgTok * kPeWgTok;
  return static_cast<int>((M + len - 1) / len);
}

// the weight gradient takes the split count its caller sized the slabs by: it must be the actual one
inline void patch_wgrad_check(int64_t M, int splits) {
  const int actual = patch_wgrad_splits(M, splits);
  if (actual != splits)
    throw std::runtime_error("patch_embed_wgrad: splits must be patch_embed_wgrad_splits(M, splits) = " +
                             std::to_string(actual) + ", got " + std::to_string(splits));
}

inline PatchGeometry patch_geometry(int64_t B, int H, int W, int C, int p, int D, int splits) {
  PatchGeometry g{};
  g.gh = H / p, g.gw = W / p, g.n = g.gh * g.gw;
  g.cpr = p * C / 8;
  g.kp = p * p * C;
  g.kw = 3 * p * p;
  g.row_pitch = W * C;
  g.patch_pitch = p * C;
  g.sample = static_cast<int64_t>(H) * W * C;
  g.M = B * g.n;
  g.fwd_grid = (g.M + kPeFwdTok - 1) / kPeFwdTok * (D / kPeFwdDim);
  if (g.fwd_grid > 0x7fffffffLL) throw std::runtime_error("patch_embed_fwd: too many workgroups for one launch");
  g.splits = patch_wgrad_splits(g.M, splits);
  const int64_t per = (g.M + g.splits - 1) / g.splits;
  g.split_tokens = (per + kPeWgTok - 1) / kPeWgTok * kPeWgTok;
  g.step_b = kPeWgTok / g.n;
  const int rem = kPeWgTok % g.n;
  g.step_pi = rem / g.gw;
  g.step_pj = rem % g.gw;
  return g;
}

}  // namespace fluxmpi
