// ViT patch embedding as an implicit GEMM on the NHWC bf16 batch — gfx950.
//
// The projection of non-overlapping p x p patches is a convolution with stride = kernel size: in NHWC
// every 8-element K chunk of a token is 16 contiguous, 16-byte-aligned bytes of the image (K order
// k' = (i, j, c), a patch row = p C elements = cpr chunks), so the A operand is read from the image
// itself, with 3 or 4 channels, and no patch matrix exists in either direction. Three entries:
//
// patch_weight_pack: the parameter [D][3 p p] in (c, i, j) order -> Wp [D][p][p][C] in (i, j, c)
//   order, channel 3 (C = 4) zero. A lane gathers 8 elements and stores 16 B.
//
// patch_embed_fwd: out[b, 1 + t, :] = bf16(A . Wp^T + bias + pos[1 + t]), out[b, 0, :] = bf16(cls + pos[0]).
//   * Split: a workgroup of 4 waves owns 256 tokens x 64 columns, all of K; the grid is not
//     persistent (a tile is 24-32 steps long, the launch has 2352 of them at ViT-B/16, batch 256), and
//     the D / 64 column tiles of one token tile are adjacent workgroups, so that the image tile is
//     fetched from HBM once and the other column tiles find it in L2. 64 columns because D % 64 == 0
//     is the limit; the token side carries the tile's size instead (Wp is 1.2-1.5 MB and L2-resident).
//   * Data movement: register staging, two LDS stages of [256 + 64][32 + 8] bf16 (50 KiB). Per step
//     a lane loads 4 image chunks + 1 Wp chunk (16 B each) for step s + 1 before the MFMAs of step s
//     and writes them to the other stage after them: one barrier per step. The + 8 elements of row
//     padding keep ds_read_b128 of 16 rows off each other's banks. LDS-DMA was not used: its
//     4-byte-per-lane form would need 4x the load instructions for the same bytes, and the image side
//     is a gather (a token's chunk address has no common stride across the tile's rows).
//   * Addresses: per row a 64-bit pointer to the token's first pixel (formed once per tile), plus one
//     32-bit chunk offset per lane that steps with compare-and-wrap: (q % cpr, q / cpr) advance by 4
//     chunks per step. No division in the loop. Rows past M re-read token M - 1 and are never stored.
//   * MFMA: v_mfma_f32_16x16x32_bf16, A operand = Wp rows (columns of the output), B operand =
//     tokens; a wave owns 64 tokens x 64 columns = 4 x 4 tiles, 64 accumulator VGPRs. Wp rows are
//     assigned to A-operand rows so that a lane's results of the tile pair (2 jj, 2 jj + 1) are 8
//     CONSECUTIVE columns of one token: the epilogue adds bias and pos in fp32, rounds once and
//     stores 16 B from registers, with no staging tile.
//   * The [CLS] row of sample b is written by the workgroups that own token (b, 0), 64 columns each.
//
// patch_embed_wgrad: ws[s][d][(c, i, j)] = sum over the tokens of range s of dY[b, 1 + t, d] A[m][k'].
//   * Both operands have the reduction index (the token) as their slow index, so both are transposed
//     on the way to LDS: a lane loads the same 8 columns of 4 consecutive tokens (4 x 16 B), transposes
//     4 x 8 in registers and writes 8 x 8 B to the [column][token] tiles; waves 0-1 stage dY, waves 2-3
//     the image. dY is read in place (row m + m / n + 1: the [CLS] rows are skipped by address).
//   * Split: 64 x 64 of dW' per workgroup, 64 tokens per step, split-K over token ranges (grid z); each
//     wave owns 32 x 32. Small tiles: D % 64 and K' % 64 are the limits, the accumulators are 16 VGPRs,
//     and several workgroups share a CU. Tokens advance per step by a host-made (sample, patch row,
//     patch column) decomposition of 64 with compare-and-wrap; tokens past the range are zeros in LDS.
//   * A operand = dY^T (4 consecutive d per lane), B operand = image^T (16 consecutive k' across the
//     lanes): a slab is stored as fp32 directly in the parameter's (d, c, i, j) order, channel 3
//     dropped; gemm_splitk_reduce sums the slabs.
//
// Not tuned: tile sizes and split count were chosen by the arithmetic above, not by a sweep; see
// profiles/patch_embed_vit_b16.jsonl for what was measured.
#include <stdexcept>
#include <string>

#include "../api.h"
#include "c3_frag.h"
#include "common.h"
#include "patch_embed_host.h"

namespace fluxmpi {
namespace {

constexpr int kLdF = kPeFwdK + 8;    // forward LDS row stride (elements)
constexpr int kLdW = kPeWgTok + 8;   // weight-gradient LDS row stride (elements)

// ---------------------------------------------------------------------------------------- pack
template <int C>
__global__ __launch_bounds__(256) void patch_weight_pack_kernel(const bf16* __restrict__ w, bf16* __restrict__ wp,
                                                                int D, int pp) {
  const int kp = pp * C, kw = 3 * pp;
  const int64_t v = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;  // one 8-element vector of Wp
  if (v >= static_cast<int64_t>(D) * (kp / 8)) return;
  const int d = static_cast<int>(v / (kp / 8)), k0 = static_cast<int>(v % (kp / 8)) * 8;
  const bf16* row = w + static_cast<int64_t>(d) * kw;
  bf16x8 o;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int k = k0 + e, c = k % C, ij = k / C;
    o[e] = c < 3 ? row[c * pp + ij] : static_cast<bf16>(0.f);
  }
  *reinterpret_cast<bf16x8*>(wp + static_cast<int64_t>(d) * kp + k0) = o;
}

// ---------------------------------------------------------------------------------------- forward
struct FwdArgs {
  const bf16* x;     // [B][H][W][C]
  const bf16* wp;    // [D][K']
  const void* bias;  // [D]
  const void* cls;   // [D]
  const void* pos;   // [n + 1][D]
  bf16* out;         // [B (n + 1)][ldo]
  int64_t sample, ldo;
  int M, n, gw, D, kp, cpr, row_pitch, patch_pitch, p;
  int bias_f32, cls_f32;  // bias / cls are fp32 (else bf16): a uniform branch; pos' type is the template's
};

template <typename PT>
__device__ __forceinline__ void load8f(const PT* __restrict__ q, float (&f)[8]) {
  PT t[8];
  load8(q, t);
#pragma unroll
  for (int e = 0; e < 8; ++e) f[e] = static_cast<float>(t[e]);
}

// 8 elements of a vector whose type is a kernel argument (bias, cls: D elements each)
__device__ __forceinline__ void load8f_rt(const void* q, int d, bool f32, float (&f)[8]) {
  if (f32) load8f(static_cast<const float*>(q) + d, f);
  else load8f(static_cast<const bf16*>(q) + d, f);
}

template <typename PT>
__global__ __launch_bounds__(kPeThreads) void patch_embed_fwd_kernel(FwdArgs a) {
  __shared__ __attribute__((aligned(16))) bf16 lds[2][(kPeFwdTok + kPeFwdDim) * kLdF];
  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int ntile = a.D / kPeFwdDim;
  const int mt = blockIdx.x / ntile, nt = blockIdx.x - mt * ntile;
  const int m0 = mt * kPeFwdTok, d0 = nt * kPeFwdDim;

  // loader: chunk t & 3 of the step, rows (t >> 2) + 64 u of the token tile and row t >> 2 of Wp's
  const int kc = t & 3, lr = t >> 2;
  const bf16* rowp[4];
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    int m = m0 + lr + 64 * u;
    m = m < a.M ? m : a.M - 1;
    const int b = m / a.n, tk = m - b * a.n;
    const int pi = tk / a.gw, pj = tk - pi * a.gw;
    rowp[u] = a.x + b * a.sample + (pi * a.p * a.row_pitch + pj * a.patch_pitch);
  }
  const bf16* wrow = a.wp + static_cast<int64_t>(d0 + lr) * a.kp + kc * 8;
  int qr = kc, qoff = 0;  // chunk q = 4 step + kc as (q % cpr, (q / cpr) image rows in elements)
  while (qr >= a.cpr) qr -= a.cpr, qoff += a.row_pitch;

  bf16x8 ra[4], rw;
  auto issue = [&](int step) {
    const int off = qoff + qr * 8;
#pragma unroll
    for (int u = 0; u < 4; ++u) ra[u] = *reinterpret_cast<const bf16x8*>(rowp[u] + off);
    rw = *reinterpret_cast<const bf16x8*>(wrow + step * kPeFwdK);
    qr += 4;
    while (qr >= a.cpr) qr -= a.cpr, qoff += a.row_pitch;
  };
  auto commit = [&](int stage) {
    bf16* s = lds[stage];
#pragma unroll
    for (int u = 0; u < 4; ++u) *reinterpret_cast<bf16x8*>(s + (lr + 64 * u) * kLdF + kc * 8) = ra[u];
    *reinterpret_cast<bf16x8*>(s + (kPeFwdTok + lr) * kLdF + kc * 8) = rw;
  };

  f32x4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int li = lane & 15, g = lane >> 4;
  // A-operand row li of tile j is Wp row 32 (j >> 1) + 8 (li >> 2) + 4 (j & 1) + (li & 3): see the header
  const int wofs = (kPeFwdTok + 8 * (li >> 2) + (li & 3)) * kLdF + 8 * g;
  const int tofs = (64 * wave + li) * kLdF + 8 * g;

  const int steps = a.kp / kPeFwdK;
  issue(0);
  commit(0);
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    if (s + 1 < steps) issue(s + 1);
    const bf16* cur = lds[s & 1];
    bf16x8 fw[4], ft[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
      fw[j] = *reinterpret_cast<const bf16x8*>(cur + wofs + (32 * (j >> 1) + 4 * (j & 1)) * kLdF);
#pragma unroll
    for (int i = 0; i < 4; ++i) ft[i] = *reinterpret_cast<const bf16x8*>(cur + tofs + 16 * i * kLdF);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[j], ft[i], acc[i][j], 0, 0, 0);
    if (s + 1 < steps) commit((s + 1) & 1);
    __syncthreads();
  }

  // acc[i][j][r] = token m0 + 64 wave + 16 i + li, column d0 + 32 (j >> 1) + 8 g + 4 (j & 1) + r
  const PT* pos = static_cast<const PT*>(a.pos);
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int m = m0 + 64 * wave + 16 * i + li;
    if (m >= a.M) continue;
    const int b = m / a.n, tk = m - b * a.n;
    bf16* orow = a.out + (static_cast<int64_t>(b) * (a.n + 1) + 1 + tk) * a.ldo;
    const PT* prow = pos + static_cast<int64_t>(1 + tk) * a.D;
#pragma unroll
    for (int jj = 0; jj < 2; ++jj) {
      const int d = d0 + 32 * jj + 8 * g;
      float fb[8], fp[8];
      load8f_rt(a.bias, d, a.bias_f32 != 0, fb);
      load8f(prow + d, fp);
      bf16x8 o;
#pragma unroll
      for (int e = 0; e < 8; ++e) o[e] = static_cast<bf16>(acc[i][2 * jj + (e >> 2)][e & 3] + fb[e] + fp[e]);
      *reinterpret_cast<bf16x8*>(orow + d) = o;
    }
  }
  // the [CLS] rows of the samples that start in this tile
  {
    const int m = m0 + t;
    if (m < a.M) {
      const int b = m / a.n;
      if (m - b * a.n == 0) {
        bf16* orow = a.out + static_cast<int64_t>(b) * (a.n + 1) * a.ldo;
#pragma unroll
        for (int d = d0; d < d0 + kPeFwdDim; d += 8) {
          float fc[8], fp[8];
          load8f_rt(a.cls, d, a.cls_f32 != 0, fc);
          load8f(pos + d, fp);
          bf16x8 o;
#pragma unroll
          for (int e = 0; e < 8; ++e) o[e] = static_cast<bf16>(fc[e] + fp[e]);
          *reinterpret_cast<bf16x8*>(orow + d) = o;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------- weight gradient
struct WgArgs {
  const bf16* x;   // [B][H][W][C]
  const bf16* dy;  // [B (n + 1)][D]
  float* ws;       // [splits][D][3 p p]
  int64_t sample, split_tokens;
  int M, n, gh, gw, D, kp, kw, cpr, row_pitch, patch_pitch, p, C, pp;
  int step_b, step_pi, step_pj;
};

// 4 rows x 8 columns of bf16 (one uint4 per row) -> per column the 4 rows, 8 B
__device__ __forceinline__ uint2 column4(const uint4 (&r)[4], int c) {
  const auto word = [&](const uint4& v) { return (c >> 1) == 0 ? v.x : (c >> 1) == 1 ? v.y : (c >> 1) == 2 ? v.z : v.w; };
  const unsigned w0 = word(r[0]), w1 = word(r[1]), w2 = word(r[2]), w3 = word(r[3]);
  if (c & 1) return uint2{(w0 >> 16) | (w1 & 0xffff0000u), (w2 >> 16) | (w3 & 0xffff0000u)};
  return uint2{(w0 & 0xffffu) | (w1 << 16), (w2 & 0xffffu) | (w3 << 16)};
}

__global__ __launch_bounds__(kPeThreads) void patch_embed_wgrad_kernel(WgArgs a) {
  // per stage: dY^T [64 d][64 tokens + 8], then image^T [64 k'][64 tokens + 8]
  __shared__ __attribute__((aligned(16))) bf16 lds[2][(kPeWgDim + kPeWgK) * kLdW];
  const int t = threadIdx.x;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6), lane = t & 63;
  const int d0 = blockIdx.x * kPeWgDim, k0 = blockIdx.y * kPeWgK;
  const int64_t mbeg64 = static_cast<int64_t>(blockIdx.z) * a.split_tokens;
  const int mbeg = static_cast<int>(mbeg64 < a.M ? mbeg64 : a.M);
  const int mend = static_cast<int>(mbeg64 + a.split_tokens < a.M ? mbeg64 + a.split_tokens : a.M);

  // loader: waves 0-1 dY, waves 2-3 the image; tokens 4 tg .. + 3 of the step, columns 8 cg .. + 7
  const bool img = wave >= 2;
  const int l = t & 127, tg = l & 15, cg = l >> 4;
  // this lane's column offset (elements): into a dY row, or into a token's patch
  int coff;
  if (img) {
    const int q = (k0 >> 3) + cg;
    coff = (q / a.cpr) * a.row_pitch + (q % a.cpr) * 8;
  } else {
    coff = d0 + cg * 8;
  }
  // the first of this lane's tokens in step 0, as (sample, patch row, patch column)
  int m = mbeg + 4 * tg;
  int tb, tpi, tpj;
  {
    const int mm = m < a.M ? m : 0;  // (past the end: any valid start; its loads are masked off)
    tb = mm / a.n;
    const int tk = mm - tb * a.n;
    tpi = tk / a.gw, tpj = tk - tpi * a.gw;
  }

  uint4 r[4];
  auto issue = [&]() {
    int b = tb, pi = tpi, pj = tpj;
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      r[u] = uint4{0u, 0u, 0u, 0u};
      if (m + u < mend) {
        const bf16* src = img ? a.x + b * a.sample + (pi * a.p * a.row_pitch + pj * a.patch_pitch + coff)
                              : a.dy + (static_cast<int64_t>(b) * (a.n + 1) + 1 + pi * a.gw + pj) * a.D + coff;
        r[u] = *reinterpret_cast<const uint4*>(src);
      }
      if (++pj == a.gw) {
        pj = 0;
        if (++pi == a.gh) pi = 0, ++b;
      }
    }
    // the step's advance of 64 tokens
    m += kPeWgTok;
    tpj += a.step_pj;
    if (tpj >= a.gw) tpj -= a.gw, ++tpi;
    tpi += a.step_pi;
    if (tpi >= a.gh) tpi -= a.gh, ++tb;
    tb += a.step_b;
  };
  auto commit = [&](int stage) {
    bf16* s = lds[stage] + ((img ? kPeWgDim : 0) + 8 * cg) * kLdW + 4 * tg;
#pragma unroll
    for (int c = 0; c < 8; ++c) *reinterpret_cast<uint2*>(s + c * kLdW) = column4(r, c);
  };

  f32x4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int li = lane & 15, g = lane >> 4;
  const int wd = wave & 1, wk = wave >> 1;
  const int aofs = (32 * wd + li) * kLdW + 8 * g;
  const int bofs = (kPeWgDim + 32 * wk + li) * kLdW + 8 * g;

  const int steps = (mend - mbeg + kPeWgTok - 1) / kPeWgTok;
  if (steps > 0) {
    issue();
    commit(0);
  }
  __syncthreads();
  for (int s = 0; s < steps; ++s) {
    if (s + 1 < steps) issue();
    const bf16* cur = lds[s & 1];
#pragma unroll
    for (int kk = 0; kk < kPeWgTok / 32; ++kk) {
      bf16x8 fa[2], fb[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) fa[i] = *reinterpret_cast<const bf16x8*>(cur + aofs + 16 * i * kLdW + 32 * kk);
#pragma unroll
      for (int j = 0; j < 2; ++j) fb[j] = *reinterpret_cast<const bf16x8*>(cur + bofs + 16 * j * kLdW + 32 * kk);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
          acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
    }
    if (s + 1 < steps) commit((s + 1) & 1);
    __syncthreads();
  }

  // acc[i][j][r] = dW'[d0 + 32 wd + 16 i + 4 g + r][k0 + 32 wk + 16 j + li] -> (d, c, i, j) order
  float* slab = a.ws + static_cast<int64_t>(blockIdx.z) * a.D * a.kw;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int k = k0 + 32 * wk + 16 * j + li;
    const int ij = a.C == 4 ? k >> 2 : k / 3;
    const int c = k - ij * a.C;
    if (c >= 3) continue;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int rr = 0; rr < 4; ++rr)
        slab[static_cast<int64_t>(d0 + 32 * wd + 16 * i + 4 * g + rr) * a.kw + c * a.pp + ij] = acc[i][j][rr];
  }
}

}  // namespace

void patch_weight_pack(const void* w, void* wp, int D, int p, int C, hipStream_t stream) {
  patch_check("patch_weight_pack", nullptr, false, 0, 0, 0, C, p, D);
  patch_need16("patch_weight_pack", {w, wp});
  const int64_t vecs = static_cast<int64_t>(D) * (p * p * C / 8);
  const unsigned grid = static_cast<unsigned>((vecs + 255) / 256);
  const bf16* src = static_cast<const bf16*>(w);
  bf16* dst = static_cast<bf16*>(wp);
  if (C == 3) patch_weight_pack_kernel<3><<<grid, 256, 0, stream>>>(src, dst, D, p * p);
  else patch_weight_pack_kernel<4><<<grid, 256, 0, stream>>>(src, dst, D, p * p);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

void patch_embed_fwd(const void* x, const void* wp, const void* bias, const void* cls, const void* pos, void* out,
                     int64_t B, int H, int W, int C, int p, int D, int64_t ldo, int bias_dtype, int cls_dtype, int pos_dtype,
                     hipStream_t stream) {
  patch_check("patch_embed_fwd", x, true, B, H, W, C, p, D);
  patch_need16("patch_embed_fwd", {wp, bias, cls, pos, static_cast<const void*>(out)});
  patch_fwd_check(D, ldo, bias_dtype, cls_dtype, pos_dtype);
  const PatchGeometry g = patch_geometry(B, H, W, C, p, D, 1);
  const FwdArgs a{static_cast<const bf16*>(x), static_cast<const bf16*>(wp), bias, cls, pos, static_cast<bf16*>(out),
                  g.sample, ldo, static_cast<int>(g.M), g.n, g.gw, D, g.kp, g.cpr, g.row_pitch, g.patch_pitch, p,
                  bias_dtype == static_cast<int>(kF32), cls_dtype == static_cast<int>(kF32)};
  const unsigned grid = static_cast<unsigned>(g.fwd_grid);
  if (pos_dtype == static_cast<int>(kBF16)) patch_embed_fwd_kernel<bf16><<<grid, kPeThreads, 0, stream>>>(a);
  else patch_embed_fwd_kernel<float><<<grid, kPeThreads, 0, stream>>>(a);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

int patch_embed_wgrad_splits(int64_t M, int splits) { return patch_wgrad_splits(M, splits); }

void patch_embed_wgrad(const void* x, const void* dy, float* ws, int64_t B, int H, int W, int C, int p, int D, int splits,
                       hipStream_t stream) {
  patch_check("patch_embed_wgrad", x, true, B, H, W, C, p, D);
  patch_need16("patch_embed_wgrad", {dy, static_cast<const void*>(ws)});
  const PatchGeometry g = patch_geometry(B, H, W, C, p, D, splits);
  patch_wgrad_check(g.M, splits);
  const WgArgs a{static_cast<const bf16*>(x), static_cast<const bf16*>(dy), ws, g.sample, g.split_tokens,
                 static_cast<int>(g.M), g.n, g.gh, g.gw, D, g.kp, g.kw, g.cpr, g.row_pitch, g.patch_pitch, p, C, p * p,
                 g.step_b, g.step_pi, g.step_pj};
  const dim3 grid(D / kPeWgDim, g.kp / kPeWgK, g.splits);
  patch_embed_wgrad_kernel<<<grid, kPeThreads, 0, stream>>>(a);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace fluxmpi
