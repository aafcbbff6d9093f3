// MX (block-scaled) fp8 quantisation of a bf16 matrix — gfx950.
//
// Every 32 consecutive elements along the reduction axis of the GEMM that will read the image share one
// power-of-two scale s = 2^p (mx_host.h has the rule); the elements are cast(clamp(x * s, +-FMAX)) with
// v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32 (round to nearest even, the only rounding), and the block's E8M0 byte
// 127 - p goes to a scale image. A non-finite input is written as the format's non-finite code; its block has
// s = 1 (byte 127). There is no global amax, so ONE launch reads x once and writes the row-wise image
// (blocks along C), the transposed image (blocks along R; its own scales and its own bytes, not the
// transpose of the first), or both. No atomics, no scale block, no state: the result is the same bits in
// every run by construction.
//
// mx_quantize: a workgroup of 256 lanes owns a 128 x 128 tile of x, which is 4 blocks = one scale dword per
// row of the row-wise image and one per column of the transposed one: no two workgroups write the same
// scale dword, and a partial last tile writes the 127 padding of its dwords itself.
//   * Row-wise: in each of 4 passes a lane reads 16 consecutive columns of one row (2 x 16 B; rows past R and
//     columns past C are not read and count as zero). A block is the 2 x 16 columns of lanes 2 i and 2 i + 1:
//     the block amax is the max of the two lanes' integer maxima of the bf16 bit patterns without sign (one
//     cross-lane exchange); p comes from that pattern's exponent field and a "> 1.75" test of its
//     significand, in integers. The lane casts its 16 values and stores 16 B. The four block bytes of the
//     row's 128 columns are ORed together over the row's 8 lanes (two exchanges) and leave as one dword.
//   * Transposed: the passes also put the bf16 tile into LDS ([128 rows][256 B + 16]; the + 16 keeps 16-byte
//     alignment and staggers the banks of the row-wise writes). After one barrier a lane owns two adjacent
//     columns and one 32-row block of them (wave w owns block w): 32 ds_read_b32, each wave reading 256
//     contiguous bytes of one row, then amax, scale and cast per column, and 2 x 16 B stores per column. The
//     block bytes meet in a [128 columns][4] LDS table and leave as one dword per column.
// The cast helpers repeat fp8_quant.hip's (that file's ISA is kept as it is).
#include <stdexcept>
#include <string>

#include "../api.h"
#include "common.h"
#include "mx_host.h"

namespace fluxmpi {
namespace {

constexpr int kLdX = kMxQTile * 2 + 16;  // LDS row stride (bytes) of the bf16 tile

template <int FMT> struct MxFormat;
template <> struct MxFormat<kFp8E4M3> {
  static constexpr float kMax = 448.f;
  static constexpr int kMaxExp = 8;  // FMAX = 1.75 * 2^8
  static __device__ __forceinline__ int pack2(float a, float b, int old, bool hi) {
    return hi ? __builtin_amdgcn_cvt_pk_fp8_f32(a, b, old, true) : __builtin_amdgcn_cvt_pk_fp8_f32(a, b, old, false);
  }
  static __device__ __forceinline__ unsigned nonfinite(unsigned bits) { return ((bits >> 8) & 0x80u) | 0x7Fu; }
};
template <> struct MxFormat<kFp8E5M2> {
  static constexpr float kMax = 57344.f;
  static constexpr int kMaxExp = 15;  // FMAX = 1.75 * 2^15
  static __device__ __forceinline__ int pack2(float a, float b, int old, bool hi) {
    return hi ? __builtin_amdgcn_cvt_pk_bf8_f32(a, b, old, true) : __builtin_amdgcn_cvt_pk_bf8_f32(a, b, old, false);
  }
  static __device__ __forceinline__ unsigned nonfinite(unsigned bits) {
    return ((bits >> 8) & 0x80u) | ((bits & 0x7Fu) != 0 ? 0x7Eu : 0x7Cu);
  }
};

struct MxQuantArgs {
  const uint16_t* x;  // bf16 bits [R][ld]
  uint8_t* q;         // [R][ldq] or null
  uint8_t* s;         // [R][lds]
  uint8_t* qt;        // [C][ldt] or null
  uint8_t* st;        // [C][ldst]
  int64_t ld, ldq, lds, ldt, ldst;
  int R, C, col_tiles;
};

// log2 of the block's scale from its amax (a bf16 bit pattern without sign). The exponent field 0 (zero
// excluded: a subnormal) gives more than 126 and is clamped like every amax below 2^(kMaxExp - 126).
template <int FMT>
__device__ __forceinline__ int scale_log2(unsigned amax) {
  if (amax == 0u || amax >= 0x7f80u) return 0;
  const int p = MxFormat<FMT>::kMaxExp + 127 - static_cast<int>(amax >> 7) - ((amax & 0x7fu) > 0x60u ? 1 : 0);
  return p < -126 ? -126 : (p > 126 ? 126 : p);
}

__device__ __forceinline__ float pow2f(int p) { return __builtin_bit_cast(float, static_cast<unsigned>(127 + p) << 23); }

__device__ __forceinline__ unsigned umax(unsigned a, unsigned b) { return a > b ? a : b; }

// 4 bf16 bit patterns (the low 16 bits of each argument) -> 4 fp8 bytes in one word
template <int FMT>
__device__ __forceinline__ unsigned cast4(unsigned b0, unsigned b1, unsigned b2, unsigned b3, float s) {
  using F = MxFormat<FMT>;
  const unsigned bits[4] = {b0 & 0xffffu, b1 & 0xffffu, b2 & 0xffffu, b3 & 0xffffu};
  float y[4];
  bool bad = false;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    bad |= (bits[e] & 0x7fffu) >= 0x7f80u;
    const float v = __builtin_bit_cast(float, bits[e] << 16) * s;
    y[e] = fminf(fmaxf(v, -F::kMax), F::kMax);
  }
  unsigned out = static_cast<unsigned>(F::pack2(y[0], y[1], 0, false));
  out = static_cast<unsigned>(F::pack2(y[2], y[3], static_cast<int>(out), true));
  if (bad) {  // rare: patch the non-finite inputs' bytes
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if ((bits[e] & 0x7fffu) >= 0x7f80u) out = (out & ~(0xffu << (8 * e))) | (F::nonfinite(bits[e]) << (8 * e));
  }
  return out;
}

// max of the two bf16 magnitudes of a word
__device__ __forceinline__ unsigned mag2(unsigned w) { return umax(w & 0x7fffu, (w >> 16) & 0x7fffu); }

template <int FMT>
__global__ __launch_bounds__(kFp8Threads) void mx_quantize_kernel(MxQuantArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[kMxQTile * kLdX];
  __shared__ uint32_t tscale[kMxQTile];
  const int t = threadIdx.x;
  const int rt = blockIdx.x / a.col_tiles, ct = blockIdx.x - rt * a.col_tiles;
  const int r0 = rt * kMxQTile, c0 = ct * kMxQTile;
  const int lr = t >> 3, lc = (t & 7) * 16;  // this lane's row (of a pass) and first column inside the tile
  const int c = c0 + lc;                     // C % 32 == 0: the lane's 16 columns are inside or outside as a whole

#pragma unroll
  for (int pass = 0; pass < 4; ++pass) {
    const int row = lr + 32 * pass, r = r0 + row;
    const bool inside = r < a.R && c < a.C;
    uint4 v0{0u, 0u, 0u, 0u}, v1{0u, 0u, 0u, 0u};
    if (inside) {
      const uint4* src = reinterpret_cast<const uint4*>(a.x + static_cast<int64_t>(r) * a.ld + c);
      v0 = src[0], v1 = src[1];
    }
    if (a.q != nullptr) {  // (uniform)
      unsigned amax = umax(umax(umax(mag2(v0.x), mag2(v0.y)), umax(mag2(v0.z), mag2(v0.w))),
                           umax(umax(mag2(v1.x), mag2(v1.y)), umax(mag2(v1.z), mag2(v1.w))));
      amax = umax(amax, static_cast<unsigned>(__shfl_xor(static_cast<int>(amax), 1, 64)));
      const int p = scale_log2<FMT>(amax);
      const float s = pow2f(p);
      uint4 o;
      o.x = cast4<FMT>(v0.x, v0.x >> 16, v0.y, v0.y >> 16, s);
      o.y = cast4<FMT>(v0.z, v0.z >> 16, v0.w, v0.w >> 16, s);
      o.z = cast4<FMT>(v1.x, v1.x >> 16, v1.y, v1.y >> 16, s);
      o.w = cast4<FMT>(v1.z, v1.z >> 16, v1.w, v1.w >> 16, s);
      if (inside) *reinterpret_cast<uint4*>(a.q + static_cast<int64_t>(r) * a.ldq + c) = o;
      // the row's four block bytes as one dword (a block past C is all zero: 127, the padding)
      unsigned sw = static_cast<unsigned>(127 - p) << (8 * ((t & 7) >> 1));
      sw |= static_cast<unsigned>(__shfl_xor(static_cast<int>(sw), 2, 64));
      sw |= static_cast<unsigned>(__shfl_xor(static_cast<int>(sw), 4, 64));
      if ((t & 7) == 0 && r < a.R) *reinterpret_cast<uint32_t*>(a.s + static_cast<int64_t>(r) * a.lds + 4 * ct) = sw;
    }
    if (a.qt != nullptr) {  // (uniform)
      uint4* dst = reinterpret_cast<uint4*>(tile + row * kLdX + lc * 2);
      dst[0] = v0, dst[1] = v1;
    }
  }

  if (a.qt != nullptr) {  // (uniform)
    __syncthreads();
    const int cp = t & 63, blk = t >> 6;  // columns 2 cp and 2 cp + 1 of the tile, its rows 32 blk .. + 31
    unsigned w[32];
    unsigned amax0 = 0, amax1 = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      w[i] = *reinterpret_cast<const uint32_t*>(tile + (32 * blk + i) * kLdX + cp * 4);
      amax0 = umax(amax0, w[i] & 0x7fffu), amax1 = umax(amax1, (w[i] >> 16) & 0x7fffu);
    }
    const int p0 = scale_log2<FMT>(amax0), p1 = scale_log2<FMT>(amax1);
    const float s0 = pow2f(p0), s1 = pow2f(p1);
    unsigned o0[8], o1[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      o0[i] = cast4<FMT>(w[4 * i], w[4 * i + 1], w[4 * i + 2], w[4 * i + 3], s0);
      o1[i] = cast4<FMT>(w[4 * i] >> 16, w[4 * i + 1] >> 16, w[4 * i + 2] >> 16, w[4 * i + 3] >> 16, s1);
    }
    // C % 32 == 0 and R % 32 == 0: the column pair and the row block are inside or outside as a whole
    const int col = c0 + 2 * cp, rb = r0 + 32 * blk;
    if (col < a.C && rb < a.R) {
      uint4* d0 = reinterpret_cast<uint4*>(a.qt + static_cast<int64_t>(col) * a.ldt + rb);
      uint4* d1 = reinterpret_cast<uint4*>(a.qt + static_cast<int64_t>(col + 1) * a.ldt + rb);
      d0[0] = uint4{o0[0], o0[1], o0[2], o0[3]}, d0[1] = uint4{o0[4], o0[5], o0[6], o0[7]};
      d1[0] = uint4{o1[0], o1[1], o1[2], o1[3]}, d1[1] = uint4{o1[4], o1[5], o1[6], o1[7]};
    }
    // a block past R is all zero: 127, the padding of the column's dword
    uint8_t* tb = reinterpret_cast<uint8_t*>(tscale);
    tb[(2 * cp) * 4 + blk] = static_cast<uint8_t>(127 - p0);
    tb[(2 * cp + 1) * 4 + blk] = static_cast<uint8_t>(127 - p1);
    __syncthreads();
    if (t < kMxQTile && c0 + t < a.C)
      *reinterpret_cast<uint32_t*>(a.st + static_cast<int64_t>(c0 + t) * a.ldst + 4 * rt) = tscale[t];
  }
}

}  // namespace

void mx_quantize(const void* x, int64_t R, int64_t C, int64_t ld, int fmt, void* q, int64_t ldq, void* s, int64_t lds,
                 void* qt, int64_t ldt, void* st, int64_t ldst, hipStream_t stream) {
  const MxQuantGeometry g = mx_quant_check(x, R, C, ld, fmt, q, ldq, s, lds, qt, ldt, st, ldst);
  if (fmt == kFp8E2M1) return mx4_quantize_launch(x, R, C, ld, q, ldq, s, lds, qt, ldt, st, ldst, g.col_tiles, g.grid, stream);
  if (mx_is_fp6(fmt))
    return mx6_quantize_launch(x, R, C, ld, fmt, q, ldq, s, lds, qt, ldt, st, ldst, g.col_tiles, g.grid, stream);
  const MxQuantArgs a{static_cast<const uint16_t*>(x), static_cast<uint8_t*>(q), static_cast<uint8_t*>(s),
                      static_cast<uint8_t*>(qt), static_cast<uint8_t*>(st), ld, ldq, lds, ldt, ldst,
                      static_cast<int>(R), static_cast<int>(C), static_cast<int>(g.col_tiles)};
  const unsigned grid = static_cast<unsigned>(g.grid);
  if (fmt == kFp8E4M3) mx_quantize_kernel<kFp8E4M3><<<grid, kFp8Threads, 0, stream>>>(a);
  else mx_quantize_kernel<kFp8E5M2><<<grid, kFp8Threads, 0, stream>>>(a);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace fluxmpi
