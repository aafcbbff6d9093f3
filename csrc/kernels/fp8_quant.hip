// Per-tensor power-of-two fp8 quantisation of a bf16 matrix — gfx950.
//
// q = cast(clamp(x * s, -FMAX, FMAX)) with s = 2^p read from the tensor's device scale block (fp8_host.h:
// {scale, 1 / scale, amax bits, consumed amax, ...}), so scaling and unscaling are exact and the cast
// (v_cvt_pk_fp8_f32 / v_cvt_pk_bf8_f32, round to nearest even) is the only rounding. A non-finite INPUT is
// written as the format's non-finite code (e4m3: NaN; e5m2: inf for inf, NaN for NaN) whatever the scale;
// a finite input whose product overflows saturates (a stale scale under delayed scaling is safe).
//
// fp8_quantize: a workgroup of 256 lanes owns a 64 x 64 tile of x.
//   * A lane reads 16 consecutive columns of one row (2 x 16 B), converts them in registers and stores the
//     row-major image as 16 B. Rows past R and columns past C read as zero; C % 8 == 0, and the row-major
//     image's rows are written up to C rounded up to 16 with zeros, as the transposed image's are (a GEMM
//     whose K is not a multiple of 16 reads the padding of both operands).
//   * The transposed image [C][R'] (R' = R rounded up to 16, the padding zero) goes through an LDS tile of
//     [64 columns][64 rows + 16] bytes: every lane writes its 16 bytes down one LDS column, and after one
//     barrier reads 16 consecutive rows of one column back as 16 B and stores them: both images leave in
//     16-byte stores. The + 16 keeps the rows 16-byte aligned and moves consecutive columns to other banks.
//   * amax: the bf16 bit pattern without its sign orders |x| as an integer, with inf and NaN above every
//     finite value; max over the lane's 16 elements, over the wave by lane shuffles, over the 4 waves through
//     LDS, then ONE integer atomicMax per workgroup on the block's amax word (as fp32 bits). An integer max
//     is independent of the order, so the result is the same bits in every run: the one atomic this tree
//     allows itself. With both outputs null the launch is the amax pass alone.
//
// fp8_scale_update: one thread, as adam_advance and loss_scale_update. scale = 2^floor(log2(FMAX / amax))
//   with the exponent kept in -126 .. 126 (scale and inverse both normal fp32), 1 when amax is 0 or not
//   finite; stores the exact inverse, moves amax to the "consumed" word and clears it.
//
// Nothing is read back to the host; every launch is HIP-graph capturable.
#include <stdexcept>
#include <string>

#include "../api.h"
#include "common.h"
#include "fp8_host.h"

namespace fluxmpi {
namespace {

constexpr int kLdT = kFp8QTile + 16;  // LDS row stride (bytes) of the transposed tile

template <int FMT> struct Fp8Format;
template <> struct Fp8Format<kFp8E4M3> {
  static constexpr float kMax = 448.f;
  static constexpr int kMaxExp = 8;  // FMAX = 1.75 * 2^8
  static __device__ __forceinline__ int pack2(float a, float b, int old, bool hi) {
    return hi ? __builtin_amdgcn_cvt_pk_fp8_f32(a, b, old, true) : __builtin_amdgcn_cvt_pk_fp8_f32(a, b, old, false);
  }
  static __device__ __forceinline__ unsigned nonfinite(unsigned bits) { return ((bits >> 8) & 0x80u) | 0x7Fu; }
};
template <> struct Fp8Format<kFp8E5M2> {
  static constexpr float kMax = 57344.f;
  static constexpr int kMaxExp = 15;  // FMAX = 1.75 * 2^15
  static __device__ __forceinline__ int pack2(float a, float b, int old, bool hi) {
    return hi ? __builtin_amdgcn_cvt_pk_bf8_f32(a, b, old, true) : __builtin_amdgcn_cvt_pk_bf8_f32(a, b, old, false);
  }
  // inf (no significand bits) -> inf, NaN -> NaN
  static __device__ __forceinline__ unsigned nonfinite(unsigned bits) {
    return ((bits >> 8) & 0x80u) | ((bits & 0x7Fu) != 0 ? 0x7Eu : 0x7Cu);
  }
};

struct QuantArgs {
  const uint16_t* x;  // bf16 bits [R][ld]
  uint8_t* q;         // [R][ldq] or null
  uint8_t* qt;        // [C][ldt] or null
  uint32_t* block;
  int64_t ld, ldq, ldt;
  int R, C, rpad, col_tiles, want_amax;
};

// 4 bf16 bit patterns (two words) -> 4 fp8 bytes in one word
template <int FMT>
__device__ __forceinline__ unsigned quant4(unsigned w0, unsigned w1, float s, unsigned& amax) {
  using F = Fp8Format<FMT>;
  const unsigned bits[4] = {w0 & 0xffffu, w0 >> 16, w1 & 0xffffu, w1 >> 16};
  float y[4];
  bool bad = false;
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    const unsigned mag = bits[e] & 0x7fffu;
    amax = amax > mag ? amax : mag;
    bad |= mag >= 0x7f80u;
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

template <int FMT>
__global__ __launch_bounds__(kFp8Threads) void fp8_quantize_kernel(QuantArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[kFp8QTile * kLdT];
  __shared__ unsigned wave_max[kFp8Threads / 64];
  const int t = threadIdx.x;
  const int rt = blockIdx.x / a.col_tiles, ct = blockIdx.x - rt * a.col_tiles;
  const int r0 = rt * kFp8QTile, c0 = ct * kFp8QTile;
  const int lr = t >> 2, lc = (t & 3) * 16;  // this lane's row and first column inside the tile
  const int r = r0 + lr, c = c0 + lc;
  // C % 8 == 0: each half of the lane's 16 columns is inside or outside as a whole; an outside half is zero,
  // which is the zero padding of the row up to C rounded up to 16 (ldq covers it)
  const bool inside = r < a.R && c < a.C, inside_hi = r < a.R && c + 8 < a.C;

  uint4 v0{0u, 0u, 0u, 0u}, v1{0u, 0u, 0u, 0u};
  const uint4* src = reinterpret_cast<const uint4*>(a.x + static_cast<int64_t>(r) * a.ld + c);
  if (inside) v0 = src[0];
  if (inside_hi) v1 = src[1];
  const float s = __builtin_bit_cast(float, a.block[0]);
  unsigned amax = 0;
  uint4 o;
  o.x = quant4<FMT>(v0.x, v0.y, s, amax);
  o.y = quant4<FMT>(v0.z, v0.w, s, amax);
  o.z = quant4<FMT>(v1.x, v1.y, s, amax);
  o.w = quant4<FMT>(v1.z, v1.w, s, amax);

  if (a.q != nullptr && inside) *reinterpret_cast<uint4*>(a.q + static_cast<int64_t>(r) * a.ldq + c) = o;

  if (a.qt != nullptr) {  // (uniform)
    const unsigned w[4] = {o.x, o.y, o.z, o.w};
#pragma unroll
    for (int e = 0; e < 16; ++e) tile[(lc + e) * kLdT + lr] = static_cast<uint8_t>(w[e >> 2] >> (8 * (e & 3)));
    __syncthreads();
    // column t >> 2 of the tile, its rows 16 (t & 3) .. + 15: inside [C][R'] or not as a whole
    const int tc = c0 + (t >> 2), tr = r0 + (t & 3) * 16;
    if (tc < a.C && tr < a.rpad)
      *reinterpret_cast<uint4*>(a.qt + static_cast<int64_t>(tc) * a.ldt + tr) =
          *reinterpret_cast<const uint4*>(tile + (t >> 2) * kLdT + (t & 3) * 16);
  }

  if (a.want_amax) {  // (uniform)
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
      const unsigned other = static_cast<unsigned>(__shfl_xor(static_cast<int>(amax), off, 64));
      amax = amax > other ? amax : other;
    }
    if ((t & 63) == 0) wave_max[t >> 6] = amax;
    __syncthreads();
    if (t == 0) {
      unsigned m = wave_max[0];
#pragma unroll
      for (int w = 1; w < kFp8Threads / 64; ++w) m = m > wave_max[w] ? m : wave_max[w];
      if (m != 0) atomicMax(a.block + 2, m << 16);  // bf16 bits -> fp32 bits
    }
  }
}

__global__ void fp8_scale_update_kernel(uint32_t* __restrict__ blk, int max_exp) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const uint32_t bits = blk[2];
  int p = 0;
  if (bits != 0 && bits < 0x7f800000u) {
    const float amax = __builtin_bit_cast(float, bits);
    const int e = ilogbf(amax);
    const float m = scalbnf(amax, -e);  // in [1, 2)
    p = max_exp - e - (m > 1.75f ? 1 : 0);
    p = p < -126 ? -126 : (p > 126 ? 126 : p);
  }
  blk[0] = static_cast<uint32_t>(127 + p) << 23;
  blk[1] = static_cast<uint32_t>(127 - p) << 23;
  blk[3] = bits;
  blk[2] = 0;
}

}  // namespace

void fp8_quantize(const void* x, int64_t R, int64_t C, int64_t ld, void* block, int fmt, void* q, int64_t ldq, void* qt,
                  int64_t ldt, int want_amax, hipStream_t stream) {
  const Fp8QuantGeometry g = fp8_quant_check(x, R, C, ld, block, fmt, q, ldq, qt, ldt, want_amax != 0);
  const QuantArgs a{static_cast<const uint16_t*>(x), static_cast<uint8_t*>(q), static_cast<uint8_t*>(qt),
                    static_cast<uint32_t*>(block), ld, ldq, ldt, static_cast<int>(R), static_cast<int>(C),
                    static_cast<int>(g.rpad), static_cast<int>(g.col_tiles), want_amax != 0};
  const unsigned grid = static_cast<unsigned>(g.grid);
  if (fmt == kFp8E4M3) fp8_quantize_kernel<kFp8E4M3><<<grid, kFp8Threads, 0, stream>>>(a);
  else fp8_quantize_kernel<kFp8E5M2><<<grid, kFp8Threads, 0, stream>>>(a);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

void fp8_scale_update(void* block, int fmt, hipStream_t stream) {
  fp8_format_check("fp8_scale_update", fmt);
  fp8_block_check("fp8_scale_update", block);
  fp8_scale_update_kernel<<<1, 64, 0, stream>>>(static_cast<uint32_t*>(block),
                                                fmt == kFp8E4M3 ? Fp8Format<kFp8E4M3>::kMaxExp : Fp8Format<kFp8E5M2>::kMaxExp);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace fluxmpi
