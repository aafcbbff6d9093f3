// MX block-scaled fp6 (e2m3 / e3m2) quantisation of a bf16 matrix — gfx950. Reached through mx_quantize(fmt = 3, 4).
//
// The formats (mx_host.h): OCP FP6, code = sign << 5 | exponent << MB | mantissa with no inf / NaN.
//   e2m3: MB = 3, bias 1: 0, 0.125 .. 0.875 (subnormal), then 1.m * 2^(e - 1) up to 7.5 = 1.875 * 2^2
//   e3m2: MB = 2, bias 3: 0, 0.0625 .. 0.1875 (subnormal), then 1.m * 2^(e - 3) up to 28 = 1.75 * 2^4
// Every 32 consecutive values along the reduction axis share s = 2^p, p = PMAX - (exponent of amax) - (significand
// of amax > TOP): the scaled amax lies in (FMAX / 2, FMAX] and nothing finite is clamped. The block's E8M0 byte
// 127 - p goes to the scale image, which is mx_quant.hip's. A block that holds an inf or NaN is zeros under the
// byte 255, as mx4_quant.hip's.
//
// Rounding is to nearest, ties to the even code, in integer arithmetic on the fp32 bit pattern of |x| * s (a bf16
// times a power of two: exact, so this is the only rounding). A normal result is the fp32 pattern rebiased and
// shifted right by 23 - MB with the usual "+ half - 1 + lsb" (a carry out of the mantissa moves into the
// exponent field, which is the next code); below the smallest normal the significand with its hidden bit is
// shifted by the exponent's distance as well. No float rounding mode, no conversion instruction: gfx950's scaled
// bf16 -> fp6 conversions are not used (they were not compared with the reference here).
//
// Storage: four codes in three bytes, value i of a block at bits 6 i .. 6 i + 5 of the block's 24 bytes read as one
// little-endian bit string, which is the order the scaled MFMA reads a lane's six VGPRs in (mx6_gemm.hip's header).
//
// The split of the work is mx_quant.hip's: 256 lanes own a 128 x 128 tile of x, whole scale dwords of both images.
//   * Row-wise: in each of 4 passes a lane reads 16 consecutive columns of one row (2 x 16 B) and makes their 16
//     codes: 12 bytes, at byte 12 (t & 7) of the tile row's 96. A 16-byte store needs the bytes of more than one
//     lane. The lanes are PAIRED UP IN QUADS, in registers: the four lanes of a quad hold 48 consecutive bytes
//     (two blocks), every lane fetches the three dwords of the lane above it, and lanes 0 - 2 of the quad store
//     chunks 0 - 2 (16 B each, 16-byte aligned because 96 ct + 48 quad is). That is three cross-lane moves per
//     pass; staging the packed tile through LDS would have cost 12 KiB, three ds_writes, a barrier and the reads
//     for the same stores. C % 32 == 0 lets a quad end after its first block: chunk 1 is then an 8-byte store.
//   * Transposed: the passes also put the bf16 tile into LDS ([128 rows][256 B + 16]). After the barrier a lane
//     owns ONE column and 64 rows of it, two blocks (lanes 0 - 127: rows 0 - 63): 48 bytes, three 16-byte stores at
//     96 rt + 48 half, so that here no lanes have to meet at all. Each of the 64 reads is a ds_read_u16 in which
//     the wave reads 128 consecutive bytes of one tile row (two lanes per bank, one dword: no conflict); it is
//     twice mx4_quant.hip's read count for the same tile and was not measured against a 2-column split that
//     stages its output. R % 32 == 0: a lane may own one block only (a 16-byte and an 8-byte store).
//   The block bytes leave as in mx4_quant.hip: one dword per row (ORed over the row's 8 lanes) and, through a
//   [128 columns][4] LDS table, one per column. No atomics, no state.
#include <stdexcept>
#include <string>

#include "../api.h"
#include "common.h"
#include "mx_host.h"

namespace fluxmpi {
namespace {

constexpr int kLdX = kMxQTile * 2 + 16;  // LDS row stride (bytes) of the bf16 tile
constexpr unsigned kNanByte = 255;       // E8M0's NaN: the byte of a block with a non-finite value

template <int FMT> struct Fp6;
template <> struct Fp6<kMxE2M3> {
  static constexpr int kMB = 3, kBias = 1, kPMax = 2;  // FMAX = 1.875 * 2^2
  static constexpr unsigned kTop = 0x70u;              // 1.875's seven mantissa bits
};
template <> struct Fp6<kMxE3M2> {
  static constexpr int kMB = 2, kBias = 3, kPMax = 4;  // FMAX = 1.75 * 2^4
  static constexpr unsigned kTop = 0x60u;
};

struct Mx6QuantArgs {
  const uint16_t* x;  // bf16 bits [R][ld]
  uint8_t* q;         // [R][ldq] or null, 3 C / 4 bytes a row
  uint8_t* s;         // [R][lds]
  uint8_t* qt;        // [C][ldt] or null, 3 R / 4 bytes a row
  uint8_t* st;        // [C][ldst]
  int64_t ld, ldq, lds, ldt, ldst;
  int R, C, col_tiles;
};

__device__ __forceinline__ unsigned umax6(unsigned a, unsigned b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned mag2x(unsigned w) { return umax6(w & 0x7fffu, (w >> 16) & 0x7fffu); }

// the block's scale from its amax (a bf16 bit pattern without sign): the fp32 bits of 2^p, or 0 for a block
// with a non-finite value (its codes are then all zero); `byte` is what the scale image gets
template <int FMT>
__device__ __forceinline__ unsigned block_scale(unsigned amax, unsigned& byte) {
  if (amax >= 0x7f80u) {
    byte = kNanByte;
    return 0u;
  }
  int p = 0;
  if (amax != 0u) {
    p = Fp6<FMT>::kPMax + 127 - static_cast<int>(amax >> 7) - ((amax & 0x7fu) > Fp6<FMT>::kTop ? 1 : 0);
    p = p < -126 ? -126 : (p > 126 ? 126 : p);
  }
  byte = static_cast<unsigned>(127 - p);
  return static_cast<unsigned>(127 + p) << 23;
}

// one bf16 bit pattern (the low 16 bits of b) -> its 6-bit code
template <int FMT>
__device__ __forceinline__ unsigned code1(unsigned b, float s) {
  constexpr int kShift = 23 - Fp6<FMT>::kMB;
  constexpr unsigned kNormal = 127 + 1 - Fp6<FMT>::kBias;  // the fp32 exponent field of the smallest normal
  const unsigned y = __builtin_bit_cast(unsigned, __builtin_bit_cast(float, (b & 0x7fffu) << 16) * s);
  const unsigned e = y >> 23;
  // normal: exponent field e - kNormal + 1 above the mantissa, then one rounding shift
  const unsigned v = y - ((kNormal - 1) << 23);
  const unsigned rn = (v + ((1u << (kShift - 1)) - 1u) + ((v >> kShift) & 1u)) >> kShift;
  // below it: the significand in units of the subnormal step, 2^(kNormal - e) further down
  const unsigned sig = (y & 0x7fffffu) | 0x800000u;
  int sh = kShift + static_cast<int>(kNormal) - static_cast<int>(e);  // (only used where e < kNormal)
  sh = sh > 31 ? 31 : (sh < 1 ? 1 : sh);
  const unsigned rs = (sig + ((1u << (sh - 1)) - 1u) + ((sig >> sh) & 1u)) >> sh;
  unsigned mag = e >= kNormal ? rn : rs;
  mag = mag > 31u ? 31u : mag;  // (a scale held at 2^+-126 aside, nothing reaches this)
  return ((b >> 10) & 0x20u) | mag;
}

// 16 codes -> 96 bits, code i at bit 6 i
__device__ __forceinline__ void pack16(const unsigned (&c)[16], unsigned (&d)[3]) {
  d[0] = d[1] = d[2] = 0u;
#pragma unroll
  for (int i = 0; i < 16; ++i) {
    const int w = (6 * i) >> 5, sh = (6 * i) & 31;
    d[w] |= c[i] << sh;
    if (sh > 26) d[w + 1] |= c[i] >> (32 - sh);
  }
}

template <int FMT>
__global__ __launch_bounds__(kFp8Threads) void mx6_quantize_kernel(Mx6QuantArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t tile[kMxQTile * kLdX];
  __shared__ uint32_t tscale[kMxQTile];
  const int t = threadIdx.x;
  const int rt = blockIdx.x / a.col_tiles, ct = blockIdx.x - rt * a.col_tiles;
  const int r0 = rt * kMxQTile, c0 = ct * kMxQTile;
  const int lr = t >> 3, lc = (t & 7) * 16;  // this lane's row (of a pass) and first column inside the tile
  const int c = c0 + lc;                     // C % 32 == 0: the lane's 16 columns are inside or outside as a whole
  // the quad's 64 columns = 48 bytes: how many of them are inside C (0, 24 or 48), and this lane's chunk
  const int quad = (t & 7) >> 2, j = t & 3;
  const int left = a.C - (c0 + 64 * quad);
  const int qbytes = left >= 64 ? 48 : (left >= 32 ? 24 : 0);

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
      unsigned amax = umax6(umax6(umax6(mag2x(v0.x), mag2x(v0.y)), umax6(mag2x(v0.z), mag2x(v0.w))),
                            umax6(umax6(mag2x(v1.x), mag2x(v1.y)), umax6(mag2x(v1.z), mag2x(v1.w))));
      amax = umax6(amax, static_cast<unsigned>(__shfl_xor(static_cast<int>(amax), 1, 64)));
      unsigned byte;
      const float s = __builtin_bit_cast(float, block_scale<FMT>(amax, byte));
      const unsigned w[8] = {v0.x, v0.y, v0.z, v0.w, v1.x, v1.y, v1.z, v1.w};
      unsigned codes[16], d[3];
#pragma unroll
      for (int i = 0; i < 8; ++i) codes[2 * i] = code1<FMT>(w[i], s), codes[2 * i + 1] = code1<FMT>(w[i] >> 16, s);
      pack16(codes, d);
      if (byte == kNanByte) d[0] = d[1] = d[2] = 0u;  // (inf * 0 is a NaN, which would count as the top code)
      unsigned n[3];                                  // the three dwords of the next lane of the quad
#pragma unroll
      for (int i = 0; i < 3; ++i) n[i] = static_cast<unsigned>(__shfl_down(static_cast<int>(d[i]), 1, 64));
      const uint4 o = j == 0 ? uint4{d[0], d[1], d[2], n[0]} : (j == 1 ? uint4{d[1], d[2], n[0], n[1]} : uint4{d[2], n[0], n[1], n[2]});
      if (r < a.R && j < 3) {
        uint8_t* dst = a.q + static_cast<int64_t>(r) * a.ldq + 96 * ct + 48 * quad + 16 * j;
        if (16 * j + 16 <= qbytes) *reinterpret_cast<uint4*>(dst) = o;
        else if (16 * j + 8 <= qbytes) *reinterpret_cast<uint2*>(dst) = uint2{o.x, o.y};
      }
      // the row's four block bytes as one dword (a block past C is all zero: 127, the padding)
      unsigned sw = byte << (8 * ((t & 7) >> 1));
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
    const int col = t & 127, half = t >> 7;  // column `col` of the tile, its rows 64 half .. + 63
    unsigned out[12];
    uint8_t* tb = reinterpret_cast<uint8_t*>(tscale);
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      unsigned w[32], amax = 0;
#pragma unroll
      for (int i = 0; i < 32; ++i) {
        w[i] = *reinterpret_cast<const uint16_t*>(tile + (64 * half + 32 * b + i) * kLdX + col * 2);
        amax = umax6(amax, w[i] & 0x7fffu);
      }
      unsigned byte;
      const float s = __builtin_bit_cast(float, block_scale<FMT>(amax, byte));
#pragma unroll
      for (int hb = 0; hb < 2; ++hb) {
        unsigned codes[16], d[3];
#pragma unroll
        for (int i = 0; i < 16; ++i) codes[i] = code1<FMT>(w[16 * hb + i], s);
        pack16(codes, d);
#pragma unroll
        for (int i = 0; i < 3; ++i) out[6 * b + 3 * hb + i] = byte == kNanByte ? 0u : d[i];
      }
      tb[col * 4 + 2 * half + b] = static_cast<uint8_t>(byte);  // a block past R is all zero: 127, the padding
    }
    // R % 32 == 0: the lane's blocks are inside or outside as a whole
    const int rleft = a.R - (r0 + 64 * half);
    const int cbytes = rleft >= 64 ? 48 : (rleft >= 32 ? 24 : 0);
    if (c0 + col < a.C) {
      uint8_t* dst = a.qt + static_cast<int64_t>(c0 + col) * a.ldt + 96 * rt + 48 * half;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        if (16 * k + 16 <= cbytes) *reinterpret_cast<uint4*>(dst + 16 * k) = uint4{out[4 * k], out[4 * k + 1], out[4 * k + 2], out[4 * k + 3]};
        else if (16 * k + 8 <= cbytes) *reinterpret_cast<uint2*>(dst + 16 * k) = uint2{out[4 * k], out[4 * k + 1]};
      }
    }
    __syncthreads();
    if (t < kMxQTile && c0 + t < a.C)
      *reinterpret_cast<uint32_t*>(a.st + static_cast<int64_t>(c0 + t) * a.ldst + 4 * rt) = tscale[t];
  }
}

}  // namespace

void mx6_quantize_launch(const void* x, int64_t R, int64_t C, int64_t ld, int fmt, void* q, int64_t ldq, void* s,
                         int64_t lds, void* qt, int64_t ldt, void* st, int64_t ldst, int64_t col_tiles, int64_t grid,
                         hipStream_t stream) {
  const Mx6QuantArgs a{static_cast<const uint16_t*>(x), static_cast<uint8_t*>(q), static_cast<uint8_t*>(s),
                       static_cast<uint8_t*>(qt), static_cast<uint8_t*>(st), ld, ldq, lds, ldt, ldst,
                       static_cast<int>(R), static_cast<int>(C), static_cast<int>(col_tiles)};
  if (fmt == kMxE2M3) mx6_quantize_kernel<kMxE2M3><<<static_cast<unsigned>(grid), kFp8Threads, 0, stream>>>(a);
  else mx6_quantize_kernel<kMxE3M2><<<static_cast<unsigned>(grid), kFp8Threads, 0, stream>>>(a);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace fluxmpi
