// MX block-scaled fp4 (e2m1) quantisation of a bf16 matrix — gfx950. Reached through mx_quantize(fmt = 2).
//
// The format (mx_host.h): values +-{0, 0.5, 1, 1.5, 2, 3, 4, 6}, code = sign << 3 | magnitude index, two codes per
// byte with element 2 i in the low nibble of byte i. Every 32 consecutive values along the reduction axis share
// s = 2^p, p = 2 - (exponent of amax) - (significand of amax > 1.5): the scaled amax lies in (3, 6] and nothing
// finite is clamped. The block's E8M0 byte 127 - p goes to the scale image, which is mx_quant.hip's. A block
// that holds an inf or NaN is written as zeros with the byte 255 (E8M0's NaN): e2m1 has no code for either.
//
// Rounding is to nearest with ties to the even code, done on the bit pattern of |x| * s (a bf16 times a power
// of two: exact in fp32) by counting the grid's seven midpoints below it:
//   code = (y > 0.25) + (y >= 0.75) + (y > 1.25) + (y >= 1.75) + (y > 2.5) + (y >= 3.5) + (y > 5)
// A midpoint belongs to the neighbour with the even code, which is what decides > against >=. Integer compares
// of the fp32 bits, no float rounding mode, no conversion instruction: gfx950's packed bf16 -> fp4 conversions
// with a scale operand are not used (they were not compared with the reference here).
//
// The split of the work is mx_quant.hip's, so that a workgroup still owns whole scale dwords of both images:
// 256 lanes own a 128 x 128 tile of x and read it once.
//   * Row-wise: in each of 4 passes a lane reads 16 consecutive columns of one row (2 x 16 B) and writes their
//     16 codes as 8 bytes; a block is the columns of lanes 2 i and 2 i + 1 (one exchange for the amax), the
//     row's four block bytes are ORed over its 8 lanes and leave as one dword.
//   * Transposed: the passes also put the bf16 tile into LDS ([128 rows][256 B + 16]). The transposed image
//     packs PAIRS ALONG R into a byte, so the tile has to be consumed two rows at a time. It is, in registers
//     and not in the LDS access: after the barrier a lane owns two adjacent columns and one 32-row block of
//     them (wave w owns block w) and reads the block's 32 rows one ds_read_b32 each. In every such read the 64
//     lanes of a wave read 64 consecutive dwords of ONE tile row, i.e. every bank twice in two conflict-free
//     halves, whatever the row stride is; rows 2 i and 2 i + 1 then sit in the lane's registers i apart, and
//     byte i of a column's 16 is built from them. A lane stores 16 B per column. The block bytes meet in a
//     [128 columns][4] LDS table and leave as one dword per column.
#include <stdexcept>
#include <string>

#include "../api.h"
#include "common.h"
#include "mx_host.h"

namespace fluxmpi {
namespace {

constexpr int kLdX = kMxQTile * 2 + 16;  // LDS row stride (bytes) of the bf16 tile
constexpr unsigned kNanByte = 255;       // E8M0's NaN: the byte of a block with a non-finite value

struct Mx4QuantArgs {
  const uint16_t* x;  // bf16 bits [R][ld]
  uint8_t* q;         // [R][ldq] or null, C / 2 bytes a row
  uint8_t* s;         // [R][lds]
  uint8_t* qt;        // [C][ldt] or null, R / 2 bytes a row
  uint8_t* st;        // [C][ldst]
  int64_t ld, ldq, lds, ldt, ldst;
  int R, C, col_tiles;
};

__device__ __forceinline__ unsigned umax4(unsigned a, unsigned b) { return a > b ? a : b; }
__device__ __forceinline__ unsigned mag2x(unsigned w) { return umax4(w & 0x7fffu, (w >> 16) & 0x7fffu); }

// the block's scale from its amax (a bf16 bit pattern without sign): the fp32 bits of 2^p, or 0 for a block
// with a non-finite value (its codes are then all zero); `byte` is what the scale image gets
__device__ __forceinline__ unsigned block_scale(unsigned amax, unsigned& byte) {
  if (amax >= 0x7f80u) {
    byte = kNanByte;
    return 0u;
  }
  int p = 0;
  if (amax != 0u) {
    p = 2 + 127 - static_cast<int>(amax >> 7) - ((amax & 0x7fu) > 0x40u ? 1 : 0);
    p = p < -126 ? -126 : (p > 126 ? 126 : p);
  }
  byte = static_cast<unsigned>(127 - p);
  return static_cast<unsigned>(127 + p) << 23;
}

// one bf16 bit pattern (the low 16 bits of b) -> its e2m1 code
__device__ __forceinline__ unsigned code1(unsigned b, float s) {
  const unsigned y = __builtin_bit_cast(unsigned, __builtin_bit_cast(float, (b & 0x7fffu) << 16) * s);
  const unsigned mag = (y > 0x3e800000u) + (y >= 0x3f400000u) + (y > 0x3fa00000u) + (y >= 0x3fe00000u) +
                       (y > 0x40200000u) + (y >= 0x40600000u) + (y > 0x40a00000u);
  return ((b >> 12) & 0x8u) | mag;
}

// 8 bf16 values in 4 words (element 2 i in the low half of word i) -> 8 codes in one word, element 0 lowest
__device__ __forceinline__ unsigned cast8(unsigned w0, unsigned w1, unsigned w2, unsigned w3, float s) {
  const unsigned w[4] = {w0, w1, w2, w3};
  unsigned out = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) out |= (code1(w[i], s) | (code1(w[i] >> 16, s) << 4)) << (8 * i);
  return out;
}

__global__ __launch_bounds__(kFp8Threads) void mx4_quantize_kernel(Mx4QuantArgs a) {
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
      unsigned amax = umax4(umax4(umax4(mag2x(v0.x), mag2x(v0.y)), umax4(mag2x(v0.z), mag2x(v0.w))),
                            umax4(umax4(mag2x(v1.x), mag2x(v1.y)), umax4(mag2x(v1.z), mag2x(v1.w))));
      amax = umax4(amax, static_cast<unsigned>(__shfl_xor(static_cast<int>(amax), 1, 64)));
      unsigned byte;
      const float s = __builtin_bit_cast(float, block_scale(amax, byte));
      uint2 o;
      o.x = cast8(v0.x, v0.y, v0.z, v0.w, s);
      o.y = cast8(v1.x, v1.y, v1.z, v1.w, s);
      if (byte == kNanByte) o = uint2{0u, 0u};  // (inf * 0 is a NaN, which would count as code 7)
      if (inside) *reinterpret_cast<uint2*>(a.q + static_cast<int64_t>(r) * a.ldq + (c >> 1)) = o;
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
    const int cp = t & 63, blk = t >> 6;  // columns 2 cp and 2 cp + 1 of the tile, its rows 32 blk .. + 31
    unsigned w[32];
    unsigned amax0 = 0, amax1 = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      w[i] = *reinterpret_cast<const uint32_t*>(tile + (32 * blk + i) * kLdX + cp * 4);
      amax0 = umax4(amax0, w[i] & 0x7fffu), amax1 = umax4(amax1, (w[i] >> 16) & 0x7fffu);
    }
    unsigned byte0, byte1;
    const float s0 = __builtin_bit_cast(float, block_scale(amax0, byte0));
    const float s1 = __builtin_bit_cast(float, block_scale(amax1, byte1));
    // byte i of a column = rows 2 i (low nibble) and 2 i + 1 of the block
    unsigned o0[4] = {0u, 0u, 0u, 0u}, o1[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int i = 0; i < 32; ++i) {
      o0[i >> 3] |= code1(w[i], s0) << (4 * (i & 7));
      o1[i >> 3] |= code1(w[i] >> 16, s1) << (4 * (i & 7));
    }
    if (byte0 == kNanByte) o0[0] = o0[1] = o0[2] = o0[3] = 0u;
    if (byte1 == kNanByte) o1[0] = o1[1] = o1[2] = o1[3] = 0u;
    // C % 32 == 0 and R % 32 == 0: the column pair and the row block are inside or outside as a whole
    const int col = c0 + 2 * cp, rb = r0 + 32 * blk;
    if (col < a.C && rb < a.R) {
      *reinterpret_cast<uint4*>(a.qt + static_cast<int64_t>(col) * a.ldt + (rb >> 1)) = uint4{o0[0], o0[1], o0[2], o0[3]};
      *reinterpret_cast<uint4*>(a.qt + static_cast<int64_t>(col + 1) * a.ldt + (rb >> 1)) = uint4{o1[0], o1[1], o1[2], o1[3]};
    }
    // a block past R is all zero: 127, the padding of the column's dword
    uint8_t* tb = reinterpret_cast<uint8_t*>(tscale);
    tb[(2 * cp) * 4 + blk] = static_cast<uint8_t>(byte0);
    tb[(2 * cp + 1) * 4 + blk] = static_cast<uint8_t>(byte1);
    __syncthreads();
    if (t < kMxQTile && c0 + t < a.C)
      *reinterpret_cast<uint32_t*>(a.st + static_cast<int64_t>(c0 + t) * a.ldst + 4 * rt) = tscale[t];
  }
}

}  // namespace

void mx4_quantize_launch(const void* x, int64_t R, int64_t C, int64_t ld, void* q, int64_t ldq, void* s, int64_t lds,
                         void* qt, int64_t ldt, void* st, int64_t ldst, int64_t col_tiles, int64_t grid,
                         hipStream_t stream) {
  const Mx4QuantArgs a{static_cast<const uint16_t*>(x), static_cast<uint8_t*>(q), static_cast<uint8_t*>(s),
                       static_cast<uint8_t*>(qt), static_cast<uint8_t*>(st), ld, ldq, lds, ldt, ldst,
                       static_cast<int>(R), static_cast<int>(C), static_cast<int>(col_tiles)};
  mx4_quantize_kernel<<<static_cast<unsigned>(grid), kFp8Threads, 0, stream>>>(a);
  FLUXMPI_HIP_CHECK(hipGetLastError());
}

}  // namespace fluxmpi
