// Device helpers that the input-pipeline kernels share (augment.hip, resize_crop.hip): the mixing a
// launch was given (by value or in the device block), the guarded 16-byte load of the uint8 batch, and
// the arithmetic from a source byte to the stored element. Each is a template over the kernel's own
// argument struct K, which names the fields it reads: in, in_bytes, dev_block, step, mode, y0, x0, y1,
// x1, lam, a[3], b[3]. Everything is inlined, so a kernel's code is what it was with the helpers in
// its own file. The products and sums are rounded separately: this header turns contraction off for the
// rest of the translation unit, so include it last.
#pragma once
#include <cstdint>

#include "common.h"

#pragma clang fp contract(off)

namespace fluxmpi {

// words of the device block (api.h: aug_block_set)
constexpr int kAugStep = 0, kAugMode = 1, kAugY0 = 2, kAugX0 = 3, kAugY1 = 4, kAugX1 = 5, kAugLam = 6;

// what a launch mixes with, wave-uniform
struct Mix {
  uint32_t step;
  int mode, y0, x0, y1, x1;
  float lam;
};

template <typename K> __device__ __forceinline__ Mix mix_of(const K& k) {
  const uint32_t* __restrict__ blk = k.dev_block;
  if (blk == nullptr) return {k.step, k.mode, k.y0, k.x0, k.y1, k.x1, k.lam};
  return {blk[kAugStep], static_cast<int>(blk[kAugMode]), static_cast<int>(blk[kAugY0]),
          static_cast<int>(blk[kAugX0]), static_cast<int>(blk[kAugY1]), static_cast<int>(blk[kAugX1]),
          __builtin_bit_cast(float, blk[kAugLam])};
}

// one aligned 16-byte chunk of the batch; the bytes of it that lie outside the tensor read as 0
// (they are never picked) and are not loaded
template <typename K> __device__ __forceinline__ uint4 load_chunk(const K& k, const uint8_t* p) {
  const uint8_t* end = k.in + k.in_bytes;
  if (p >= k.in && p + 16 <= end) return *reinterpret_cast<const uint4*>(p);
  uint32_t v[4] = {0u, 0u, 0u, 0u};
#pragma unroll
  for (int t = 0; t < 16; ++t) {
    const uint8_t* q = p + t;
    if (q >= k.in && q < end) v[t >> 2] |= static_cast<uint32_t>(*q) << (8 * (t & 3));
  }
  return make_uint4(v[0], v[1], v[2], v[3]);
}

// channel c of a packed pixel (channel c at bits 8c), normalised
template <typename K> __device__ __forceinline__ float normalise(const K& k, uint32_t px, int c) {
  const float u = static_cast<float>((px >> (8 * c)) & 0xffu);
  const float m = u * k.a[c];  // rounded on its own: contraction is off
  return m + k.b[c];
}

// one output pixel's C stores from its packed bytes and its partner's
template <typename T, int C, typename K>
__device__ __forceinline__ void pixel_out(const K& k, const Mix& m, uint32_t px, uint32_t pp, bool use_p, bool inbox,
                                          T* o) {
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float z = normalise(k, px, c);
    if (use_p) {
      const float yp = normalise(k, pp, c);
      if (m.mode == 1) {
        const float d = z - yp;
        const float t = m.lam * d;
        z = yp + t;
      } else if (inbox) {
        z = yp;
      }
    }
    o[c] = static_cast<T>(z);
  }
  if constexpr (C == 4) o[3] = static_cast<T>(0.f);
}

}  // namespace fluxmpi
