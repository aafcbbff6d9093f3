// MFMA operand helpers shared by the one-pass conv3 -> bn3 backward kernels (conv3bn3_bwd.hip and
// conv3bn3_s2_bwd.hip, the identity blocks of stages 1 and 2; conv3ds_bwd.hip, the downsample block): one
// copy of the transposed fragment read, and the identity-block kernels' argument block.
#pragma once
#include <hip/hip_runtime.h>

namespace fluxmpi {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// the operands of the identity blocks' kernel (conv3bn3_bwd.hip: Cout = 256, Cin = 64; conv3bn3_s2_bwd.hip:
// Cout = 512, Cin = 128)
struct C3Args {
  const __bf16* dy;          // [P][Cout]
  const __bf16* x3;          // [P][Cout]
  const uint8_t* mask;       // [P * Cout / 8]
  const float* w;            // bn3 weight (nullable: 1)
  const float* mean;
  const float* inv;
  const float* sum_dy;       // [Cout] = dbias
  const float* sum_dy_xhat;  // [Cout] = dweight
  const __bf16* a2;          // [P][Cin]
  const __bf16* wt;          // conv3 filter [Cout][Cin]
  __bf16* d_a2;              // [P][Cin]
  float* ws;                 // [gridDim.x][Cout][Cin]
  int64_t P;
};

// the Cout = 512, Cin = 128 form (conv3bn3_s2_bwd.hip), launched by conv3bn3_bwd once it has checked the problem
void conv3bn3_s2_launch(const C3Args& p, int slabs, hipStream_t stream);

// lane l: img[k0 + 8 (l >> 4) + j][c0 + (l & 15)], j = 0..7 (two transposed reads), ld in elements
__device__ __forceinline__ bf16x8 frag_tr(const __bf16* __restrict__ img, int ld, int k0, int c0) {
  const int l = threadIdx.x & 63;
  const int g = l >> 4, li = l & 15, q = li >> 2, p = li & 3;
  const __bf16* a0 = img + (k0 + 8 * g + q) * ld + c0 + 4 * p;
  const __bf16* a1 = a0 + 4 * ld;
  typedef short short4v __attribute__((ext_vector_type(4)));
  typedef __attribute__((address_space(3))) short4v lds_short4v;
  short4v lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4v*)(a0));
  short4v hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_short4v*)(a1));
  bf16x8 out;
  __builtin_memcpy(&out, &lo, 8);
  __builtin_memcpy(reinterpret_cast<char*>(&out) + 8, &hi, 8);
  return out;
}

}  // namespace fluxmpi
