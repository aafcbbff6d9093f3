// The BatchNorm input-gradient arithmetic, shared by every kernel that forms dx (batchnorm.hip's dx
// passes, single and dual, and conv3bn3_bwd.hip / conv3ds_bwd.hip, which form the same dx in registers): one
// copy, so the bits agree.
//
// dx = w*invstd * (dy_eff - sum_dy/R - xhat * sum_dy_xhat/R); dres = dy_eff
// (sum_dy = db, sum_dy_xhat = dw, produced by bn_finalize_bwd_kernel), evaluated as
// dx = A*dy_eff + B*x + D with per-channel A = w*invstd, B = -A*invstd*mean(dy_eff*xhat),
// D = A*(mean*invstd*mean(dy_eff*xhat) - mean(dy_eff)).
#pragma once
#include <hip/hip_runtime.h>

namespace fluxmpi {

struct DxCoef {
  float a, b, d, sh;  // sh: forward shift (RM == 2 mask recompute, with a == forward scale)
};

// the coefficients of one channel from the per-channel values themselves (however they were loaded)
__device__ __forceinline__ DxCoef dx_coef_of(bool has_w, float wv, bool has_bias, float bv, float m, float iv,
                                             float dwv, float dbv, float inv_n) {
  const float sc = (has_w ? wv : 1.f) * iv;
  const float k2 = dbv * inv_n, k3 = dwv * inv_n;
  DxCoef k;
  k.a = sc;
  k.b = -sc * iv * k3;
  k.d = sc * (m * iv * k3 - k2);
  k.sh = fmaf(-m, sc, has_bias ? bv : 0.f);
  return k;
}

__device__ __forceinline__ DxCoef dx_coef(int c, const float* __restrict__ w, const float* __restrict__ bias,
                                          const float* __restrict__ smean, const float* __restrict__ sinv,
                                          const float* __restrict__ dw, const float* __restrict__ db, float inv_n) {
  const float iv = sinv[c], m = smean[c];
  const float wv = w ? w[c] : 1.f, dwv = dw[c], dbv = db[c], bv = bias ? bias[c] : 0.f;
  return dx_coef_of(true, wv, true, bv, m, iv, dwv, dbv, inv_n);
}

// d <- dy_eff (dy under the ReLU mode RM), xv <- dx, for a lane's 8 channels with coefficients k[0..8)
template <typename T, int RM, bool DRES>
__device__ __forceinline__ void dx_vec(float (&d)[8], float (&xv)[8], const float (&yv)[8], unsigned mbs,
                                       const DxCoef* k) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    float dd = d[j];
    if (RM == 1) dd = yv[j] > 0.f ? dd : 0.f;
    if (RM == 3) dd = (mbs >> j) & 1u ? dd : 0.f;
    if (RM == 2) dd = fmaf(xv[j], k[j].a, k[j].sh) > 0.f ? dd : 0.f;
    d[j] = dd;
    xv[j] = fmaf(k[j].a, dd, fmaf(k[j].b, xv[j], k[j].d));
  }
}

}  // namespace fluxmpi
