// The 3 x 3 bilinear weights of a sub-pixel cycle spin (jolideco/utils/torch.py:122-143, `grid_weights`), shared by the
// element-wise priors (elementwise.hip) and the GMM patch prior (gmm_subpix.hip): ONE definition, so both form the same
// bits from the same offsets.
#pragma once
#include <hip/hip_runtime.h>

namespace jd {

// k[i][j] = wx(j - 1) * wy(i - 1), w(t) = 1 - |t - o| where |t - o| < 1, else 0: the float32 operations of
// `grid_weights`, one by one (no contraction), so the weights carry the reference's bits
__device__ __forceinline__ void subpix_weights(float x0, float y0, float (&k)[3][3]) {
#pragma clang fp contract(off)
  float wx[3], wy[3];
#pragma unroll
  for (int t = 0; t < 3; ++t) {
    const float dx = fabsf((float)(t - 1) - x0), dy = fabsf((float)(t - 1) - y0);
    wx[t] = dx < 1.f ? 1.f - dx : 0.f;
    wy[t] = dy < 1.f ? 1.f - dy : 0.f;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) k[i][j] = wx[j] * wy[i];
}

}  // namespace jd
