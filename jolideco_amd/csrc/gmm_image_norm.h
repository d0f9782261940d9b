// Image norms of the GMM patch prior, shared by the 8x8 (gmm_gather.hip) and the 16x16 (gmm256.hip) kernels: n(f), n^-1(v), n'(f), the
// argument block of the overlap-add kernels and the chain-rule term they add.  ONE definition of each, so both patch
// sizes produce the same bits for the same pixel.
#pragma once
#include <hip/hip_runtime.h>

#include <type_traits>

#include "jd_adam.h"

namespace jd {

enum { NORM_IDENTITY = 0, NORM_ASINH = 1, NORM_FIXED_MAX = 2, NORM_SIGMOID = 3, NORM_ATAN = 4, NORM_LOG = 5, NORM_POWER = 6,
       NORM_COUNT = 7 };
constexpr float NORM_PI = 3.14159265358979323846f;  // float(torch.pi)

struct ImageNormArgs {
  int kind;
  float p0, p1;
  float c;  // asinh: asinh(p1 / p0), the denominator (host, jd_gmm_set_image_norm); otherwise unused
};

template <int KIND>
__device__ __forceinline__ float image_norm_value(float f, const ImageNormArgs& nm) {
#pragma clang fp contract(off)
  if (KIND == NORM_ASINH) return asinhf(f / nm.p0) / nm.c;
  if (KIND == NORM_FIXED_MAX) {
    const float t = f / nm.p0;
    return t < 0.f ? 0.f : (t > 1.f ? 1.f : t);  // (torch.clip: a NaN stays a NaN)
  }
  if (KIND == NORM_SIGMOID) return 1.f / (1.f + expf(-(f - nm.p1 / 2.f) / nm.p0));
  if (KIND == NORM_ATAN) return 2.f * atanf(f / nm.p0) / NORM_PI;
  if (KIND == NORM_LOG) return logf(f / nm.p0);
  if (KIND == NORM_POWER) return powf(f / nm.p1, nm.p0);
  return f;
}

// n^-1(v), the host `inverse` of jolideco_amd/utils/norms.py term by term (the prior image, gmm_prior_image.hip): asinh
// alpha sinh(v asinh(beta / alpha)); fixed-max v max_value (no clip to undo); sigmoid alpha log(v / (1 - v)) + beta / 2; atan
// pi / 2 tan(v), WITHOUT alpha as the reference has it; log alpha exp(v); power beta v^(1 / alpha)
template <int KIND>
__device__ __forceinline__ float image_norm_inverse(float v, const ImageNormArgs& nm) {
#pragma clang fp contract(off)
  if (KIND == NORM_ASINH) return nm.p0 * sinhf(v * nm.c);
  if (KIND == NORM_FIXED_MAX) return v * nm.p0;
  if (KIND == NORM_SIGMOID) return nm.p0 * logf(v / (1.f - v)) + nm.p1 / 2.f;
  if (KIND == NORM_ATAN) return 0.5f * NORM_PI * tanf(v);
  if (KIND == NORM_LOG) return nm.p0 * expf(v);
  if (KIND == NORM_POWER) return nm.p1 * powf(v, 1.f / nm.p0);
  return v;
}

// n'(f); the kind is uniform over the launch (one scalar branch per call)
__device__ __forceinline__ float image_norm_deriv(float f, const ImageNormArgs& nm) {
#pragma clang fp contract(off)  // (the same bits wherever it is inlined: tiled = per-pixel gather)
  switch (nm.kind) {
    case NORM_ASINH: {
      const float t = f / nm.p0;
      return 1.f / (nm.p0 * sqrtf(1.f + t * t) * nm.c);
    }
    case NORM_FIXED_MAX: {
      const float t = f / nm.p0;
      return t >= 0.f && t <= 1.f ? 1.f / nm.p0 : 0.f;  // (inclusive ends: torch.clip's backward)
    }
    case NORM_SIGMOID: {
      const float sg = 1.f / (1.f + expf(-(f - nm.p1 / 2.f) / nm.p0));
      return sg * (1.f - sg) / nm.p0;
    }
    case NORM_ATAN: {
      const float t = f / nm.p0;
      return 2.f / (NORM_PI * nm.p0 * (1.f + t * t));
    }
    case NORM_LOG: return 1.f / f;
    case NORM_POWER: return (nm.p0 / nm.p1) * powf(f / nm.p1, nm.p0 - 1.f);
    default: return 1.f;
  }
}

// sum * n'(f), the product rounded (NORM), or the sum itself: what the adjoint kernels of the staged passes (gmm_subpix.hip,
// gmm_jitter.hip) add for a non-zero sum.  Each keeps its own rule for an exact zero.
template <bool NORM>
__device__ __forceinline__ float normed_sum(float sum, float f, const ImageNormArgs& nm) {
#pragma clang fp contract(off)
  return NORM ? sum * image_norm_deriv(f, nm) : sum;
}

// f(std::integral_constant<int, KIND>{}) for the NORM_* constant that equals `kind`: the host's way to the kernel
// instantiated for it.  False for a kind outside the enum; the caller refuses in its own words.
template <class F>
bool dispatch_norm_kind(int kind, F&& f) {
  switch (kind) {
    case NORM_IDENTITY: f(std::integral_constant<int, NORM_IDENTITY>{}); return true;
    case NORM_ASINH: f(std::integral_constant<int, NORM_ASINH>{}); return true;
    case NORM_FIXED_MAX: f(std::integral_constant<int, NORM_FIXED_MAX>{}); return true;
    case NORM_SIGMOID: f(std::integral_constant<int, NORM_SIGMOID>{}); return true;
    case NORM_ATAN: f(std::integral_constant<int, NORM_ATAN>{}); return true;
    case NORM_LOG: f(std::integral_constant<int, NORM_LOG>{}); return true;
    case NORM_POWER: f(std::integral_constant<int, NORM_POWER>{}); return true;
    default: return false;
  }
}

struct GmmGatherArgs {
  const float* gpatch;
  float* grad;
  int H, W, stride, nPx, nPy, shift_y, shift_x, row_begin, row_end;  // patch-row shard
  const int* shift_dev;  // nullable, device [2] = {shift_y, shift_x} residues: read instead of the two members above (use_device_shift)
  int y_begin, y_end;                                                // rolled-frame pixel rows covered
  float coef;
  // fused backward pass (winner != nullptr and no fallback): the row of patch n is grec[winner[n]] (none if < 0)
  const int32_t* winner;
  const float* grec;
  const int* flag;
  int gen;
  // band output (band != nullptr): instead of accumulating into `grad` at the un-rolled position, the rows
  // [y_begin, y_end) of the ROLLED frame are written (assigned; 0 where no patch of the shard covers a pixel) to
  // band[(Y - y_begin) * W + X] -- the compact piece a rank of a sharded prior exchanges (jd_add_rolled_bands)
  float* band;
  // tile kernel: W % 4 == 0 and 16-byte aligned images: the pixel groups of a thread start at X = shift_x (mod 4), so that
  // their un-rolled column is a multiple of 4 and the gradient image is read and written with 16-byte accesses
  int vec;
  // fused optimizer step (do_step; tile kernel, whole image): instead of grad += coef * sum the kernel forms
  // g = step.grad_flux[pixel] + coef * sum (the other gradient terms, read only) and applies the stand-alone step's update to
  // the pixel -- one pass less over the gradient image and one launch less per step
  int do_step;
  int preload;  // do_step: the step's streams are loaded before the patch rows (JD_GMM_GATHER_PRELOAD=0: behind the barrier)
  AdamArgs step;
  // image norm of the pass (kind != 0: the NORM instantiations of the gather kernels): every pixel's coef * sum is
  // multiplied by n'(raw_flux[pixel]), the rounded product (coef * sum) * n' in all three output forms; a pixel whose sum
  // is exactly 0 receives nothing (n' may be infinite there: log norm of a zero pixel)
  ImageNormArgs norm;
  const float* raw_flux;
};

// (coef * sum) * n'(f), each product rounded (callers run under `fp contract(off)`); nothing for an exact zero sum
__device__ __forceinline__ float gather_normed_term(const GmmGatherArgs& a, float sum, float f) {
#pragma clang fp contract(off)
  if (sum == 0.f) return 0.f;
  const float cs = a.coef * sum;
  return cs * image_norm_deriv(f, a.norm);
}

}  // namespace jd
