// GMM patch prior for 16x16 patches (D = 256): the dense fp32 path of gmm256.hip, reached from the public entries of
// gmm.hip through a D = 256 handle.
#pragma once
#include "jd_common.h"
#include "gmm_image_norm.h"

namespace jd {

struct Gmm256;  // mixture constants in MFMA fragment order + the workspaces of one handle

int gmm256_create(int K, const float* prec_chol, const float* mu_prec, const float* const_k, const float* pixel_w,
                  Gmm256** out);
void gmm256_destroy(Gmm256* g);
bool gmm256_is_triangular(const Gmm256* g);
int gmm256_set_const_residual(Gmm256* g, const float* residual);  // host (K,): jd_gmm_set_const_residual
// Whole-image pass: `image` is what the patches are cut from (n(flux) under an image norm, else the flux itself),
// `raw_flux` what the overlap-add evaluates n' on.  Same value / gradient / arg-max contract as jd_gmm_prior_fwd_bwd.
// patch_norm: 0 = subtract-mean, 1 = std-subtract-mean (jd_gmm_set_patch_norm).
int gmm256_prior(Gmm256* g, const float* image, const float* raw_flux, const ImageNormArgs& norm, int H, int W, int stride,
                 int shift_y, int shift_x, int marginalize, float value_scale, float* value_out, int accumulate_value,
                 float grad_coef, float* grad_flux_accum, int32_t* argmax_out, const int* shift_dev, hipStream_t stream,
                 int patch_norm = 0);
// x: (n, 256) device, out: (n, K) device
int gmm256_estimate_log_prob(Gmm256* g, const float* x, int n, float* out, hipStream_t stream);

}  // namespace jd
