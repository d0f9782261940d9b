// The prior image of the GMM patch prior (jolideco/priors/patches/core.py:123-175, `prior_image`): what the mixture believes
// the flux looks like.  With N = n(flux), R0 = roll(N, (sy, sx)) and the patch grid of the plain prior (n_y x n_x patches of
// P x P pixels at stride s), patch (i, j) has the mean m_ij and the arg-max component k_ij of its mean-free pixels (the
// unchanged max-mode forward pass; -1 for a filtered patch), and with a table T of K images of P x P pixels
//
//   R[Y, X]     = sum over the patches (i, j) that cover (Y, X), i ascending then j ascending, k_ij >= 0, of
//                 w[Y - i s, X - j s] (T[k_ij][Y - i s, X - j s] + m_ij)           (0 where no patch covers the pixel)
//   out[y, x] (+)= scale n^-1(R[(y + sy) mod H, (x + sx) mod W])
//
// w = get_pixel_weights((P, P), s) (jolideco/utils/numpy.py:54-79): the outer product of a trapezoid profile, rescaled to
// sum s^2.  The host forms the profile and the factor in float64 as numpy does; a kernel multiplies them in float32.
//
// Two launches behind the forward pass, no atomics, a fixed order of the additions -- run-to-run identical:
//   gmm_patch_mean_kernel          one thread per patch: the P^2 pixels of the rolled, normed image, rows then columns in order
//   gmm_prior_image_gather_kernel  tiles of PI_TY x PI_TX pixels of the ROLLED frame, 256 threads; winners and means of the
//                                  patches a tile touches go to LDS once per block (at most (PI_TY + P - 1) x (PI_TX + P - 1)
//                                  of them, stride 1), as does w; a thread owns one column and 4 rows of the tile, so a wave
//                                  reads 64 neighbouring table entries of a few components (L2) and writes 64 consecutive
//                                  pixels of a row of the output (two runs where the roll's seam cuts the row)
// HBM traffic per pixel: 4 B accumulator write (+ 4 B read when accumulating); the normed image is read P^2 / s^2 times for
// the means and served by L2 beyond the first; winners and means are 8 B per patch and tile; the table (K P^2 floats) stays in L2.
#include "gmm_internal.h"

namespace jd {

constexpr int PI_TX = 64, PI_TY = 16;  // gather tile
constexpr int PI_MAX_P = 16;
constexpr int PI_LROWS = PI_TY + PI_MAX_P - 1, PI_LCOLS = PI_TX + PI_MAX_P - 1;  // patch rows / columns a tile can touch

struct GmmPriorImageArgs {
  const float* normed;    // n(flux), (H, W), un-rolled
  const int32_t* winner;  // per patch (row-major over the grid): component or -1
  float* mean;            // per patch: written by the mean kernel, read by the gather
  const float* table;     // (K, P, P)
  float* out;             // (H, W)
  int K, H, W, stride, nPy, nPx, shift_y, shift_x;
  const int* shift_dev;  // nullable, device [2] = {shift_y, shift_x} residues: read instead of the two members above (use_device_shift)
  float scale;
  int accumulate;
  float4 profile[PI_MAX_P / 4];  // the trapezoid profile of the pixel weights, w[dy][dx] = (profile[dy] * profile[dx]) * wscale
  float wscale;
  ImageNormArgs norm;
};

template <int PP>
__global__ __launch_bounds__(256) void gmm_patch_mean_kernel(GmmPriorImageArgs a) {
  use_device_shift(a);
  const int n = blockIdx.x * 256 + threadIdx.x;
  if (n >= a.nPy * a.nPx) return;
  if (a.winner[n] < 0) {  // a filtered patch adds nothing
    a.mean[n] = 0.f;
    return;
  }
  const int py = n / a.nPx, px = n - py * a.nPx;
  int xx[PP];
#pragma unroll
  for (int c = 0; c < PP; ++c) xx[c] = wrap(px * a.stride + c - a.shift_x, a.W);
  float total = 0.f;
  for (int r = 0; r < PP; ++r) {
    const float* row = a.normed + (size_t)wrap(py * a.stride + r - a.shift_y, a.H) * a.W;
    float sum = row[xx[0]];
#pragma unroll
    for (int c = 1; c < PP; ++c) sum += row[xx[c]];
    total += sum;
  }
  a.mean[n] = total * (1.f / (PP * PP));
}

// profile[d] without a dynamic index into the kernel arguments (that would move them to scratch)
__device__ __forceinline__ float profile_at(const GmmPriorImageArgs& a, int d) {
  const float lo = d < 4 ? f4_get(a.profile[0], d & 3) : f4_get(a.profile[1], d & 3);
  const float hi = d < 12 ? f4_get(a.profile[2], d & 3) : f4_get(a.profile[3], d & 3);
  return d < 8 ? lo : hi;
}

// first patch index whose P pixels at stride s reach pixel v: ceil((v - P + 1) / s), not below 0
__device__ __forceinline__ int first_patch(int v, int patch, int s) {
  const int t = v - patch + 1;
  return t <= 0 ? 0 : (t + s - 1) / s;
}

template <int PP, int KIND>
__global__ __launch_bounds__(256) void gmm_prior_image_gather_kernel(GmmPriorImageArgs a) {
#pragma clang fp contract(off)  // (scale * n^-1(R) is rounded before it is added; the sum over the patches is fmaf by name)
  __shared__ int32_t Lk[PI_LROWS * PI_LCOLS];
  __shared__ float Lm[PI_LROWS * PI_LCOLS];
  __shared__ float Lw[PP * PP];
  use_device_shift(a);
  const int s = a.stride, H = a.H, W = a.W;
  const int X0 = blockIdx.x * PI_TX, Y0 = blockIdx.y * PI_TY;
  // the patches that reach the tile: rows [i_lo, i_lo + ni), columns [j_lo, j_lo + nj) (none: ni <= 0 or nj <= 0)
  const int i_lo = first_patch(Y0, PP, s), j_lo = first_patch(X0, PP, s);
  const int ni = min(a.nPy - 1, (min(Y0 + PI_TY, H) - 1) / s) - i_lo + 1;
  const int nj = min(a.nPx - 1, (min(X0 + PI_TX, W) - 1) / s) - j_lo + 1;
  if (ni > 0 && nj > 0) {
    for (int t = threadIdx.x; t < ni * nj; t += 256) {
      const int ii = t / nj, jj = t - ii * nj;
      const int n = (i_lo + ii) * a.nPx + j_lo + jj;
      Lk[t] = a.winner[n];
      Lm[t] = a.mean[n];
    }
  }
  if (threadIdx.x < PP * PP) {
    Lw[threadIdx.x] = (profile_at(a, threadIdx.x / PP) * profile_at(a, threadIdx.x % PP)) * a.wscale;
  }
  __syncthreads();
  const int X = X0 + (threadIdx.x & 63);
  if (X >= W) return;
  const int j_a = first_patch(X, PP, s), j_b = min(a.nPx - 1, X / s);
  const int x = wrap(X - a.shift_x, W);
  const ImageNormArgs nm = a.norm;
#pragma unroll
  for (int q = 0; q < PI_TY / 4; ++q) {
    const int Y = Y0 + (threadIdx.x >> 6) + 4 * q;
    if (Y >= H) break;
    const int i_a = first_patch(Y, PP, s), i_b = min(a.nPy - 1, Y / s);
    float acc = 0.f;
    for (int i = i_a; i <= i_b; ++i) {
      const int dy = Y - i * s;
      const int lrow = (i - i_lo) * nj - j_lo;
      for (int j = j_a; j <= j_b; ++j) {
        const int dx = X - j * s;
        const int k = Lk[lrow + j];
        if ((unsigned)k < (unsigned)a.K)
          acc = fmaf(Lw[dy * PP + dx], a.table[(k * PP + dy) * PP + dx] + Lm[lrow + j], acc);
      }
    }
    const float v = a.scale * image_norm_inverse<KIND>(acc, nm);
    float* dst = a.out + (size_t)wrap(Y - a.shift_y, H) * W + x;
    *dst = a.accumulate ? *dst + v : v;
  }
}

// the trapezoid profile of get_pixel_weights((P, P), stride) and stride^2 / (its sum)^2, in float64 as numpy forms them
// (utils/numpy.py:37-79; 1 <= stride < P): x = d - (P - 1) / 2, a flat top of width stride - overlap (none where that is
// negative), flanks of slope 1 / overlap
static void pixel_weight_profile(int patch, int stride, float* profile, float* wscale) {
  const double overlap = patch - stride, width = stride - overlap, slope = 1.0 / overlap;
  const double top_lo = std::min(-0.5 * width, 0.0), top_hi = std::max(0.5 * width, 0.0);
  const double foot_lo = top_lo - 1.0 / slope, foot_hi = top_hi + 1.0 / slope;
  double sum = 0.0;
  for (int d = 0; d < PI_MAX_P; ++d) {
    const double x = d - 0.5 * (patch - 1.0);
    double v = 0.0;
    if (d < patch) {
      if (x >= foot_lo && x < top_lo) v = slope * (x - foot_lo);
      else if (x >= top_lo && x < top_hi) v = 1.0;
      else if (x >= top_hi && x < foot_hi) v = slope * (foot_hi - x);
    }
    profile[d] = (float)v;
    sum += v;
  }
  *wscale = (float)((double)stride * stride / (sum * sum));
}

template <int PP>
static bool launch_prior_image(const GmmPriorImageArgs& a, hipStream_t s) {
  const int n = a.nPy * a.nPx;
  const dim3 grid((a.W + PI_TX - 1) / PI_TX, (a.H + PI_TY - 1) / PI_TY);
  ProfScope prof(JD_KERNEL_GMM_GATHER, s);  // (the value-only pass in front has no gather: the scope times these two launches)
  gmm_patch_mean_kernel<PP><<<(n + 255) / 256, 256, 0, s>>>(a);
  return dispatch_norm_kind(a.norm.kind, [&](auto kind) {
    gmm_prior_image_gather_kernel<PP, decltype(kind)::value><<<grid, 256, 0, s>>>(a);
  });
}

}  // namespace jd

using namespace jd;

extern "C" int jd_gmm_prior_image(jd_gmm* g, const float* flux, int H, int W, int stride, int shift_y, int shift_x,
                                  const float* patch_images, float scale, float* image_accum, int accumulate,
                                  const int* shift_dev, void* stream) {
  JD_REQUIRE(g && flux && patch_images && image_accum, "jd_gmm_prior_image: null argument");
  JD_REQUIRE(g->patch_norm == PATCH_NORM_SUBTRACT_MEAN,
             "jd_gmm_prior_image: the prior image adds back the patch mean only: no standardized patch norm");
  const int patch = g->d256 ? 16 : P;
  JD_REQUIRE(H >= patch && W >= patch, "jd_gmm_prior_image: image (%d, %d) smaller than a patch", H, W);
  JD_REQUIRE(stride >= 1 && stride < patch, "jd_gmm_prior_image: stride = %d not in [1, %d] (the pixel weights need an overlap)",
             stride, patch - 1);
  const int nPy = (H - patch) / stride + 1, nPx = (W - patch) / stride + 1;
  JD_REQUIRE((long)nPy * nPx < (1L << 31), "jd_gmm_prior_image: too many patches");
  JD_REQUIRE((H + PI_TY - 1) / PI_TY <= 65535, "jd_gmm_prior_image: image %d x %d too large", H, W);
  hipStream_t s = as_stream(stream);
  jd_gmm::PriorImage& pi = g->prior_image;
  const size_t n = (size_t)nPy * nPx;
  int rc;
  if ((rc = pi.winner.reserve(n)) || (rc = pi.mean.reserve(n)) || (rc = pi.value.reserve(1))) return rc;
  g->pass.valid = false;  // (a phase 1 waiting for its gather does not survive another pass of the handle)

  // pass: the unchanged max-mode forward pass under the handle's norm; its value is not used.  Under a norm it leaves
  // n(flux) in the handle's image
  const ImageNormArgs norm = g->norm;
  if ((rc = gmm_prior_whole(g, norm, flux, H, W, stride, shift_y, shift_x, 0, 0.f, pi.value.ptr, 0, 0.f, nullptr, pi.winner.ptr,
                            shift_dev, stream)))
    return rc;

  GmmPriorImageArgs a{};
  a.normed = norm.kind != NORM_IDENTITY ? g->normed.ptr : flux;
  a.winner = pi.winner.ptr, a.mean = pi.mean.ptr, a.table = patch_images, a.out = image_accum;
  a.K = g->K, a.H = H, a.W = W, a.stride = stride, a.nPy = nPy, a.nPx = nPx;
  a.shift_y = roll_residue(shift_y, H), a.shift_x = roll_residue(shift_x, W), a.shift_dev = shift_dev;
  a.scale = scale, a.accumulate = accumulate ? 1 : 0, a.norm = norm;
  float profile[PI_MAX_P];
  pixel_weight_profile(patch, stride, profile, &a.wscale);
  for (int q = 0; q < PI_MAX_P / 4; ++q)
    a.profile[q] = make_float4(profile[4 * q], profile[4 * q + 1], profile[4 * q + 2], profile[4 * q + 3]);
  const bool known = g->d256 ? launch_prior_image<16>(a, s) : launch_prior_image<P>(a, s);
  JD_REQUIRE(known, "jd_gmm_prior_image: image norm kind %d has no kernel", norm.kind);
  JD_LAUNCH_CHECK();
  return JD_OK;
}
