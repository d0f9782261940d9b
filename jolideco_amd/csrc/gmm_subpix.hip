// Sub-pixel cycle spin of the GMM patch prior (jolideco/priors/patches/core.py:189-246 with `cycle_spin_subpix`;
// utils/torch.py:31-38,91-143): the prior is evaluated on s = conv2d(roll(n(flux)), k, "same"), the 3 x 3 cross-correlation
// of the rolled, normed image with the bilinear weights of a shift (x0, y0) in [-0.5, 0.5]^2, ZERO outside the rolled
// image.  Two streaming kernels around the unchanged pass (gmm_prior_whole on the staged image under the identity norm, same
// roll).  With (Y, X) = ((y + sy) mod H, (x + sx) mod W) the rolled position of pixel (y, x):
//
//   stage    S[y, x]     = sum_{a,b in {-1,0,1}} k[a+1][b+1] n[(y+a) mod H, (x+b) mod W] [0 <= Y+a < H] [0 <= X+b < W]
//   adjoint  dflux[y, x] = n'(flux[y, x]) sum_{a,b} k[a+1][b+1] G[(y-a) mod H, (x-b) mod W] [0 <= Y-a < H] [0 <= X-b < W]
//
// i.e. in the frame of the flux the stencil wraps around the image except across the seam the roll puts at row H - sy and
// column W - sx, where the tap is dropped (the reference's zero padding).  G = grad_coef * d(sum of the patch values) / dS
// is what the inner pass accumulates into a zeroed image.
//
// Both kernels: 2-D tiles of GS_TY x GS_TX pixels, 256 threads, a thread owns 4 consecutive pixels of one row.  The tile plus
// a one-pixel halo is staged in LDS with wrapped addressing (the halo is loaded again by the neighbouring block: no block
// reads another's results); the nine additions run in row-major (a, b) order, a dropped tap is skipped; no atomics, one
// write of S / one read-modify-write of the gradient per pixel: run-to-run identical.  VEC: W % 4 == 0 and 16-byte
// aligned images -- a group of 4 pixels is inside the image or outside as a whole and moves in 16-byte accesses.
// HBM traffic: stage 8 B/pixel, adjoint 12 B/pixel (+ 4 under a norm: the raw flux for n').
#include "gmm_internal.h"
#include "jd_subpix.h"

namespace jd {

constexpr int GS_TX = 64, GS_TY = 16;              // tile: 16 groups of 4 columns x 16 rows = 256 threads
constexpr int GS_LW = GS_TX + 2, GS_LH = GS_TY + 2;  // LDS window: tile + 1-pixel halo

struct GmmSubpixArgs {
  const float* src;         // stage: the raw flux | adjoint: G
  float* dst;               // stage: S | adjoint: the caller's gradient image
  const float* raw_flux;    // adjoint under a norm: the raw flux (n')
  int H, W, shift_y, shift_x;  // roll residues in [0, H) x [0, W)
  const int* shift_dev;     // nullable, device [2] = {shift_y, shift_x} residues: read instead of the two members above
  float x0, y0;
  const float* offset_dev;  // nullable, device [2] = {x0, y0}: read instead of the two members above
  ImageNormArgs norm;
};

// L[r][c] = f(src[(ty0 - 1 + r) mod H][(tx0 - 1 + c) mod W]) for every window position a pixel of the image needs: rows up
// to y = H and columns up to x = W (the wrapped neighbours of the last row / column); what lies further out belongs to no
// pixel's stencil and is left 0.  -1 <= y <= H and -1 <= x <= W are in wrap()'s range.
template <bool VEC, class F>
__device__ __forceinline__ void subpix_load_window(float (&L)[GS_LH][GS_LW], const float* __restrict__ src, int H, int W,
                                                   int tx0, int ty0, F&& f) {
  const int c4 = threadIdx.x & 15, r0 = threadIdx.x >> 4;
  for (int r = r0; r < GS_LH; r += 16) {
    const int y = ty0 - 1 + r, x = tx0 + 4 * c4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (y <= H && x <= W) {
      const float* row = src + (size_t)wrap(y, H) * W;
      if (VEC) {
        if (x < W) {
          const float4 q = *reinterpret_cast<const float4*>(row + x);
          v[0] = f(q.x), v[1] = f(q.y), v[2] = f(q.z), v[3] = f(q.w);
        } else {
          v[0] = f(row[0]);  // x == W: the wrapped neighbour of the last column
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (x + i <= W) v[i] = f(row[wrap(x + i, W)]);
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) L[r][1 + 4 * c4 + i] = v[i];
  }
  if (threadIdx.x < 2 * GS_LH) {  // the halo column either side
    const int r = threadIdx.x >> 1, col = (threadIdx.x & 1) ? GS_TX + 1 : 0;
    const int y = ty0 - 1 + r, x = tx0 - 1 + col;
    L[r][col] = (y <= H && x <= W) ? f(src[(size_t)wrap(y, H) * W + wrap(x, W)]) : 0.f;
  }
}

// the roll of the launch into the kernel's own copy of its arguments, and the nine weights of its offsets (device memory first)
__device__ __forceinline__ void subpix_scalars(GmmSubpixArgs& a, float (&k)[3][3]) {
  use_device_shift(a);
  subpix_weights(a.offset_dev ? a.offset_dev[0] : a.x0, a.offset_dev ? a.offset_dev[1] : a.y0, k);
}

template <int KIND, bool VEC>
__global__ __launch_bounds__(256) void gmm_subpix_stage_kernel(GmmSubpixArgs a) {
#pragma clang fp contract(off)
  __shared__ float L[GS_LH][GS_LW];
  const int H = a.H, W = a.W;
  const int tx0 = blockIdx.x * GS_TX, ty0 = blockIdx.y * GS_TY;
  float k[3][3];
  subpix_scalars(a, k);
  const int sy = a.shift_y, sx = a.shift_x;
  const ImageNormArgs nm = a.norm;
  subpix_load_window<VEC>(L, a.src, H, W, tx0, ty0, [&](float f) { return image_norm_value<KIND>(f, nm); });
  __syncthreads();
  const int c4 = threadIdx.x & 15, r0 = threadIdx.x >> 4;
  const int y = ty0 + r0, x = tx0 + 4 * c4;
  if (y >= H || x >= W) return;
  const int Y = wrap(y + sy, H);
  const bool row_ok[3] = {Y >= 1, true, Y + 1 < H};  // tap a - 1 stays inside the rolled image
  float out[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (!VEC && x + e >= W) break;
    const int X = wrap(x + e + sx, W);
    const bool col_ok[3] = {X >= 1, true, X + 1 < W};
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (row_ok[i] && col_ok[j]) s = fmaf(k[i][j], L[r0 + i][4 * c4 + e + j], s);
    out[e] = s;
  }
  float* dst = a.dst + (size_t)y * W + x;
  if (VEC) {
    *reinterpret_cast<float4*>(dst) = make_float4(out[0], out[1], out[2], out[3]);
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (x + e < W) dst[e] = out[e];
  }
}

// (sum of the adjoint stencil) * n'(f), the product rounded; nothing for an exact zero sum (n' may be infinite there) --
// the rule of gather_normed_term with the coefficient already inside G
template <bool NORM>
__device__ __forceinline__ float subpix_normed_term(float sum, float f, const ImageNormArgs& nm) {
#pragma clang fp contract(off)
  return sum == 0.f ? 0.f : normed_sum<NORM>(sum, f, nm);
}

template <bool NORM, bool VEC>
__global__ __launch_bounds__(256) void gmm_subpix_adjoint_kernel(GmmSubpixArgs a) {
#pragma clang fp contract(off)
  __shared__ float L[GS_LH][GS_LW];
  const int H = a.H, W = a.W;
  const int tx0 = blockIdx.x * GS_TX, ty0 = blockIdx.y * GS_TY;
  float k[3][3];
  subpix_scalars(a, k);
  const int sy = a.shift_y, sx = a.shift_x;
  subpix_load_window<VEC>(L, a.src, H, W, tx0, ty0, [](float g) { return g; });
  __syncthreads();
  const int c4 = threadIdx.x & 15, r0 = threadIdx.x >> 4;
  const int y = ty0 + r0, x = tx0 + 4 * c4;
  if (y >= H || x >= W) return;
  const int Y = wrap(y + sy, H);
  const bool row_ok[3] = {Y + 1 < H, true, Y >= 1};  // the pixel (Y - (a - 1)) the tap a - 1 came from is inside
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if (!VEC && x + e >= W) break;
    const int X = wrap(x + e + sx, W);
    const bool col_ok[3] = {X + 1 < W, true, X >= 1};
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        if (row_ok[i] && col_ok[j]) s = fmaf(k[i][j], L[r0 + 2 - i][4 * c4 + e + 2 - j], s);
    sum[e] = s;
  }
  float* dst = a.dst + (size_t)y * W + x;
  const float* raw = NORM ? a.raw_flux + (size_t)y * W + x : nullptr;
  const ImageNormArgs nm = a.norm;
  if (VEC) {
    float4 q = *reinterpret_cast<float4*>(dst);
    float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
    if (NORM) f = *reinterpret_cast<const float4*>(raw);
    q.x += subpix_normed_term<NORM>(sum[0], f.x, nm), q.y += subpix_normed_term<NORM>(sum[1], f.y, nm);
    q.z += subpix_normed_term<NORM>(sum[2], f.z, nm), q.w += subpix_normed_term<NORM>(sum[3], f.w, nm);
    *reinterpret_cast<float4*>(dst) = q;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (x + e < W) dst[e] += subpix_normed_term<NORM>(sum[e], NORM ? raw[e] : 0.f, nm);
  }
}

}  // namespace jd

using namespace jd;

extern "C" int jd_gmm_prior_subpix_fwd_bwd(jd_gmm* g, const float* flux, int H, int W, int stride, int shift_y, int shift_x,
                                           float x0, float y0, int marginalize, float value_scale, float* value_out,
                                           int accumulate_value, float grad_coef, float* grad_flux_accum, int32_t* argmax_out,
                                           const int* shift_dev, const float* offset_dev, void* stream) {
  JD_REQUIRE(g && flux && value_out, "jd_gmm_prior_subpix_fwd_bwd: null argument");
  const int patch = g->d256 ? 16 : P;
  JD_REQUIRE(H >= patch && W >= patch, "jd_gmm_prior_subpix_fwd_bwd: image (%d, %d) smaller than a patch", H, W);
  JD_REQUIRE(stride >= 1 && (g->d256 || stride <= P), "jd_gmm_prior_subpix_fwd_bwd: stride = %d not valid", stride);
  // (the negated form refuses NaN too)
  JD_REQUIRE(offset_dev || (x0 >= -0.5f && x0 <= 0.5f && y0 >= -0.5f && y0 <= 0.5f),
             "jd_gmm_prior_subpix_fwd_bwd: offsets (%g, %g) not in [-0.5, 0.5]", (double)x0, (double)y0);
  const dim3 grid((W + GS_TX - 1) / GS_TX, (H + GS_TY - 1) / GS_TY);
  JD_REQUIRE(grid.y <= 65535, "jd_gmm_prior_subpix_fwd_bwd: image %d x %d too large", H, W);
  hipStream_t s = as_stream(stream);
  const size_t n = (size_t)H * W;
  int rc;
  if ((rc = g->reserve_staged(n, grad_flux_accum != nullptr))) return rc;
  float* const S = g->normed.ptr;
  float* const G = grad_flux_accum ? g->staged_grad.ptr : nullptr;
  const ImageNormArgs norm = g->norm;
  const bool has_norm = norm.kind != NORM_IDENTITY;

  // stage: S = the stencil of n(flux)
  GmmSubpixArgs a{};
  a.H = H, a.W = W, a.shift_y = roll_residue(shift_y, H), a.shift_x = roll_residue(shift_x, W), a.shift_dev = shift_dev;
  a.x0 = x0, a.y0 = y0, a.offset_dev = offset_dev, a.norm = norm;
  a.src = flux, a.dst = S;
  const bool vec_stage = W % 4 == 0 && aligned16(flux) && aligned16(S);
  const bool known = dispatch_norm_kind(norm.kind, [&](auto kind) {
    if (vec_stage)
      gmm_subpix_stage_kernel<decltype(kind)::value, true><<<grid, 256, 0, s>>>(a);
    else
      gmm_subpix_stage_kernel<decltype(kind)::value, false><<<grid, 256, 0, s>>>(a);
  });
  JD_REQUIRE(known, "jd_gmm_prior_subpix_fwd_bwd: image norm kind %d has no kernel", norm.kind);
  JD_LAUNCH_CHECK();

  // pass: the whole prior on S under the identity (S is normed already; the chain rule of n is the adjoint kernel's), the
  // handle's patch norm, the same roll; its gradient goes to the zeroed G
  if (G) JD_HIP(hipMemsetAsync(G, 0, n * sizeof(float), s));
  rc = gmm_prior_whole(g, ImageNormArgs{}, S, H, W, stride, shift_y, shift_x, marginalize, value_scale, value_out,
                       accumulate_value, grad_coef, G, argmax_out, shift_dev, stream);
  if (rc || !G) return rc;

  // adjoint: the caller's gradient += n'(flux) * the transposed stencil of G
  a.src = G, a.dst = grad_flux_accum, a.raw_flux = flux;
  const bool vec = W % 4 == 0 && aligned16(G) && aligned16(grad_flux_accum) && (!has_norm || aligned16(flux));
  dispatch_bools(has_norm, vec, [&](auto with_norm, auto with_vec) {
    gmm_subpix_adjoint_kernel<decltype(with_norm)::value, decltype(with_vec)::value><<<grid, 256, 0, s>>>(a);
  });
  JD_LAUNCH_CHECK();
  return JD_OK;
}
