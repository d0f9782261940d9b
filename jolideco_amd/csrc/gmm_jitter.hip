// Jittered patch grid of the GMM patch prior (jolideco/priors/patches/core.py:189-220 with `jitter`; utils/torch.py:278-334):
// behind the norm and the roll every patch row i and every patch column j is moved by a draw of its own,
//   patch (i, j) = rolled_normed[py_i : py_i + P, px_j : px_j + P],   py_i = overlap + i s + jitter_y[i],   px_j likewise.
// Two streaming kernels around the unchanged pass.  The stage kernel lays the patches side by side, without overlap,
//   S[i P + a, j P + b] = n(flux[(py_i + a - sy) mod H, (px_j + b - sx) mod W]),
// gmm_prior_whole runs on S (shape (n_y P, n_x P), stride P, no roll, identity norm, the handle's patch norm) with its
// gradient G = grad_coef d(sum v_patch)/dS going to a zeroed image, and the adjoint kernel gathers per flux pixel, with
// (Y, X) = ((y + sy) mod H, (x + sx) mod W),
//   grad[y, x] += n'(flux[y, x]) sum_{i: 0 <= Y - py_i < P} sum_{j: 0 <= X - px_j < P} G[i P + (Y - py_i), j P + (X - px_j)]
// i ascending, then j ascending; no atomics, one read-modify-write per pixel: run-to-run identical.  A pixel whose sum is
// exactly 0 -- no patch covers it, or the terms cancel -- is not written.
//
// Stage: one thread per 4 consecutive columns of S (P is 8 or 16: a group lies in one patch), 16-byte stores of S and of the
// zeros of G; the flux is read through a non-negative mod, so no value of a jitter array can make it read outside.
// Adjoint: tiles of 16 x 64 flux pixels, 256 threads, 4 pixels of a row per thread.  The rows (columns) of S that hold a
// pixel row (column) of the tile -- `jitter_cover` of jd_jitter.h: the candidates of the bounded window that do cover -- go to
// LDS once (at most 4 entries each on a safe axis); a thread then walks its row list and per entry issues the 16 loads of G of
// its four pixels together -- list entries beyond a list's length are a valid index -- and adds them under a mask
// (DESIGN_LOG.md, "What the compiler made of the loads").
#include "gmm_internal.h"
#include "jd_jitter.h"

namespace jd {

constexpr int GJ_TX = 64, GJ_TY = 16;  // adjoint tile: 16 groups of 4 columns x 16 rows = 256 threads
// The longest cover list of a SAFE axis: the last base position L obeys L + stride >= n - stride - overlap (it is the last)
// and L + overlap <= n - P (safe), hence overlap <= stride, stride >= P / 2, and jitter_window_max <= (2 P - 1) / (P / 2) + 1.
constexpr int GJ_MAXC = 4;

struct GmmJitterArgs {
  const float* flux;         // the raw flux (stage: source | adjoint under a norm: n')
  float* S;                  // stage: the staged image (n_y P, n_x P)
  float* G;                  // stage: zeroed (nullable) | adjoint: read
  float* grad;               // adjoint: the caller's gradient image (H, W)
  const int* jitter_y;       // device [n_y], [n_x]: the draws (clamped to [-overlap, overlap] where they are read)
  const int* jitter_x;
  int H, W, P, stride, n_y, n_x;
  int shift_y, shift_x;      // roll residues in [0, H) x [0, W)
  const int* shift_dev;      // nullable, device [2] = {shift_y, shift_x} residues: read instead of the two members above
  ImageNormArgs norm;
};

template <int KIND>
__global__ __launch_bounds__(256) void gmm_jitter_stage_kernel(GmmJitterArgs a) {
#pragma clang fp contract(off)
  const int SW = a.n_x * a.P, SH = a.n_y * a.P;
  const int c = 4 * (blockIdx.x * 64 + (threadIdx.x & 63)), r = blockIdx.y * 4 + (threadIdx.x >> 6);
  if (r >= SH || c >= SW) return;
  use_device_shift(a);
  const int H = a.H, W = a.W, P = a.P, sy = a.shift_y, sx = a.shift_x;
  const int i = r / P, j = c / P;  // (c % 4 == 0 and P % 4 == 0: the four columns are one patch's)
  const int Y = jitter_pos(i, P, a.stride, a.jitter_y[i]) + (r - i * P);
  const int X = jitter_pos(j, P, a.stride, a.jitter_x[j]) + (c - j * P);
  const float* row = a.flux + (size_t)jitter_mod(Y - sy, H) * W;
  const int x0 = jitter_mod(X - sx, W);
  int x[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) x[e] = x0 + e >= W ? x0 + e - W : x0 + e;  // (W >= P >= 8 > 4: one wrap at most)
  float f[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) f[e] = row[x[e]];
  const ImageNormArgs nm = a.norm;
  float4 q;
  q.x = image_norm_value<KIND>(f[0], nm), q.y = image_norm_value<KIND>(f[1], nm);
  q.z = image_norm_value<KIND>(f[2], nm), q.w = image_norm_value<KIND>(f[3], nm);
  const size_t at = (size_t)r * SW + c;  // (SW % 8 == 0 and the buffers are the handle's own: 16-byte aligned)
  *reinterpret_cast<float4*>(a.S + at) = q;
  if (a.G) *reinterpret_cast<float4*>(a.G + at) = make_float4(0.f, 0.f, 0.f, 0.f);
}

// g + sum * n'(f), the product rounded; g itself, bit for bit, for an exact zero sum (n' may be infinite there): the
// gather's rule with the coefficient already inside G
template <bool NORM>
__device__ __forceinline__ float jitter_add(float g, float sum, float f, const ImageNormArgs& nm) {
#pragma clang fp contract(off)
  return sum == 0.f ? g : g + normed_sum<NORM>(sum, f, nm);
}

template <bool NORM, bool VEC>
__global__ __launch_bounds__(256) void gmm_jitter_adjoint_kernel(GmmJitterArgs a) {
#pragma clang fp contract(off)
  // cover lists of the tile's rows and columns: rows (columns) of S, entries beyond a list's length are 0 (a valid index)
  __shared__ int row_s[GJ_MAXC][GJ_TY], col_s[GJ_MAXC][GJ_TX];
  __shared__ int row_n[GJ_TY], col_n[GJ_TX];
  use_device_shift(a);
  const int H = a.H, W = a.W, P = a.P, sy = a.shift_y, sx = a.shift_x;
  const int tx0 = blockIdx.x * GJ_TX, ty0 = blockIdx.y * GJ_TY;
  const int t = threadIdx.x;
  if (t < GJ_TY + GJ_TX) {
    const bool is_row = t < GJ_TY;
    const int l = is_row ? t : t - GJ_TY;
    const int p = is_row ? ty0 + l : tx0 + l, n = is_row ? H : W;
    int* list = is_row ? &row_s[0][l] : &col_s[0][l];
    const int lstride = is_row ? GJ_TY : GJ_TX;
    int cnt = 0;
    if (p < n)
      cnt = jitter_cover(jitter_mod(p + (is_row ? sy : sx), n), P, a.stride, is_row ? a.n_y : a.n_x,
                         is_row ? a.jitter_y : a.jitter_x, list, lstride);
    for (int c = cnt; c < GJ_MAXC; ++c) list[c * lstride] = 0;
    (is_row ? row_n : col_n)[l] = cnt;
  }
  __syncthreads();
  const int c4 = t & 15, r0 = t >> 4;
  const int y = ty0 + r0, x = tx0 + 4 * c4;
  if (y >= H || x >= W) return;
  const int SW = a.n_x * P;
  const int rn = row_n[r0];
  int cn[4];
#pragma unroll
  for (int e = 0; e < 4; ++e) cn[e] = col_n[4 * c4 + e];  // (0 for a column beyond W)
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
  for (int ci = 0; ci < rn; ++ci) {
    const float* Grow = a.G + (size_t)row_s[ci][r0] * SW;
    // the 16 loads of the thread's four pixels together: every list entry is a valid column of S (0 beyond its length)
    float v[4][GJ_MAXC];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int k = 0; k < GJ_MAXC; ++k) v[e][k] = Grow[col_s[k][4 * c4 + e]];
#pragma unroll
    for (int e = 0; e < 4; ++e)
#pragma unroll
      for (int k = 0; k < GJ_MAXC; ++k) sum[e] = k < cn[e] ? sum[e] + v[e][k] : sum[e];
  }
  if (sum[0] == 0.f && sum[1] == 0.f && sum[2] == 0.f && sum[3] == 0.f) return;  // nothing to add: not touched
  float* dst = a.grad + (size_t)y * W + x;
  const float* raw = NORM ? a.flux + (size_t)y * W + x : nullptr;
  const ImageNormArgs nm = a.norm;
  if (VEC) {
    float4 q = *reinterpret_cast<float4*>(dst);
    float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
    if (NORM) f = *reinterpret_cast<const float4*>(raw);
    q.x = jitter_add<NORM>(q.x, sum[0], f.x, nm), q.y = jitter_add<NORM>(q.y, sum[1], f.y, nm);
    q.z = jitter_add<NORM>(q.z, sum[2], f.z, nm), q.w = jitter_add<NORM>(q.w, sum[3], f.w, nm);
    *reinterpret_cast<float4*>(dst) = q;
  } else {
#pragma unroll
    for (int e = 0; e < 4; ++e)
      if (x + e < W && sum[e] != 0.f) dst[e] = jitter_add<NORM>(dst[e], sum[e], NORM ? raw[e] : 0.f, nm);
  }
}

}  // namespace jd

using namespace jd;

extern "C" int jd_gmm_prior_jitter_fwd_bwd(jd_gmm* g, const float* flux, int H, int W, int stride, int shift_y, int shift_x,
                                           const int* jitter_y_dev, const int* jitter_x_dev, int marginalize,
                                           float value_scale, float* value_out, int accumulate_value, float grad_coef,
                                           float* grad_flux_accum, int32_t* argmax_out, const int* shift_dev, void* stream) {
  JD_REQUIRE(g && flux && value_out && jitter_y_dev && jitter_x_dev, "jd_gmm_prior_jitter_fwd_bwd: null argument");
  const int patch = g->d256 ? 16 : P;
  JD_REQUIRE(stride >= 1 && stride <= patch, "jd_gmm_prior_jitter_fwd_bwd: stride = %d not in [1, %d]", stride, patch);
  JD_REQUIRE(H >= patch && W >= patch, "jd_gmm_prior_jitter_fwd_bwd: image (%d, %d) smaller than a patch", H, W);
  const int n_y = jitter_count(H, patch, stride), n_x = jitter_count(W, patch, stride);
  JD_REQUIRE(n_y > 0 && n_x > 0, "jd_gmm_prior_jitter_fwd_bwd: image (%d, %d) has no jittered patch at stride %d", H, W, stride);
  JD_REQUIRE(jitter_safe(H, patch, stride) && jitter_safe(W, patch, stride),
             "jd_gmm_prior_jitter_fwd_bwd: image (%d, %d) is not safe at stride %d: a draw can push a patch outside", H, W,
             stride);
  // (the adjoint kernel's LDS lists: safe implies stride >= P / 2, so this cannot fire behind the check above)
  JD_REQUIRE(jitter_window_max(patch, stride) <= GJ_MAXC, "jd_gmm_prior_jitter_fwd_bwd: cover list of %d entries",
             jitter_window_max(patch, stride));
  const size_t n = (size_t)n_y * patch * (size_t)n_x * patch;
  JD_REQUIRE(n < ((size_t)1 << 31), "jd_gmm_prior_jitter_fwd_bwd: the staged image of (%d, %d) has 2^31 elements or more", H, W);
  const int SH = n_y * patch, SW = n_x * patch;
  const dim3 grid_s((SW / 4 + 63) / 64, (SH + 3) / 4), grid_a((W + GJ_TX - 1) / GJ_TX, (H + GJ_TY - 1) / GJ_TY);
  JD_REQUIRE(grid_s.y <= 65535 && grid_a.y <= 65535, "jd_gmm_prior_jitter_fwd_bwd: image %d x %d too large", H, W);
  hipStream_t s = as_stream(stream);
  int rc;
  if ((rc = g->reserve_staged(n, grad_flux_accum != nullptr))) return rc;
  float* const S = g->normed.ptr;
  float* const G = grad_flux_accum ? g->staged_grad.ptr : nullptr;
  const ImageNormArgs norm = g->norm;
  const bool has_norm = norm.kind != NORM_IDENTITY;

  // stage: S = the patches of n(flux) side by side, G = 0
  GmmJitterArgs a{};
  a.flux = flux, a.S = S, a.G = G, a.grad = grad_flux_accum, a.jitter_y = jitter_y_dev, a.jitter_x = jitter_x_dev;
  a.H = H, a.W = W, a.P = patch, a.stride = stride, a.n_y = n_y, a.n_x = n_x;
  a.shift_y = roll_residue(shift_y, H), a.shift_x = roll_residue(shift_x, W), a.shift_dev = shift_dev;
  a.norm = norm;
  const bool known = dispatch_norm_kind(
      norm.kind, [&](auto kind) { gmm_jitter_stage_kernel<decltype(kind)::value><<<grid_s, 256, 0, s>>>(a); });
  JD_REQUIRE(known, "jd_gmm_prior_jitter_fwd_bwd: image norm kind %d has no kernel", norm.kind);
  JD_LAUNCH_CHECK();

  // pass: the whole prior on S, whose patches lie on a regular grid of stride P, under the identity (S is normed already;
  // the chain rule of n is the adjoint kernel's), the handle's patch norm, no roll
  rc = gmm_prior_whole(g, ImageNormArgs{}, S, SH, SW, patch, 0, 0, marginalize, value_scale, value_out, accumulate_value,
                       grad_coef, G, argmax_out, nullptr, stream);
  if (rc || !G) return rc;

  // adjoint: the caller's gradient += n'(flux) * the sum of G over the patches that cover the pixel
  const bool vec = W % 4 == 0 && aligned16(grad_flux_accum) && (!has_norm || aligned16(flux));
  dispatch_bools(has_norm, vec, [&](auto with_norm, auto with_vec) {
    gmm_jitter_adjoint_kernel<decltype(with_norm)::value, decltype(with_vec)::value><<<grid_a, 256, 0, s>>>(a);
  });
  JD_LAUNCH_CHECK();
  return JD_OK;
}
