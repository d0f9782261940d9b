// Sparse point-source flux component (reference: jolideco/models/core.py:54-342, utils/torch.py:31-38): a list of
// sources (flux_n, x_n, y_n) rendered onto the (H, W) grid with the bilinear weights of `grid_weights`,
//   image[y, x] = sum_n (wx_n(x) * wy_n(y)) * f_n,   w(t) = 1 - |t - t0| where |t - t0| < 1, else 0,
// and the gradient of a loss with respect to the three parameter vectors, given its gradient image.
//
// A source touches the pixels {floor(x_n), floor(x_n) + 1} x {floor(y_n), floor(y_n) + 1} (its four TAPS) at most: for every
// other integer t the float32 difference |t - x_n| is >= 1 (rounding is monotonic and 1 is representable).  A tap whose
// weight is 0 on either axis (a coordinate that is exactly an integer, or so close below one that the difference rounds to
// 1) does not touch its pixel, like the zero the reference's `torch.where` puts there.
#include "jd_common.h"
#include "kernels.h"

namespace jd {

constexpr int SPARSE_BLOCK = 256;
constexpr int SPARSE_CHUNK = 1024;      // sources staged in LDS at a time: 12 KiB
constexpr int SPARSE_TRIP = 8;          // sources per trip of the render's walk
constexpr float SPARSE_FAR = 3.0e38f;   // coordinate of the padding behind the last source of a chunk: no pixel is near
static_assert(SPARSE_CHUNK % SPARSE_TRIP == 0 && SPARSE_TRIP % 4 == 0, "a chunk is whole trips of 16-byte reads");
constexpr int SPARSE_MAX_N = 1 << 16;   // the render tests every tap against every source: O(n^2)
constexpr int SPARSE_MAX_SIDE = 1 << 24;  // pixel indices are exact in float32

// w(t) of one axis, in the reference's float32 operations one by one; `d` is |t - t0|
__device__ __forceinline__ float sparse_weight(int t, float t0, float& d) {
#pragma clang fp contract(off)
  d = fabsf((float)t - t0);
  return d < 1.f ? 1.f - d : 0.f;
}

// a coordinate with no pixel of [0, size) within one pixel (NaN and infinities included): the source has no tap there
__device__ __forceinline__ bool sparse_axis_inside(float t0, int size) { return t0 > -1.f && t0 < (float)size; }

__global__ __launch_bounds__(SPARSE_BLOCK) void sparse_zero_kernel(float* __restrict__ out, size_t n, size_t n4) {
  const size_t stride = (size_t)gridDim.x * SPARSE_BLOCK;
  const size_t i0 = (size_t)blockIdx.x * SPARSE_BLOCK + threadIdx.x;
  for (size_t i = i0; i < n4; i += stride) gst4(out + 4 * i, make_float4(0.f, 0.f, 0.f, 0.f));
  for (size_t i = 4 * n4 + i0; i < n; i += stride) out[i] = 0.f;
}

// One thread per (source, tap).  The thread of the LOWEST source index that touches a pixel owns it: it adds the
// contributions of all sources to that pixel in ascending index order and stores the sum -- one store per touched pixel, no
// atomics, the reference's order of summation.  A thread that meets a lower-index source on its pixel gives up; the owner
// is the only one that reaches the end of the list.  The walk is bound by the latency of the LDS reads, not by their number
// (a few waves per CU, each on a serial loop): eight sources per trip -- four 16-byte reads in flight, one branch for the
// rare trip in which a source touches the pixel.
__global__ __launch_bounds__(SPARSE_BLOCK) void sparse_render_kernel(const float* __restrict__ param, const float* __restrict__ xs,
                                                                     const float* __restrict__ ys, int n, int linear, int H, int W,
                                                                     float* __restrict__ out) {
#pragma clang fp contract(off)
  __shared__ __attribute__((aligned(16))) float sx[SPARSE_CHUNK], sy[SPARSE_CHUNK], sf[SPARSE_CHUNK];
  const int g = blockIdx.x * SPARSE_BLOCK + threadIdx.x;
  const int self = g >> 2, tap = g & 3;
  int px = 0, py = 0;
  bool active = false;
  if (self < n) {
    const float x0 = xs[self], y0 = ys[self];
    if (sparse_axis_inside(x0, W) && sparse_axis_inside(y0, H)) {
      px = (int)floorf(x0) + (tap & 1), py = (int)floorf(y0) + (tap >> 1);
      if (px >= 0 && px < W && py >= 0 && py < H) {
        float dx, dy;
        const float wx = sparse_weight(px, x0, dx), wy = sparse_weight(py, y0, dy);
        active = wx > 0.f && wy > 0.f;
      }
    }
  }
  const float fx = (float)px, fy = (float)py;
  float acc = 0.f;
  // (sources behind the last one of this block cannot own a pixel of it, but they contribute: the whole list is walked)
  for (int base = 0; base < n; base += SPARSE_CHUNK) {
    const int count = min(SPARSE_CHUNK, n - base);
    const int padded = (count + SPARSE_TRIP - 1) / SPARSE_TRIP * SPARSE_TRIP;  // (SPARSE_CHUNK is a multiple of a trip)
    __syncthreads();
    for (int i = threadIdx.x; i < padded; i += SPARSE_BLOCK) {
      if (i < count) {
        const float p = param[base + i];
        sx[i] = xs[base + i], sy[i] = ys[base + i], sf[i] = linear ? p : expf(p);
      } else {
        sx[i] = sy[i] = SPARSE_FAR, sf[i] = 0.f;  // (touches no pixel)
      }
    }
    __syncthreads();
    if (!active) continue;
    for (int i = 0; i < padded && active; i += SPARSE_TRIP) {
      float dx[SPARSE_TRIP], dy[SPARSE_TRIP];
#pragma unroll
      for (int q = 0; q < SPARSE_TRIP; q += 4) {
        const float4 X = *reinterpret_cast<const float4*>(&sx[i + q]), Y = *reinterpret_cast<const float4*>(&sy[i + q]);
        dx[q] = fabsf(fx - X.x), dx[q + 1] = fabsf(fx - X.y), dx[q + 2] = fabsf(fx - X.z), dx[q + 3] = fabsf(fx - X.w);
        dy[q] = fabsf(fy - Y.x), dy[q + 1] = fabsf(fy - Y.y), dy[q + 2] = fabsf(fy - Y.z), dy[q + 3] = fabsf(fy - Y.w);
      }
      unsigned hit = 0;  // (bit k: source i + k touches the pixel; no short-circuit: one branch per trip)
#pragma unroll
      for (int k = 0; k < SPARSE_TRIP; ++k) hit |= (unsigned)((dx[k] < 1.f) & (dy[k] < 1.f)) << k;
      if (hit == 0) continue;
#pragma unroll
      for (int k = 0; k < SPARSE_TRIP; ++k) {
        if (active && (hit >> k & 1)) {
          if (base + i + k < self) {
            active = false;  // a lower-index source owns this pixel
          } else {
            const float w = (1.f - dx[k]) * (1.f - dy[k]);  // (both factors > 0: d < 1)
            acc = acc + w * sf[i + k];
          }
        }
      }
    }
  }
  if (active) out[(size_t)py * W + px] = acc;
}

// One thread per source: its <= 4 taps of the gradient image G (0 for a tap outside the image), in autograd's order of
// operations -- d/d weights = G f; the gradient of a row weight wy_j is the sum of (G f) wx over the row's two taps, and
// d/d y0 = sum_j (that sum) sign(y_j - y0); columns alike; sign(0) = 0, and 0 for a tap with |t - t0| >= 1.  Sums that
// cancel in exact arithmetic (a uniform G) then cancel here too.  d/d f = sum G (wx wy), d/d param = (d/d f) f for log flux.
__global__ __launch_bounds__(SPARSE_BLOCK) void sparse_backward_kernel(const float* __restrict__ param, const float* __restrict__ xs,
                                                                       const float* __restrict__ ys, int n, int linear, int H, int W,
                                                                       const float* __restrict__ G, float* __restrict__ gparam,
                                                                       float* __restrict__ gx, float* __restrict__ gy) {
#pragma clang fp contract(off)
  const int self = blockIdx.x * SPARSE_BLOCK + threadIdx.x;
  if (self >= n) return;
  const float x0 = xs[self], y0 = ys[self], p = param[self];
  const float f = linear ? p : expf(p);
  float gf = 0.f, gxs = 0.f, gys = 0.f;
  if (sparse_axis_inside(x0, W) && sparse_axis_inside(y0, H)) {
    const int ix = (int)floorf(x0), iy = (int)floorf(y0);
    float wx[2], wy[2], sgx[2], sgy[2], gw[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      float dx, dy;
      wx[i] = sparse_weight(ix + i, x0, dx), wy[i] = sparse_weight(iy + i, y0, dy);
      const float tx = (float)(ix + i) - x0, ty = (float)(iy + i) - y0;
      sgx[i] = dx < 1.f ? (tx > 0.f ? 1.f : (tx < 0.f ? -1.f : 0.f)) : 0.f;
      sgy[i] = dy < 1.f ? (ty > 0.f ? 1.f : (ty < 0.f ? -1.f : 0.f)) : 0.f;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int px = ix + i, py = iy + j;
        const bool inside = px >= 0 && px < W && py >= 0 && py < H;
        const float g = inside ? G[(size_t)py * W + px] : 0.f;
        gw[j][i] = g * f;
        gf = gf + g * (wx[i] * wy[j]);
      }
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      gxs = gxs + (gw[0][i] * wy[0] + gw[1][i] * wy[1]) * sgx[i];
      gys = gys + (gw[i][0] * wx[0] + gw[i][1] * wx[1]) * sgy[i];
    }
  }
  gparam[self] = linear ? gf : gf * f;
  gx[self] = gxs;
  gy[self] = gys;
}

}  // namespace jd

using namespace jd;

static int sparse_check(const char* who, const void* a, const void* b, const void* c, int n, int H, int W) {
  JD_REQUIRE(a && b && c, "%s: null argument", who);
  JD_REQUIRE(n >= 1 && n <= SPARSE_MAX_N, "%s: n = %d sources not in [1, %d]", who, n, SPARSE_MAX_N);
  JD_REQUIRE(H > 0 && W > 0, "%s: non-positive shape %d x %d", who, H, W);
  JD_REQUIRE(H <= SPARSE_MAX_SIDE && W <= SPARSE_MAX_SIDE, "%s: image %d x %d too large (a side is at most %d)", who, H, W,
             SPARSE_MAX_SIDE);
  return JD_OK;
}

extern "C" int jd_sparse_max_sources(void) { return SPARSE_MAX_N; }

extern "C" int jd_sparse_render(const float* param_flux, const float* x_pos, const float* y_pos, int n, int use_log_flux,
                                int H, int W, float* flux_out, void* stream) {
  int rc = sparse_check("jd_sparse_render", param_flux, x_pos, y_pos, n, H, W);
  if (rc) return rc;
  JD_REQUIRE(flux_out, "jd_sparse_render: null argument");
  hipStream_t s = as_stream(stream);
  const size_t pixels = (size_t)H * (size_t)W;
  const size_t n4 = (reinterpret_cast<uintptr_t>(flux_out) & 15) == 0 ? pixels / 4 : 0;
  size_t zero_blocks = (n4 + (pixels - 4 * n4) + SPARSE_BLOCK - 1) / SPARSE_BLOCK;
  if (zero_blocks > 8192) zero_blocks = 8192;
  const unsigned blocks = (unsigned)(((size_t)4 * (size_t)n + SPARSE_BLOCK - 1) / SPARSE_BLOCK);
  {
    ProfScope prof(JD_KERNEL_SPARSE_RENDER, s);
    sparse_zero_kernel<<<(unsigned)zero_blocks, SPARSE_BLOCK, 0, s>>>(flux_out, pixels, n4);
    sparse_render_kernel<<<blocks, SPARSE_BLOCK, 0, s>>>(param_flux, x_pos, y_pos, n, use_log_flux ? 0 : 1, H, W, flux_out);
  }
  JD_LAUNCH_CHECK();
  return JD_OK;
}

extern "C" int jd_sparse_backward(const float* param_flux, const float* x_pos, const float* y_pos, int n, int use_log_flux,
                                  int H, int W, const float* grad_flux_image, float* grad_param, float* grad_x,
                                  float* grad_y, void* stream) {
  int rc = sparse_check("jd_sparse_backward", param_flux, x_pos, y_pos, n, H, W);
  if (rc) return rc;
  JD_REQUIRE(grad_flux_image && grad_param && grad_x && grad_y, "jd_sparse_backward: null argument");
  hipStream_t s = as_stream(stream);
  const unsigned blocks = (unsigned)((n + SPARSE_BLOCK - 1) / SPARSE_BLOCK);
  {
    ProfScope prof(JD_KERNEL_SPARSE_BACKWARD, s);
    sparse_backward_kernel<<<blocks, SPARSE_BLOCK, 0, s>>>(param_flux, x_pos, y_pos, n, use_log_flux ? 0 : 1, H, W,
                                                          grad_flux_image, grad_param, grad_x, grad_y);
  }
  JD_LAUNCH_CHECK();
  return JD_OK;
}
