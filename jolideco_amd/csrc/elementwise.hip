// HBM-bound element-wise kernels of the MAP step (gfx950): pad*exposure (K1), k-space complex
// multiply (K2), fused clip + background + Poisson NLL + gradient (K3), adjoint epilogue (K5)
// and the element-wise priors (the optimizer step, K6, is optimizer.hip).  All are streaming kernels:
// one pass over each operand, 16 B per lane where the row alignment allows it, fp64 block
// partials + a single fixed-order finalize for every scalar so results are run-to-run identical.
#include <cstdint>
#include <cstdlib>

#include "jd_common.h"
#include "jd_subpix.h"
#include "kernels.h"

namespace jd {

constexpr int BLOCK = 256;

// ------------------------------------------------------------------------------------------
// finalize: out = [out +] scale * sum(partials) + offset   (one block, fixed order)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void finalize_sum_kernel(const double* __restrict__ partials, int n,
                                                            double scale, double offset,
                                                            float* __restrict__ out, int accumulate) {
  __shared__ double smem[BLOCK / 64];
  double acc = 0.0;
  for (int i = threadIdx.x; i < n; i += BLOCK) acc += partials[i];
  double total = block_sum<BLOCK>(acc, smem);
  if (threadIdx.x == 0) {
    double v = scale * total + offset;
    if (accumulate) v += (double)out[0];
    out[0] = (float)v;
  }
}

int launch_finalize_sum(const double* partials, int n, double scale, double offset, float* out,
                        int accumulate, hipStream_t stream) {
  finalize_sum_kernel<<<1, BLOCK, 0, stream>>>(partials, n, scale, offset, out, accumulate);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

struct FinalizeRowsArgs {
  const double* partials;
  int n;
  double scale;
  float offset[SEP_MAX_BATCH];
  float* out[SEP_MAX_BATCH];
};

__global__ __launch_bounds__(BLOCK) void finalize_rows_kernel(FinalizeRowsArgs a) {
  __shared__ double smem[BLOCK / 64];
  const double* row = a.partials + (size_t)blockIdx.x * a.n;
  double acc = 0.0;
  for (int i = threadIdx.x; i < a.n; i += BLOCK) acc += row[i];
  const double total = block_sum<BLOCK>(acc, smem);
  if (threadIdx.x == 0) a.out[blockIdx.x][0] = (float)(a.scale * total + (double)a.offset[blockIdx.x]);
}

int launch_finalize_rows(const double* partials, int n, int n_out, double scale, const float* offset_host,
                         float* const* out, hipStream_t stream) {
  if (n_out < 1 || n_out > SEP_MAX_BATCH) return fail(JD_ERR_INVALID, "finalize_rows: %d outputs not in [1, %d]", n_out, SEP_MAX_BATCH);
  FinalizeRowsArgs a{};
  a.partials = partials, a.n = n, a.scale = scale;
  for (int d = 0; d < n_out; ++d) a.offset[d] = offset_host[d], a.out[d] = out[d];
  finalize_rows_kernel<<<n_out, BLOCK, 0, stream>>>(a);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

// ------------------------------------------------------------------------------------------
// K1: padded[y][x] = image[y][x] * scale[y][x] inside (H, W), 0 in the padding
// ------------------------------------------------------------------------------------------
template <int VEC>
__global__ __launch_bounds__(BLOCK) void pad_mul_kernel(const float* __restrict__ image,
                                                       const float* __restrict__ scale,
                                                       float* __restrict__ padded, int H, int W, int Wp) {
  const int y = blockIdx.y;
  const int x0 = (blockIdx.x * BLOCK + threadIdx.x) * VEC;
  if (x0 >= Wp) return;
  float v[VEC];
#pragma unroll
  for (int i = 0; i < VEC; ++i) v[i] = 0.f;
  if (y < H && x0 < W) {
    const size_t off = (size_t)y * W + x0;
    if constexpr (VEC == 4) {
      // W % 4 == 0 on this path, so x0 < W implies x0 + 3 < W
      const float4 a = *reinterpret_cast<const float4*>(image + off);
      float4 s = make_float4(1.f, 1.f, 1.f, 1.f);
      if (scale) s = *reinterpret_cast<const float4*>(scale + off);
      v[0] = a.x * s.x, v[1] = a.y * s.y, v[2] = a.z * s.z, v[3] = a.w * s.w;
    } else {
      v[0] = image[off] * (scale ? scale[off] : 1.f);
    }
  }
  float* dst = padded + (size_t)y * Wp + x0;
  if constexpr (VEC == 4) {
    *reinterpret_cast<float4*>(dst) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    dst[0] = v[0];
  }
}

int launch_pad_mul(const float* image, const float* scale, float* padded, int H, int W, int Hp, int Wp,
                   hipStream_t stream) {
  const bool vec = (W % 4 == 0) && (Wp % 4 == 0);
  const int per_block = BLOCK * (vec ? 4 : 1);
  dim3 grid((Wp + per_block - 1) / per_block, Hp);
  ProfScope prof(JD_KERNEL_PAD_MUL, stream);
  if (vec)
    pad_mul_kernel<4><<<grid, BLOCK, 0, stream>>>(image, scale, padded, H, W, Wp);
  else
    pad_mul_kernel<1><<<grid, BLOCK, 0, stream>>>(image, scale, padded, H, W, Wp);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

// ------------------------------------------------------------------------------------------
// K2: spec *= khat   or   spec *= conj(khat)     (interleaved complex64)
// ------------------------------------------------------------------------------------------
template <bool CONJ>
__global__ __launch_bounds__(BLOCK) void cmul_kernel(float2* __restrict__ spec,
                                                    const float2* __restrict__ khat, size_t n) {
  const size_t stride = (size_t)gridDim.x * BLOCK * 2;
  for (size_t i = ((size_t)blockIdx.x * BLOCK + threadIdx.x) * 2; i < n; i += stride) {
    if (i + 1 < n) {
      float4 a = *reinterpret_cast<float4*>(spec + i);
      const float4 k = *reinterpret_cast<const float4*>(khat + i);
      const float k1 = CONJ ? -k.y : k.y, k3 = CONJ ? -k.w : k.w;
      float4 r;
      r.x = a.x * k.x - a.y * k1;
      r.y = a.x * k1 + a.y * k.x;
      r.z = a.z * k.z - a.w * k3;
      r.w = a.z * k3 + a.w * k.z;
      *reinterpret_cast<float4*>(spec + i) = r;
    } else {
      const float2 a = spec[i];
      const float2 k = khat[i];
      const float ky = CONJ ? -k.y : k.y;
      spec[i] = make_float2(a.x * k.x - a.y * ky, a.x * ky + a.y * k.x);
    }
  }
}

int launch_cmul(float2* spec, const float2* khat, size_t n, bool conj, hipStream_t stream) {
  size_t blocks = (n / 2 + BLOCK - 1) / BLOCK;
  if (blocks > 8192) blocks = 8192;
  if (blocks == 0) blocks = 1;
  ProfScope prof(JD_KERNEL_CMUL, stream);
  if (conj)
    cmul_kernel<true><<<(unsigned)blocks, BLOCK, 0, stream>>>(spec, khat, n);
  else
    cmul_kernel<false><<<(unsigned)blocks, BLOCK, 0, stream>>>(spec, khat, n);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

// ------------------------------------------------------------------------------------------
// K3: fused clip + sum over components + background + Poisson NLL partial sums + gradient.
// Reads conv_c at the crop offset of the padded grid, writes g_c over the WHOLE padded grid
// (zeros outside (H, W)) so the buffer is directly the input of the adjoint R2C.
// Algorithmic bytes: 16 B/pixel for one component (conv, background, counts in; g out).
// ------------------------------------------------------------------------------------------
// CAL: a dataset calibration is present (background norm read from device memory, second partial sum
// for its gradient); a compile-time switch so that the plain pass carries none of it.
template <int VEC, int ROWS, bool CAL>
__global__ __launch_bounds__(BLOCK) void poisson_fused_kernel(PoissonArgs a) {
  __shared__ double smem[BLOCK / 64];
  const int x0 = (blockIdx.x * BLOCK + threadIdx.x) * VEC;
  double local = 0.0, local_b = 0.0;
  const float bkg_norm = (CAL && a.log_bkg_norm) ? expf(a.log_bkg_norm[0]) : 1.f;  // NPredCalibration.background_norm
  // ROWS rows per thread: every load of the thread is issued before the first one is consumed
  // (ROWS x (2 + n_comp) x 16 B in flight per lane)
  float b[ROWS][VEC], c[ROWS][VEC], conv[ROWS][JD_MAX_COMPONENTS][VEC];
  bool in_image[ROWS];
#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const int y = blockIdx.y * ROWS + r;
    in_image[r] = (y < a.H) && (x0 < a.W);
    if (in_image[r]) {
      const size_t off = (size_t)y * a.W + x0;
      const size_t poff = (size_t)(y + a.oy) * a.Wp + (x0 + a.ox);
      if constexpr (VEC == 4) {
        const float4 bb = *reinterpret_cast<const float4*>(a.background + off);
        const float4 cc = *reinterpret_cast<const float4*>(a.counts + off);
        b[r][0] = bb.x, b[r][1] = bb.y, b[r][2] = bb.z, b[r][3] = bb.w;
        c[r][0] = cc.x, c[r][1] = cc.y, c[r][2] = cc.z, c[r][3] = cc.w;
      } else {
        b[r][0] = a.background[off];
        c[r][0] = a.counts[off];
      }
#pragma unroll
      for (int k = 0; k < JD_MAX_COMPONENTS; ++k) {
        if (k >= a.n_comp) break;
        if constexpr (VEC == 4) {
          const float4 v = *reinterpret_cast<const float4*>(a.conv[k] + poff);
          conv[r][k][0] = v.x, conv[r][k][1] = v.y, conv[r][k][2] = v.z, conv[r][k][3] = v.w;
        } else {
          conv[r][k][0] = a.conv[k][poff];
        }
      }
    }
  }

#pragma unroll
  for (int r = 0; r < ROWS; ++r) {
    const int y = blockIdx.y * ROWS + r;
    float g[VEC];
#pragma unroll
    for (int i = 0; i < VEC; ++i) g[i] = 0.f;
    if (in_image[r]) {
      float n[VEC];
#pragma unroll
      for (int i = 0; i < VEC; ++i) n[i] = 0.f;
#pragma unroll
      for (int k = 0; k < JD_MAX_COMPONENTS; ++k) {
        if (k >= a.n_comp) break;
#pragma unroll
        for (int i = 0; i < VEC; ++i) n[i] += fmaxf(conv[r][k][i], 0.f);  // clip per component, npred.py:191
      }
#pragma unroll
      for (int i = 0; i < VEC; ++i) {
        const float bi = (CAL && a.log_bkg_norm) ? b[r][i] * bkg_norm : b[r][i];
        n[i] += bi;  // background added last, un-convolved (npred.py:234-261)
        float term;
        poisson_point(n[i], c[r][i], a.eps, a.inv_n, term, g[i]);
        local += (double)term;
        if (CAL) local_b += (double)(g[i] * bi);
      }
      if (a.npred_out) {
        const size_t off = (size_t)y * a.W + x0;
        if constexpr (VEC == 4)
          *reinterpret_cast<float4*>(a.npred_out + off) = make_float4(n[0], n[1], n[2], n[3]);
        else
          a.npred_out[off] = n[0];
      }
    }
    if (a.write_grad && x0 < a.Wp && y < a.Hp) {
      const size_t goff = (size_t)y * a.Wp + x0;
#pragma unroll
      for (int k = 0; k < JD_MAX_COMPONENTS; ++k) {
        if (k >= a.n_comp) break;
        float gk[VEC];
#pragma unroll
        for (int i = 0; i < VEC; ++i)
          gk[i] = (in_image[r] && conv[r][k][i] >= 0.f) ? g[i] : 0.f;  // clamp backward: passes where conv >= 0
        if constexpr (VEC == 4)
          *reinterpret_cast<float4*>(a.g[k] + goff) = make_float4(gk[0], gk[1], gk[2], gk[3]);
        else
          a.g[k][goff] = gk[0];
      }
    }
  }

  const double total = block_sum<BLOCK>(local, smem);
  if (threadIdx.x == 0) a.partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
  if (CAL && a.partials_b) {  // wave-uniform
    __syncthreads();
    const double total_b = block_sum<BLOCK>(local_b, smem);
    if (threadIdx.x == 0) a.partials_b[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total_b;
  }
}

int launch_poisson_fused(const PoissonArgs& a, int* n_partials, hipStream_t stream) {
  const bool vec = (a.W % 4 == 0) && (a.Wp % 4 == 0) && (a.ox % 4 == 0);
  const int per_block = BLOCK * (vec ? 4 : 1);
  const int span = a.write_grad ? a.Wp : a.W;
  const int rows = a.write_grad ? a.Hp : a.H;
  int rows_per_block = 1;  // measured on MI355X at 2048^2: 1 row 14.6 us, 2 rows 15.8 us, 4 rows 17.3 us
  {  // tuning override
    const int v = opt_value(OPT_POISSON_ROWS, 0);
    if (vec && (v == 1 || v == 2 || v == 4)) rows_per_block = v;
  }
  dim3 grid((span + per_block - 1) / per_block, (rows + rows_per_block - 1) / rows_per_block);
  *n_partials = grid.x * grid.y;
  ProfScope prof(JD_KERNEL_POISSON_FUSED, stream);
  const bool cal = a.log_bkg_norm != nullptr;
  if (!vec && cal)
    poisson_fused_kernel<1, 1, true><<<grid, BLOCK, 0, stream>>>(a);
  else if (!vec)
    poisson_fused_kernel<1, 1, false><<<grid, BLOCK, 0, stream>>>(a);
  else if (cal)
    poisson_fused_kernel<4, 1, true><<<grid, BLOCK, 0, stream>>>(a);
  else if (rows_per_block == 4)
    poisson_fused_kernel<4, 4, false><<<grid, BLOCK, 0, stream>>>(a);
  else if (rows_per_block == 2)
    poisson_fused_kernel<4, 2, false><<<grid, BLOCK, 0, stream>>>(a);
  else
    poisson_fused_kernel<4, 1, false><<<grid, BLOCK, 0, stream>>>(a);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

// ------------------------------------------------------------------------------------------
// K3 with sum-pooling (upsampling_factor u > 1, jolideco/models/npred.py:181-184): one thread per
// COUNTS pixel sums the u x u block of every component's convolution, clips, adds the background,
// accumulates the Poisson NLL and replicates g = d loss / d npred into the u x u block of g_c (the
// adjoint of the sum-pool), masked where the pooled value was clipped.  The padding of the g buffers
// (FFT method) is already zero: K1 rewrote the whole padded grid before the forward transform.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void poisson_pooled_kernel(PoissonArgs a) {
  __shared__ double smem[BLOCK / 64];
  const int u = a.up;
  const int Hd = a.H / u, Wd = a.W / u;
  const int y = blockIdx.y;
  const int x = blockIdx.x * BLOCK + threadIdx.x;
  double local = 0.0, local_b = 0.0;
  if (y < Hd && x < Wd) {
    const size_t off = (size_t)y * Wd + x;
    float pooled[JD_MAX_COMPONENTS];
    float n = 0.f;
#pragma unroll
    for (int k = 0; k < JD_MAX_COMPONENTS; ++k) {
      if (k >= a.n_comp) break;
      float acc = 0.f;
      for (int dy = 0; dy < u; ++dy) {
        const float* row = a.conv[k] + (size_t)(y * u + dy + a.oy) * a.Wp + (x * u + a.ox);
        for (int dx = 0; dx < u; ++dx) acc += row[dx];
      }
      pooled[k] = acc;
      n += fmaxf(acc, 0.f);  // clip per component after pooling (npred.py:181-191)
    }
    const float bi = a.log_bkg_norm ? a.background[off] * expf(a.log_bkg_norm[0]) : a.background[off];
    n += bi;
    const float c = a.counts[off];
    float term, g;
    poisson_point(n, c, a.eps, a.inv_n, term, g);
    local = (double)term;
    local_b = (double)(g * bi);
    if (a.npred_out) a.npred_out[off] = n;
    if (a.write_grad) {
#pragma unroll
      for (int k = 0; k < JD_MAX_COMPONENTS; ++k) {
        if (k >= a.n_comp) break;
        const float gk = pooled[k] >= 0.f ? g : 0.f;
        for (int dy = 0; dy < u; ++dy) {
          float* row = a.g[k] + (size_t)(y * u + dy) * a.Wp + (size_t)x * u;
          for (int dx = 0; dx < u; ++dx) row[dx] = gk;
        }
      }
    }
  }
  const double total = block_sum<BLOCK>(local, smem);
  if (threadIdx.x == 0) a.partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
  if (a.partials_b) {
    __syncthreads();
    const double total_b = block_sum<BLOCK>(local_b, smem);
    if (threadIdx.x == 0) a.partials_b[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total_b;
  }
}

int launch_poisson_pooled(const PoissonArgs& a, int* n_partials, hipStream_t stream) {
  const int Hd = a.H / a.up, Wd = a.W / a.up;
  dim3 grid((Wd + BLOCK - 1) / BLOCK, Hd);
  *n_partials = grid.x * grid.y;
  ProfScope prof(JD_KERNEL_POISSON_FUSED, stream);
  poisson_pooled_kernel<<<grid, BLOCK, 0, stream>>>(a);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

int poisson_fused_max_partials(int Hp, int Wp) { return ((Wp + BLOCK - 1) / BLOCK) * Hp; }

// ------------------------------------------------------------------------------------------
// K3 for flux components of DIFFERENT up-sampling factors (jd_npred_poisson_mixed_fwd_bwd; models/npred.py:181-191,
// 241-261): one pass over the COUNTS grid.  Component c's convolution lives in its own plan's buffer -- row pitch
// Wp[c], crop offset (oy[c], ox[c]), factor up[c] -- and its gradient goes to that plan's adjoint input: the
// up[c] x up[c] block of every counts pixel receives g, masked where the pooled value was clipped.
// HBM bound: 4 * (2 + sum_c 2 up[c]^2) B per counts pixel with gradients.  Two components with factors 1..4 (the
// diffuse + point-source fits) run an instantiation with both factors known at compile time: every load of a thread
// is issued before the first one is consumed, and with VEC a thread takes TWO neighbouring counts pixels, so that a
// row piece of its blocks is 2 up[c] floats -- loaded and stored as float4 (even factors) or float2 (odd ones).
// Everything else (more components, larger factors) takes the generic kernel below.
// ------------------------------------------------------------------------------------------
template <int N, int V>
__device__ __forceinline__ void load_piece(const float* __restrict__ p, float* out) {
  if constexpr (V == 4) {
#pragma unroll
    for (int i = 0; i < N / 4; ++i) {
      const float4 v = reinterpret_cast<const float4*>(p)[i];
      out[4 * i] = v.x, out[4 * i + 1] = v.y, out[4 * i + 2] = v.z, out[4 * i + 3] = v.w;
    }
  } else if constexpr (V == 2) {
#pragma unroll
    for (int i = 0; i < N / 2; ++i) {
      const float2 v = reinterpret_cast<const float2*>(p)[i];
      out[2 * i] = v.x, out[2 * i + 1] = v.y;
    }
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) out[i] = p[i];
  }
}

template <int N, int V>
__device__ __forceinline__ void store_piece(float* __restrict__ p, const float* in) {
  if constexpr (V == 4) {
#pragma unroll
    for (int i = 0; i < N / 4; ++i)
      reinterpret_cast<float4*>(p)[i] = make_float4(in[4 * i], in[4 * i + 1], in[4 * i + 2], in[4 * i + 3]);
  } else if constexpr (V == 2) {
#pragma unroll
    for (int i = 0; i < N / 2; ++i) reinterpret_cast<float2*>(p)[i] = make_float2(in[2 * i], in[2 * i + 1]);
  } else {
#pragma unroll
    for (int i = 0; i < N; ++i) p[i] = in[i];
  }
}

// vector width of a row piece of P = 2 neighbouring blocks of factor U: 2 U floats starting at a multiple of 2 U
template <int U, bool VEC>
constexpr int piece_vec() { return !VEC ? 1 : (U % 2 == 0 ? 4 : 2); }

// the u x u sums of P neighbouring blocks (rows outer, columns inner: the order of poisson_pooled_kernel)
template <int U, int P>
__device__ __forceinline__ void pool_blocks(const float (&v)[U][P * U], float* pooled) {
#pragma unroll
  for (int i = 0; i < P; ++i) {
    float acc = 0.f;
#pragma unroll
    for (int dy = 0; dy < U; ++dy)
#pragma unroll
      for (int dx = 0; dx < U; ++dx) acc += v[dy][i * U + dx];
    pooled[i] = acc;
  }
}

template <int U, int P, int V>
__device__ __forceinline__ void replicate_blocks(float* __restrict__ g, int Wp, int y, int x0, const float* gk) {
  float row[P * U];
#pragma unroll
  for (int i = 0; i < P; ++i)
#pragma unroll
    for (int dx = 0; dx < U; ++dx) row[i * U + dx] = gk[i];
#pragma unroll
  for (int dy = 0; dy < U; ++dy) store_piece<P * U, V>(g + (size_t)(y * U + dy) * Wp + (size_t)x0 * U, row);
}

template <int U0, int U1, bool VEC>
__global__ __launch_bounds__(BLOCK) void poisson_mixed_kernel(PoissonMixedArgs a) {
  __shared__ double smem[BLOCK / 64];
  constexpr int P = VEC ? 2 : 1;
  constexpr int V0 = piece_vec<U0, VEC>(), V1 = piece_vec<U1, VEC>();
  const int y = blockIdx.y;
  const int x0 = (blockIdx.x * BLOCK + threadIdx.x) * P;
  double local = 0.0;
  if (x0 < a.Wd) {  // (VEC: Wd is even, so x0 + 1 < Wd too)
    const size_t off = (size_t)y * a.Wd + x0;
    float b[P], c[P], v0[U0][P * U0], v1[U1][P * U1];
    load_piece<P, VEC ? 2 : 1>(a.background + off, b);
    load_piece<P, VEC ? 2 : 1>(a.counts + off, c);
#pragma unroll
    for (int dy = 0; dy < U0; ++dy)
      load_piece<P * U0, V0>(a.conv[0] + (size_t)(y * U0 + dy + a.oy[0]) * a.Wp[0] + ((size_t)x0 * U0 + a.ox[0]), v0[dy]);
#pragma unroll
    for (int dy = 0; dy < U1; ++dy)
      load_piece<P * U1, V1>(a.conv[1] + (size_t)(y * U1 + dy + a.oy[1]) * a.Wp[1] + ((size_t)x0 * U1 + a.ox[1]), v1[dy]);

    float p0[P], p1[P], n[P], g[P];
    pool_blocks<U0, P>(v0, p0);
    pool_blocks<U1, P>(v1, p1);
#pragma unroll
    for (int i = 0; i < P; ++i) {
      n[i] = fmaxf(p0[i], 0.f);  // clip per component after pooling (npred.py:181-191)
      n[i] += fmaxf(p1[i], 0.f);
      n[i] += b[i];              // background added last, un-convolved (npred.py:254-261)
      float term;
      poisson_point(n[i], c[i], a.eps, a.inv_n, term, g[i]);
      local += (double)term;
    }
    if (a.npred_out) store_piece<P, VEC ? 2 : 1>(a.npred_out + off, n);
    if (a.write_grad) {
      float gk[P];
#pragma unroll
      for (int i = 0; i < P; ++i) gk[i] = p0[i] >= 0.f ? g[i] : 0.f;  // clamp backward: passes where pooled >= 0
      replicate_blocks<U0, P, V0>(a.g[0], a.Wp[0], y, x0, gk);
#pragma unroll
      for (int i = 0; i < P; ++i) gk[i] = p1[i] >= 0.f ? g[i] : 0.f;
      replicate_blocks<U1, P, V1>(a.g[1], a.Wp[1], y, x0, gk);
    }
  }
  const double total = block_sum<BLOCK>(local, smem);
  if (threadIdx.x == 0) a.partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// any number of components, any factor: one counts pixel per thread, run-time loops over the block
__global__ __launch_bounds__(BLOCK) void poisson_mixed_generic_kernel(PoissonMixedArgs a) {
  __shared__ double smem[BLOCK / 64];
  const int y = blockIdx.y;
  const int x = blockIdx.x * BLOCK + threadIdx.x;
  double local = 0.0;
  if (x < a.Wd) {
    const size_t off = (size_t)y * a.Wd + x;
    float pooled[JD_MAX_COMPONENTS];
    float n = 0.f;
#pragma unroll
    for (int k = 0; k < JD_MAX_COMPONENTS; ++k) {
      if (k >= a.n_comp) break;
      const int u = a.up[k];
      float acc = 0.f;
      for (int dy = 0; dy < u; ++dy) {
        const float* row = a.conv[k] + (size_t)(y * u + dy + a.oy[k]) * a.Wp[k] + ((size_t)x * u + a.ox[k]);
        for (int dx = 0; dx < u; ++dx) acc += row[dx];
      }
      pooled[k] = acc;
      n += fmaxf(acc, 0.f);
    }
    n += a.background[off];
    float term, g;
    poisson_point(n, a.counts[off], a.eps, a.inv_n, term, g);
    local = (double)term;
    if (a.npred_out) a.npred_out[off] = n;
    if (a.write_grad) {
#pragma unroll
      for (int k = 0; k < JD_MAX_COMPONENTS; ++k) {
        if (k >= a.n_comp) break;
        const int u = a.up[k];
        const float gk = pooled[k] >= 0.f ? g : 0.f;
        for (int dy = 0; dy < u; ++dy) {
          float* row = a.g[k] + (size_t)(y * u + dy) * a.Wp[k] + (size_t)x * u;
          for (int dx = 0; dx < u; ++dx) row[dx] = gk;
        }
      }
    }
  }
  const double total = block_sum<BLOCK>(local, smem);
  if (threadIdx.x == 0) a.partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

template <int U0, bool VEC>
static void launch_poisson_mixed_u1(const PoissonMixedArgs& a, dim3 grid, hipStream_t stream) {
  switch (a.up[1]) {
    case 1: poisson_mixed_kernel<U0, 1, VEC><<<grid, BLOCK, 0, stream>>>(a); break;
    case 2: poisson_mixed_kernel<U0, 2, VEC><<<grid, BLOCK, 0, stream>>>(a); break;
    case 3: poisson_mixed_kernel<U0, 3, VEC><<<grid, BLOCK, 0, stream>>>(a); break;
    default: poisson_mixed_kernel<U0, 4, VEC><<<grid, BLOCK, 0, stream>>>(a); break;
  }
}

template <bool VEC>
static void launch_poisson_mixed_u0(const PoissonMixedArgs& a, dim3 grid, hipStream_t stream) {
  switch (a.up[0]) {
    case 1: launch_poisson_mixed_u1<1, VEC>(a, grid, stream); break;
    case 2: launch_poisson_mixed_u1<2, VEC>(a, grid, stream); break;
    case 3: launch_poisson_mixed_u1<3, VEC>(a, grid, stream); break;
    default: launch_poisson_mixed_u1<4, VEC>(a, grid, stream); break;
  }
}

int poisson_mixed_max_partials(int Hd, int Wd) { return ((Wd + BLOCK - 1) / BLOCK) * Hd; }

int launch_poisson_mixed(const PoissonMixedArgs& a, int* n_partials, hipStream_t stream) {
  const bool two = a.n_comp == 2 && a.up[0] >= 1 && a.up[0] <= 4 && a.up[1] >= 1 && a.up[1] <= 4;
  auto aligned = [](const void* p, uintptr_t bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1)) == 0; };
  // two counts pixels per thread: every row piece then starts at a multiple of its vector width
  bool vec = two && a.Wd % 2 == 0 && aligned(a.background, 8) && aligned(a.counts, 8) && aligned(a.npred_out, 8);
  for (int c = 0; vec && c < 2; ++c) {
    const int v = a.up[c] % 2 == 0 ? 4 : 2;
    vec = a.Wp[c] % v == 0 && a.ox[c] % v == 0 && aligned(a.conv[c], 4 * v) && (!a.write_grad || aligned(a.g[c], 4 * v));
  }
  const int per_block = BLOCK * (vec ? 2 : 1);
  dim3 grid((a.Wd + per_block - 1) / per_block, a.Hd);
  *n_partials = grid.x * grid.y;
  ProfScope prof(JD_KERNEL_POISSON_MIXED, stream);
  if (!two)
    poisson_mixed_generic_kernel<<<grid, BLOCK, 0, stream>>>(a);
  else if (vec)
    launch_poisson_mixed_u0<true>(a, grid, stream);
  else
    launch_poisson_mixed_u0<false>(a, grid, stream);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

// ------------------------------------------------------------------------------------------
// K5: adjoint epilogue. grad[p][q] (+)= coef * scale[p][q] * corr[(p-oy) mod Hp][(q-ox) mod Wp]
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void adjoint_epilogue_kernel(const float* __restrict__ corr,
                                                                const float* __restrict__ scale,
                                                                float* __restrict__ grad, int H, int W,
                                                                int Hp, int Wp, int oy, int ox,
                                                                float coef, int accumulate) {
  const int p = blockIdx.y;
  const int q = blockIdx.x * BLOCK + threadIdx.x;
  if (q >= W) return;
  int sy = p - oy;
  if (sy < 0) sy += Hp;
  int sx = q - ox;
  if (sx < 0) sx += Wp;
  const size_t off = (size_t)p * W + q;
  float v = corr[(size_t)sy * Wp + sx] * coef;
  if (scale) v *= scale[off];
  if (accumulate) v += grad[off];
  grad[off] = v;
}

int launch_adjoint_epilogue(const float* corr, const float* scale, float* grad, int H, int W, int Hp,
                            int Wp, int oy, int ox, float coef, int accumulate, hipStream_t stream) {
  dim3 grid((W + BLOCK - 1) / BLOCK, H);
  ProfScope prof(JD_KERNEL_ADJOINT_EPILOGUE, stream);
  adjoint_epilogue_kernel<<<grid, BLOCK, 0, stream>>>(corr, scale, grad, H, W, Hp, Wp, oy, ox, coef,
                                                      accumulate);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

// crop: out[y][x] = padded[y+oy][x+ox]
__global__ __launch_bounds__(BLOCK) void crop_kernel(const float* __restrict__ padded,
                                                    float* __restrict__ out, int H, int W, int Wp, int oy,
                                                    int ox) {
  const int y = blockIdx.y;
  const int x = blockIdx.x * BLOCK + threadIdx.x;
  if (x >= W) return;
  out[(size_t)y * W + x] = padded[(size_t)(y + oy) * Wp + (x + ox)];
}

int launch_crop(const float* padded, float* out, int H, int W, int Wp, int oy, int ox, hipStream_t stream) {
  dim3 grid((W + BLOCK - 1) / BLOCK, H);
  crop_kernel<<<grid, BLOCK, 0, stream>>>(padded, out, H, W, Wp, oy, ox);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

// ------------------------------------------------------------------------------------------
// stand-alone Poisson NLL on a flat npred (autograd.Function seam of loss.py:35-37)
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void poisson_nll_kernel(const float* __restrict__ npred,
                                                           const float* __restrict__ counts, size_t n,
                                                           float eps, float inv_n,
                                                           float* __restrict__ grad,
                                                           double* __restrict__ partials) {
  __shared__ double smem[BLOCK / 64];
  double local = 0.0;
  const size_t stride = (size_t)gridDim.x * BLOCK;
  for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
    const float v = npred[i], c = counts[i];
    float term, g;
    poisson_point(v, c, eps, inv_n, term, g);
    local += (double)term;
    if (grad) grad[i] = g;
  }
  const double total = block_sum<BLOCK>(local, smem);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

__global__ __launch_bounds__(BLOCK) void flux_from_theta_kernel(const float* __restrict__ theta,
                                                               const float* __restrict__ mask,
                                                               float* __restrict__ flux, size_t n, int linear) {
  const size_t stride = (size_t)gridDim.x * BLOCK;
  for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
    float f = linear ? theta[i] : expf(theta[i]);
    if (mask) f *= mask[i];
    flux[i] = f;
  }
}

// ------------------------------------------------------------------------------------------
// element-wise priors
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void elementwise_prior_kernel(int kind, const float* __restrict__ flux,
                                                                 size_t n, float alpha, float beta,
                                                                 float coef, float* __restrict__ grad,
                                                                 double* __restrict__ partials) {
  __shared__ double smem[BLOCK / 64];
  double local = 0.0;
  const size_t stride = (size_t)gridDim.x * BLOCK;
  for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
    const float f = flux[i];
    float value, dv;
    if (kind == 1) {  // inverse gamma: -beta/f + (-alpha-1)*log f      (priors/core.py:223-224)
      value = -beta / f + (-alpha - 1.f) * logf(f);
      dv = beta / (f * f) + (-alpha - 1.f) / f;
    } else {  // exponential: -alpha * f                                (priors/core.py:324)
      value = -alpha * f;
      dv = -alpha;
    }
    local += (double)value;
    if (grad) grad[i] += coef * dv;
  }
  const double total = block_sum<BLOCK>(local, smem);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// ------------------------------------------------------------------------------------------
// element-wise priors with sub-pixel cycle spin (priors/core.py:220-226,321-326; utils/torch.py:31-38,122-143): the
// prior is evaluated on s = K (*) f, the 3 x 3 cross-correlation of the flux with the bilinear weights of a shift
// (x0, y0) in [-0.5, 0.5]^2, zero outside the image; the gradient is the adjoint stencil of g = v'(s).  One launch over
// 2-D tiles of SP_TY x SP_TX pixels: a block stages its flux tile with a 2-pixel halo in LDS, forms s and g on the tile
// plus a 1-pixel halo (g = 0 outside the image; the halo is computed again by the neighbouring block, so no block reads
// another's results), applies the adjoint stencil from LDS and does ONE read-modify-write of grad per pixel it owns.
// v(s) is summed over the owned pixels only, into one double per block.  HBM traffic: 12 B/pixel (the halo re-reads
// come from L2), like elementwise_prior_kernel.
// ------------------------------------------------------------------------------------------
// tile height, measured on MI355X (inverse-gamma, us per launch): 2048^2 32 rows 22.6, 16 rows 24.4, 8 rows 23.8;
// 8192^2 203 / 220 / 282 (profiles/priors/README.md)
constexpr int SP_TX = 64, SP_TY = 32;
constexpr int SP_FW = SP_TX + 4, SP_FH = SP_TY + 4;  // flux window: tile + 2-pixel halo
constexpr int SP_GW = SP_TX + 2, SP_GH = SP_TY + 2;  // s / g window: tile + 1-pixel halo

struct SubpixArgs {
  const float* flux;
  float* grad;  // nullable: value only
  double* partials;
  const float* offset_dev;  // nullable, device [2] = {x0, y0}: read instead of the two members below
  float x0, y0;
  float alpha, beta, coef;
  int kind, H, W;
};

// (the nine weights k[i][j] = wx(j - 1) * wy(i - 1): `subpix_weights` of jd_subpix.h, shared with the GMM patch prior)

// VEC: W % 4 == 0 and 16-byte aligned images -- the 64 columns of the tile go in 16-byte loads, the read-modify-write of
// grad in 16-byte loads and stores (a group of 4 columns is then inside the image or outside as a whole)
template <bool VEC>
__global__ __launch_bounds__(BLOCK) void elementwise_prior_subpix_kernel(SubpixArgs a) {
  __shared__ float F[SP_FH][SP_FW];
  __shared__ float G[SP_GH][SP_GW];
  __shared__ double smem[BLOCK / 64];
  const int H = a.H, W = a.W;
  const int tx0 = blockIdx.x * SP_TX, ty0 = blockIdx.y * SP_TY;  // first owned pixel
  const float x0 = a.offset_dev ? a.offset_dev[0] : a.x0, y0 = a.offset_dev ? a.offset_dev[1] : a.y0;
  float k[3][3];
  subpix_weights(x0, y0, k);

  // ---- flux window -> LDS (zero outside the image) ----
  const int c4 = threadIdx.x & 15, r0 = threadIdx.x >> 4;  // column group of 4, row 0..15
  for (int r = r0; r < SP_FH; r += 16) {
    const int y = ty0 - 2 + r, x = tx0 + 4 * c4;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    if (y >= 0 && y < H) {
      const float* row = a.flux + (size_t)y * W;
      if (VEC) {
        if (x < W) {
          const float4 q = *reinterpret_cast<const float4*>(row + x);
          v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
        }
      } else {
#pragma unroll
        for (int i = 0; i < 4; ++i)
          if (x + i < W) v[i] = row[x + i];
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) F[r][2 + 4 * c4 + i] = v[i];
  }
  if (threadIdx.x < 4 * SP_FH) {  // the two halo columns either side
    const int r = threadIdx.x >> 2, c = threadIdx.x & 3;
    const int col = c < 2 ? c : SP_TX + c;  // 0, 1, TX + 2, TX + 3
    const int y = ty0 - 2 + r, x = tx0 - 2 + col;
    F[r][col] = (y >= 0 && y < H && x >= 0 && x < W) ? a.flux[(size_t)y * W + x] : 0.f;
  }
  __syncthreads();

  // ---- s = K (*) f and g = v'(s) on the tile + 1-pixel halo; v(s) summed over the owned pixels ----
  double local = 0.0;
  const float am1 = -a.alpha - 1.f;
  for (int idx = threadIdx.x; idx < SP_GH * SP_GW; idx += BLOCK) {
    const int ry = idx / SP_GW, rx = idx - ry * SP_GW;
    const int y = ty0 - 1 + ry, x = tx0 - 1 + rx;
    float g = 0.f;
    if (y >= 0 && y < H && x >= 0 && x < W) {
      float s = 0.f;
#pragma unroll
      for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) s = fmaf(k[i][j], F[ry + i][rx + j], s);
      float value;
      if (a.kind == 1) {  // inverse gamma: the expressions of elementwise_prior_kernel
        value = -a.beta / s + am1 * logf(s);
        g = a.beta / (s * s) + am1 / s;
      } else {
        value = -a.alpha * s;
        g = -a.alpha;
      }
      if (ry >= 1 && ry <= SP_TY && rx >= 1 && rx <= SP_TX) local += (double)value;
    }
    G[ry][rx] = g;
  }
  __syncthreads();

  // ---- adjoint stencil: df[p][q] = sum_ij k[i][j] g[p - i + 1][q - j + 1]; grad += coef * df ----
  if (a.grad) {
    for (int r = r0; r < SP_TY; r += 16) {
      const int y = ty0 + r, x = tx0 + 4 * c4;
      if (y >= H || x >= W) continue;
      float df[4] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        float gr[6];  // g[y - i + 1][x - 1 .. x + 4]: window row (r + 1) - i + 1, columns 4 c4 .. 4 c4 + 5
#pragma unroll
        for (int c = 0; c < 6; ++c) gr[c] = G[r + 2 - i][4 * c4 + c];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int j = 0; j < 3; ++j) df[e] = fmaf(k[i][j], gr[e + 2 - j], df[e]);
      }
      float* dst = a.grad + (size_t)y * W + x;
      if (VEC) {
        float4 q = *reinterpret_cast<float4*>(dst);
        q.x += a.coef * df[0], q.y += a.coef * df[1], q.z += a.coef * df[2], q.w += a.coef * df[3];
        *reinterpret_cast<float4*>(dst) = q;
      } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (x + e < W) dst[e] += a.coef * df[e];
      }
    }
  }
  const double total = block_sum<BLOCK>(local, smem);
  if (threadIdx.x == 0) a.partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] = total;
}

// ------------------------------------------------------------------------------------------
// smoothness prior epilogue (priors/core.py:373-384): with s = K (*) f already in `smooth`, the partial sums of f * s
// (value = -sum f s) and grad += coef * s, coef = grad_coef * (-2) (K symmetric: the operator is self-adjoint).  A
// streaming pass, 16 B/pixel with the gradient: the first 4 n4 pixels in 16-byte accesses (n4 = n / 4 where all images are
// 16-byte aligned, else 0), the tail pixel by pixel.
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(BLOCK) void smoothness_prior_kernel(const float* __restrict__ flux,
                                                                const float* __restrict__ smooth, size_t n, size_t n4,
                                                                float coef, float* __restrict__ grad,
                                                                double* __restrict__ partials) {
  __shared__ double smem[BLOCK / 64];
  const size_t tid = (size_t)blockIdx.x * BLOCK + threadIdx.x, nthreads = (size_t)gridDim.x * BLOCK;
  double local = 0.0;
  for (size_t i = tid; i < n4; i += nthreads) {
    const float4 f = reinterpret_cast<const float4*>(flux)[i];
    const float4 s = reinterpret_cast<const float4*>(smooth)[i];
    local += (double)(f.x * s.x) + (double)(f.y * s.y) + (double)(f.z * s.z) + (double)(f.w * s.w);
    if (grad) {
      float4 g = reinterpret_cast<float4*>(grad)[i];
      g.x += coef * s.x, g.y += coef * s.y, g.z += coef * s.z, g.w += coef * s.w;
      reinterpret_cast<float4*>(grad)[i] = g;
    }
  }
  for (size_t i = 4 * n4 + tid; i < n; i += nthreads) {
    const float s = smooth[i];
    local += (double)(flux[i] * s);
    if (grad) grad[i] += coef * s;
  }
  const double total = block_sum<BLOCK>(local, smem);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
}

// small per-process scratch for the stand-alone reductions (grown on demand, never freed while
// the library is loaded; one per device would be needed for multi-device processes -- the
// framework runs one process per GPU)
static double* g_partials = nullptr;
static size_t g_partials_cap = 0;
static int ensure_partials(size_t n) {
  if (n <= g_partials_cap) return JD_OK;
  if (g_partials) (void)hipFree(g_partials);
  g_partials = nullptr;
  g_partials_cap = 0;
  JD_HIP(hipMalloc(&g_partials, n * sizeof(double)));
  g_partials_cap = n;
  return JD_OK;
}

}  // namespace jd

// ==========================================================================================
// C ABI
// ==========================================================================================
using namespace jd;

extern "C" int jd_poisson_nll(const float* npred, const float* counts, size_t n, float stirling_mean,
                              float eps, float* loss_out, float* grad_npred, void* stream) {
  JD_REQUIRE(npred && counts && loss_out && n > 0, "jd_poisson_nll: null argument or n == 0");
  size_t blocks = (n + BLOCK - 1) / BLOCK;
  if (blocks > 2048) blocks = 2048;
  int rc = ensure_partials(8192);
  if (rc) return rc;
  hipStream_t s = as_stream(stream);
  poisson_nll_kernel<<<(unsigned)blocks, BLOCK, 0, s>>>(npred, counts, n, eps, 1.f / (float)n, grad_npred,
                                                       g_partials);
  JD_LAUNCH_CHECK();
  return launch_finalize_sum(g_partials, (int)blocks, 1.0 / (double)n, (double)stirling_mean, loss_out, 0, s);
}

extern "C" int jd_elementwise_prior_fwd_bwd(int kind, const float* flux, size_t n, float alpha, float beta,
                                            float log_const, float* value_out, float grad_coef,
                                            float* grad_flux_accum, void* stream) {
  JD_REQUIRE(kind == 1 || kind == 2, "jd_elementwise_prior_fwd_bwd: kind must be 1 (inverse-gamma) or 2 (exponential)");
  JD_REQUIRE(flux && value_out && n > 0, "jd_elementwise_prior_fwd_bwd: null argument or n == 0");
  size_t blocks = (n + BLOCK - 1) / BLOCK;
  if (blocks > 2048) blocks = 2048;
  int rc = ensure_partials(8192);
  if (rc) return rc;
  hipStream_t s = as_stream(stream);
  {
    ProfScope prof(JD_KERNEL_ELEMENTWISE_PRIOR, s);
    elementwise_prior_kernel<<<(unsigned)blocks, BLOCK, 0, s>>>(kind, flux, n, alpha, beta, grad_coef,
                                                               grad_flux_accum, g_partials);
  }
  JD_LAUNCH_CHECK();
  return launch_finalize_sum(g_partials, (int)blocks, 1.0 / (double)n, (double)log_const, value_out, 0, s);
}

extern "C" int jd_elementwise_prior_subpix_fwd_bwd(int kind, const float* flux, int H, int W, float alpha, float beta,
                                                   float log_const, float x0, float y0, const float* offset_dev,
                                                   float* value_out, float grad_coef, float* grad_flux_accum,
                                                   void* stream) {
  JD_REQUIRE(kind == 1 || kind == 2,
             "jd_elementwise_prior_subpix_fwd_bwd: kind must be 1 (inverse-gamma) or 2 (exponential)");
  JD_REQUIRE(flux && value_out && H > 0 && W > 0, "jd_elementwise_prior_subpix_fwd_bwd: null argument or non-positive shape");
  // (the negated form refuses NaN too)
  JD_REQUIRE(offset_dev || (x0 >= -0.5f && x0 <= 0.5f && y0 >= -0.5f && y0 <= 0.5f),
             "jd_elementwise_prior_subpix_fwd_bwd: offsets (%g, %g) not in [-0.5, 0.5]", (double)x0, (double)y0);
  const dim3 grid((W + SP_TX - 1) / SP_TX, (H + SP_TY - 1) / SP_TY);
  const size_t blocks = (size_t)grid.x * grid.y;
  JD_REQUIRE(blocks <= (size_t)1 << 24 && grid.y <= 65535, "jd_elementwise_prior_subpix_fwd_bwd: image %d x %d too large", H, W);
  int rc = ensure_partials(blocks > 8192 ? blocks : 8192);
  if (rc) return rc;
  hipStream_t s = as_stream(stream);
  SubpixArgs a{flux, grad_flux_accum, g_partials, offset_dev, x0, y0, alpha, beta, grad_coef, kind, H, W};
  const bool vec = W % 4 == 0 && (reinterpret_cast<uintptr_t>(flux) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(grad_flux_accum) & 15) == 0;
  {
    ProfScope prof(JD_KERNEL_ELEMENTWISE_SUBPIX, s);
    if (vec)
      elementwise_prior_subpix_kernel<true><<<grid, BLOCK, 0, s>>>(a);
    else
      elementwise_prior_subpix_kernel<false><<<grid, BLOCK, 0, s>>>(a);
  }
  JD_LAUNCH_CHECK();
  return launch_finalize_sum(g_partials, (int)blocks, 1.0 / ((double)H * (double)W), (double)log_const, value_out, 0, s);
}

// scratch image of the smoothness prior (K (*) f), grown on demand like g_partials
static float* g_smooth = nullptr;
static size_t g_smooth_cap = 0;

extern "C" int jd_smoothness_prior_fwd_bwd(jd_conv_plan* plan, const float* khat, const float* flux, float* value_out,
                                           float grad_coef, float* grad_flux_accum, void* stream) {
  JD_REQUIRE(plan && khat && flux && value_out, "jd_smoothness_prior_fwd_bwd: null argument");
  int shape[6];
  int rc = jd_conv_plan_shape(plan, shape);
  if (rc) return rc;
  const size_t n = (size_t)shape[0] * (size_t)shape[1];
  if (n > g_smooth_cap) {
    if (g_smooth) (void)hipFree(g_smooth);
    g_smooth = nullptr, g_smooth_cap = 0;
    JD_HIP(hipMalloc(&g_smooth, n * sizeof(float)));
    g_smooth_cap = n;
  }
  if ((rc = ensure_partials(8192))) return rc;
  if ((rc = jd_conv_same(plan, flux, nullptr, khat, g_smooth, stream))) return rc;
  const bool aligned = ((reinterpret_cast<uintptr_t>(flux) | reinterpret_cast<uintptr_t>(grad_flux_accum)) & 15) == 0;
  const size_t n4 = aligned ? n / 4 : 0;
  size_t blocks = (n4 + (n - 4 * n4) + BLOCK - 1) / BLOCK;
  if (blocks > 2048) blocks = 2048;
  if (blocks < 1) blocks = 1;
  hipStream_t s = as_stream(stream);
  {
    ProfScope prof(JD_KERNEL_SMOOTHNESS, s);
    smoothness_prior_kernel<<<(unsigned)blocks, BLOCK, 0, s>>>(flux, g_smooth, n, n4, -2.f * grad_coef, grad_flux_accum,
                                                              g_partials);
  }
  JD_LAUNCH_CHECK();
  return launch_finalize_sum(g_partials, (int)blocks, -1.0, 0.0, value_out, 0, s);
}

extern "C" int jd_flux_from_theta(const float* theta, const float* mask, float* flux, size_t n, int use_log_flux,
                                  void* stream) {
  JD_REQUIRE(theta && flux && n > 0, "jd_flux_from_theta: null argument or n == 0");
  size_t blocks = (n + BLOCK - 1) / BLOCK;
  if (blocks > 8192) blocks = 8192;
  flux_from_theta_kernel<<<(unsigned)blocks, BLOCK, 0, as_stream(stream)>>>(theta, mask, flux, n, use_log_flux ? 0 : 1);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

// Components that share one forward operator (models/npred.py:279-295 builds every component's model of a dataset from
// the SAME exposure and, unless `psf` is a dict, the same PSF): npred = sum_c clip(PSF * (flux_c E), 0) = PSF * ((sum_c
// flux_c) E) wherever no term is negative, and d loss / d flux_c is ONE image for all c.  The two helpers either side of
// the single-component launches (jolideco_amd/loss.py): the sum of the component fluxes, left to right, and the copy of
// the gradient image into the other components' gradient images.  16-byte accesses where n and the pointers allow.
struct ImagePtrs {
  const float* src[4];
  float* dst[4];
  int n_src, n_dst;
};

template <bool VEC>
__global__ __launch_bounds__(BLOCK) void sum_images_kernel(ImagePtrs p, size_t n) {
  const size_t stride = (size_t)gridDim.x * BLOCK;
  if (VEC) {
    const size_t n4 = n / 4;
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n4; i += stride) {
      float4 v = reinterpret_cast<const float4*>(p.src[0])[i];
      for (int c = 1; c < p.n_src; ++c) {
        const float4 w = reinterpret_cast<const float4*>(p.src[c])[i];
        v.x += w.x, v.y += w.y, v.z += w.z, v.w += w.w;
      }
      for (int d = 0; d < p.n_dst; ++d) reinterpret_cast<float4*>(p.dst[d])[i] = v;
    }
  } else {
    for (size_t i = (size_t)blockIdx.x * BLOCK + threadIdx.x; i < n; i += stride) {
      float v = p.src[0][i];
      for (int c = 1; c < p.n_src; ++c) v += p.src[c][i];
      for (int d = 0; d < p.n_dst; ++d) p.dst[d][i] = v;
    }
  }
}

static int launch_sum_images(const ImagePtrs& p, size_t n, void* stream) {
  bool vec = n % 4 == 0;
  for (int c = 0; c < p.n_src; ++c) vec = vec && (reinterpret_cast<uintptr_t>(p.src[c]) & 15) == 0;
  for (int d = 0; d < p.n_dst; ++d) vec = vec && (reinterpret_cast<uintptr_t>(p.dst[d]) & 15) == 0;
  size_t blocks = ((vec ? n / 4 : n) + BLOCK - 1) / BLOCK;
  if (blocks > 8192) blocks = 8192;
  if (vec)
    sum_images_kernel<true><<<(unsigned)blocks, BLOCK, 0, as_stream(stream)>>>(p, n);
  else
    sum_images_kernel<false><<<(unsigned)blocks, BLOCK, 0, as_stream(stream)>>>(p, n);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

extern "C" int jd_sum_images(float* out, const float* const* srcs, int n_srcs, size_t n, void* stream) {
  JD_REQUIRE(out && srcs && n > 0, "jd_sum_images: null argument or n == 0");
  JD_REQUIRE(n_srcs >= 1 && n_srcs <= 4, "jd_sum_images: %d source images (1 to 4)", n_srcs);
  ImagePtrs p{};
  for (int c = 0; c < n_srcs; ++c) {
    JD_REQUIRE(srcs[c], "jd_sum_images: source %d is null", c);
    p.src[c] = srcs[c];
  }
  p.n_src = n_srcs, p.dst[0] = out, p.n_dst = 1;
  return launch_sum_images(p, n, stream);
}

extern "C" int jd_copy_image_to(const float* src, float* const* dsts, int n_dsts, size_t n, void* stream) {
  JD_REQUIRE(src && dsts && n > 0, "jd_copy_image_to: null argument or n == 0");
  JD_REQUIRE(n_dsts >= 1 && n_dsts <= 4, "jd_copy_image_to: %d destination images (1 to 4)", n_dsts);
  ImagePtrs p{};
  p.src[0] = src, p.n_src = 1;
  for (int d = 0; d < n_dsts; ++d) {
    JD_REQUIRE(dsts[d] && dsts[d] != src, "jd_copy_image_to: destination %d is null or the source", d);
    p.dst[d] = dsts[d];
  }
  p.n_dst = n_dsts;
  return launch_sum_images(p, n, stream);
}

// The step scalars of an epoch from a pinned host row (device-accessible: zero-copy reads over the host link) into their
// device buffer: one small block instead of a hipMemcpyAsync, whose copy engine hand-over costs a stream 6-8 us between two
// epochs (tools/gpu/small_fits.py).
__global__ __launch_bounds__(256) void fetch_scalars_kernel(const int* __restrict__ src, int* __restrict__ dst, int n) {
  for (int i = threadIdx.x; i < n; i += 256) dst[i] = src[i];
}

extern "C" int jd_step_scalars_fetch(const int32_t* host_row, int32_t* dst, int n, void* stream) {
  JD_REQUIRE(host_row && dst && n > 0 && n <= (1 << 20), "jd_step_scalars_fetch: null argument or bad n");
  fetch_scalars_kernel<<<1, 256, 0, as_stream(stream)>>>(host_row, dst, n);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

extern "C" int jd_version(void) { return 100; }
extern "C" const char* jd_last_error(void) { return jd::error_buffer(); }
extern "C" const char* jd_target_arch(void) { return "gfx950"; }
