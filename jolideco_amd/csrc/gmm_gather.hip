// The image-wide passes of the 8x8 GMM patch prior: the image norm in front of phase 1, the overlap-add gather of the
// per-patch gradient rows (+ the fused optimizer step), and the sums over the rolled bands of a sharded prior.
// Overlap-add gather: every pixel of the rolled frame sums the contributions of the patches that
// cover it in a fixed order (no float atomics), un-rolls and accumulates into grad.
#include "gmm_internal.h"

namespace jd {

// ---- image norm of the prior (jolideco/utils/norms.py:225-426; jd_image_norm of the header) ------------------------
// n(f) is written once per pass into an image of the handle (gmm_image_norm_kernel: everything in phase 1 reads it in
// place of the flux); n'(f) is evaluated by the gather from the pixel's RAW flux (chain rule of the overlap-add).

// out[i] = n(in[i]), i < n: a streaming pass (4 bytes read + 4 written per pixel), grid-stride; instantiated per kind (no
// branch in the pixel loop).  The first 4 n4 pixels go in 16-byte loads and stores (n4 = n / 4 where both images are
// 16-byte aligned, else 0), the rest -- the up to 3 pixels of the tail, or everything -- pixel by pixel.
template <int KIND>
__global__ __launch_bounds__(256) void gmm_image_norm_kernel(const float* __restrict__ in, float* __restrict__ out, size_t n,
                                                             ImageNormArgs nm, size_t n4) {
  const size_t tid = (size_t)blockIdx.x * 256 + threadIdx.x, nthreads = (size_t)gridDim.x * 256;
  for (size_t i = tid; i < n4; i += nthreads) {
    const float4 v = reinterpret_cast<const float4*>(in)[i];
    reinterpret_cast<float4*>(out)[i] = make_float4(image_norm_value<KIND>(v.x, nm), image_norm_value<KIND>(v.y, nm),
                                                    image_norm_value<KIND>(v.z, nm), image_norm_value<KIND>(v.w, nm));
  }
  for (size_t i = 4 * n4 + tid; i < n; i += nthreads) out[i] = image_norm_value<KIND>(in[i], nm);
}

int launch_image_norm(const float* in, float* out, size_t n, const ImageNormArgs& nm, int n_cu, hipStream_t s) {
  const size_t n4 = aligned16(in) && aligned16(out) ? n / 4 : 0;
  const size_t items = n4 + (n - 4 * n4);
  size_t blocks = (items + 255) / 256;
  const size_t cap = (size_t)n_cu * 8;
  if (blocks > cap) blocks = cap;
  if (blocks < 1) blocks = 1;
  const unsigned gb = (unsigned)blocks;
  bool launched = false;  // (the identity has no kernel here: the callers read the flux itself)
  dispatch_norm_kind(nm.kind, [&](auto kind) {
    if constexpr (decltype(kind)::value != NORM_IDENTITY) {
      gmm_image_norm_kernel<decltype(kind)::value><<<gb, 256, 0, s>>>(in, out, n, nm, n4);
      launched = true;
    }
  });
  JD_REQUIRE(launched, "image norm kind %d has no kernel", nm.kind);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

template <bool NORM>
__global__ __launch_bounds__(256) void gmm_gather_kernel(GmmGatherArgs a) {
#pragma clang fp contract(off)
  use_device_shift(a);
  const int Y = a.y_begin + blockIdx.y;
  const int X = blockIdx.x * 256 + threadIdx.x;
  if (X >= a.W || Y >= a.y_end) return;
  // patch rows py with py*stride <= Y <= py*stride + 7
  int py_hi = Y / a.stride;
  int py_lo = (Y - (P - 1) + a.stride - 1) / a.stride;
  if (Y - (P - 1) < 0) py_lo = 0;
  if (py_lo < a.row_begin) py_lo = a.row_begin;
  if (py_hi > a.row_end - 1) py_hi = a.row_end - 1;
  int px_hi = X / a.stride;
  int px_lo = (X - (P - 1) + a.stride - 1) / a.stride;
  if (X - (P - 1) < 0) px_lo = 0;
  if (px_hi > a.nPx - 1) px_hi = a.nPx - 1;
  const bool slots = a.winner && *a.flag != a.gen;
  float sum = 0.f;
  bool any = false;
  for (int py = py_lo; py <= py_hi; ++py) {
    const int r = Y - py * a.stride;
    for (int px = px_lo; px <= px_hi; ++px) {
      const int cc = X - px * a.stride;
      if (slots) {
        const int slot = a.winner[(size_t)py * a.nPx + px];
        if (slot >= 0) sum += a.grec[(size_t)slot * D + r * P + cc];
      } else {
        const size_t n = (size_t)(py - a.row_begin) * a.nPx + px;
        sum += a.gpatch[n * D + r * P + cc];
      }
      any = true;
    }
  }
  if (NORM) {  // the same three forms with the chain rule of the image norm
    const int yy = wrap(Y - a.shift_y, a.H), xx = wrap(X - a.shift_x, a.W);
    const size_t idx = (size_t)yy * a.W + xx;
    const bool live = any && sum != 0.f;
    const float term = live ? gather_normed_term(a, sum, a.raw_flux[idx]) : 0.f;
    if (a.band) a.band[(size_t)(Y - a.y_begin) * a.W + X] = term;
    else if (live) a.grad[idx] += term;
    return;
  }
  if (a.band) {
    a.band[(size_t)(Y - a.y_begin) * a.W + X] = any ? a.coef * sum : 0.f;
    return;
  }
  if (!any) return;
  const int yy = wrap(Y - a.shift_y, a.H), xx = wrap(X - a.shift_x, a.W);
  a.grad[(size_t)yy * a.W + xx] += a.coef * sum;
}

// The same overlap-add, one 32 x 32 pixel tile of the rolled frame per block (stride >= 4: at most 10 x 10 patches touch a
// tile): the gradient rows of those patches are fetched ONCE, as whole 256-byte rows, into LDS and every pixel sums its
// contributions from there in the order of gmm_gather_kernel (patch rows ascending, then patch columns: the same bits).
// Every gather kernel adds the ROUNDED product coef * sum (`fp contract(off)`: no fused multiply-add -- hipcc's __fmul_rn
// is a plain product that the compiler contracts all the same): the band
// form stores that product and jd_add_rolled_bands adds it later, so a sharded step -- with one rank: RCCL's identity
// collectives -- gives the bits of the un-sharded one (tests/test_gpu_distributed.py).
// The per-pixel kernel reads 4 bytes from each of up to four different rows per thread -- 4x the memory instructions,
// none of them a full line; at 4096^2, where the rows no longer sit in the Infinity Cache, it took 5x the 2048^2 time.
// patches per tile and dimension: the tile's first row is a multiple of 32 above y_begin = row_begin * stride, so for
// stride 4 (and 8) it is aligned with the patch grid: 9 rows of patches (4); strides 5, 6, 7 have at most
// floor(38 / s) + 1 = 8, 7, 6.  Columns: the tile's first column is shift_x (mod 4), not aligned with the grid: 10.
constexpr int GATHER_T = 32, GATHER_MAX_P = 9, GATHER_MAX_PX = GATHER_MAX_P + 1;

// NA: addend images of the fused step (jd_adam.h: step.addend[0 .. NA) are set), added to the gradient it reads before the
// prior's term -- streams of the step like the others, loaded with them
template <bool NORM, int NA>
__global__ __launch_bounds__(256) void gmm_gather_tile_kernel(GmmGatherArgs a) {
#pragma clang fp contract(off)
  use_device_shift(a);
  use_device_bias(a.step);
  __shared__ __attribute__((aligned(16))) float rows[GATHER_MAX_P * GATHER_MAX_PX][D];
  const int tid = threadIdx.x;
  const int xoff = a.vec ? ((a.shift_x % 4) + 4) & 3 : 0;
  const int X0 = (int)blockIdx.x * GATHER_T - ((4 - xoff) & 3), Y0 = a.y_begin + blockIdx.y * GATHER_T;
  auto ceil_div_pos = [](int v, int s) { return v <= 0 ? 0 : (v + s - 1) / s; };
  int py0 = ceil_div_pos(Y0 - (P - 1), a.stride), py1 = (Y0 + GATHER_T - 1) / a.stride;
  int px0 = ceil_div_pos(X0 - (P - 1), a.stride), px1 = (X0 + GATHER_T - 1) / a.stride;
  if (py0 < a.row_begin) py0 = a.row_begin;
  if (py1 > a.row_end - 1) py1 = a.row_end - 1;
  if (px1 > a.nPx - 1) px1 = a.nPx - 1;
  int npx = px1 - px0 + 1, npy = py1 - py0 + 1;
  if (npx > GATHER_MAX_PX) npx = GATHER_MAX_PX, px1 = px0 + npx - 1;  // (cannot happen, see above: keeps LDS in bounds)
  if (npy > GATHER_MAX_P) npy = GATHER_MAX_P, py1 = py0 + npy - 1;
  const bool touched = npx > 0 && npy > 0;  // (block-uniform) some patch of the shard touches this tile
  if (!touched && !a.do_step) {
    if (a.band) {
      const int Y = Y0 + (tid >> 3);
      for (int i = 0; i < 4; ++i) {
        const int X = X0 + (tid & 7) * 4 + i;
        if (Y < a.y_end && X >= 0 && X < a.W) a.band[(size_t)(Y - a.y_begin) * a.W + X] = 0.f;
      }
    }
    return;
  }
  // the optimizer step's own streams (gradient, parameter, flux, moments, mask of the thread's four pixels) do not depend
  // on the patch rows: their loads are issued FIRST, so that they are in flight beside the winner -> row chain below
  // instead of behind the block barrier (three dependent round trips per block become two)
  const int Yt = Y0 + (tid >> 3), Xt = X0 + (tid & 7) * 4;
  const bool pre = a.do_step && a.vec && Yt < a.y_end && Xt >= 0 && Xt + 3 < a.W;
  const bool early = pre && a.preload;
  bool loaded = early;  // the step's streams of this thread are in its registers
  float4 pre_g = make_float4(0.f, 0.f, 0.f, 0.f), pre_t = pre_g, pre_f = pre_g, pre_m = pre_g, pre_v = pre_g;
  float4 pre_k = make_float4(1.f, 1.f, 1.f, 1.f);
  float4 pre_a[NA ? NA : 1];
#pragma unroll
  for (int k = 0; k < (NA ? NA : 1); ++k) pre_a[k] = pre_g;
  auto load_step_streams = [&]() {
    const AdamArgs& st = a.step;
    const size_t idx = (size_t)wrap(Yt - a.shift_y, a.H) * a.W + wrap(Xt - a.shift_x, a.W);
    pre_g = *reinterpret_cast<const float4*>(st.grad_flux + idx);
    pre_t = *reinterpret_cast<const float4*>(st.theta + idx), pre_f = *reinterpret_cast<const float4*>(st.flux_in + idx);
    if (!st.sgd) pre_m = *reinterpret_cast<const float4*>(st.m + idx), pre_v = *reinterpret_cast<const float4*>(st.v + idx);
    if (st.mask) pre_k = *reinterpret_cast<const float4*>(st.mask + idx);
#pragma unroll
    for (int k = 0; k < NA; ++k) pre_a[k] = *reinterpret_cast<const float4*>(st.addend[k] + idx);
  };
  if (touched) {
    const bool slots = a.winner && *a.flag != a.gen;
    // a wave's loads return in the order they were issued: FIRST the winner slots of all the thread's patches, then the
    // step's streams, then the rows -- the wait for the slots does not wait for the streams, and the streams have landed
    // by the time the rows have (the step's streams in front of the slots: measured slower, 56.9 against 49.9 us)
    constexpr int PER = (GATHER_MAX_P * GATHER_MAX_PX + 15) / 16;
    int slot_of[PER];  // slots: the winner's bucket slot (< 0: none); else the patch's row of gpatch
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int p = (tid >> 4) + 16 * j;
      slot_of[j] = -1;
      if (p < npy * npx) {
        const int py = py0 + p / npx, px = px0 + p % npx;
        slot_of[j] = slots ? a.winner[(size_t)py * a.nPx + px] : (py - a.row_begin) * a.nPx + px;
      }
    }
    if (early) load_step_streams();
    const float* base = slots ? a.grec : a.gpatch;
    // (every load unconditional -- row 0 stands in for "no row" -- so that all of them are in flight at once: with the load
    // under the condition the compiler emitted load, wait, LDS store per patch, six dependent round trips per thread)
    float4 rowv[PER];
#pragma unroll
    for (int j = 0; j < PER; ++j)
      rowv[j] = reinterpret_cast<const float4*>(base + (size_t)(slot_of[j] >= 0 ? slot_of[j] : 0) * D)[tid & 15];
#pragma unroll
    for (int j = 0; j < PER; ++j) {
      const int p = (tid >> 4) + 16 * j;
      if (p < npy * npx)
        *reinterpret_cast<float4*>(&rows[p][(tid & 15) * 4]) = slot_of[j] >= 0 ? rowv[j] : make_float4(0.f, 0.f, 0.f, 0.f);
    }
  } else if (early) {
    load_step_streams();
  }
  __syncthreads();
  const int Y = Y0 + (tid >> 3);
  if (Y >= a.y_end) return;
  int py_hi = Y / a.stride, py_lo = ceil_div_pos(Y - (P - 1), a.stride);
  if (py_lo < py0) py_lo = py0;
  if (py_hi > py1) py_hi = py1;
  const int yy = wrap(Y - a.shift_y, a.H);
  const int Xg = X0 + (tid & 7) * 4;  // the thread's group of four pixels of the rolled frame
  float sum[4];
  bool any[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int X = Xg + i;
    sum[i] = 0.f, any[i] = false;
    if (X < 0 || X >= a.W || !touched) continue;
    int px_hi = X / a.stride, px_lo = ceil_div_pos(X - (P - 1), a.stride);
    if (px_lo < px0) px_lo = px0;
    if (px_hi > px1) px_hi = px1;
    for (int py = py_lo; py <= py_hi; ++py) {
      const int r = Y - py * a.stride;
      for (int px = px_lo; px <= px_hi; ++px) {
        sum[i] += rows[(py - py0) * npx + (px - px0)][r * P + (X - px * a.stride)];  // (a zero row where a patch has no gradient)
        any[i] = true;
      }
    }
  }
  const size_t row = (size_t)yy * a.W;
  // image norm: term[i] = (coef * sum[i]) * n'(raw flux of the pixel) replaces coef * sum[i] below; a pixel without a
  // patch or with an exactly zero sum is not `any` any more (it receives nothing, n' is not evaluated)
  float term[4] = {0.f, 0.f, 0.f, 0.f};
  if (NORM) {
    const bool group = a.vec && Xg >= 0 && Xg + 3 < a.W;
    float fr[4] = {0.f, 0.f, 0.f, 0.f};
    if (group && a.do_step && a.raw_flux == a.step.flux_in) {
      if (!loaded) load_step_streams(), loaded = true;  // (JD_GMM_GATHER_PRELOAD=0: now, once, not here AND below)
      fr[0] = pre_f.x, fr[1] = pre_f.y, fr[2] = pre_f.z, fr[3] = pre_f.w;  // (the step's own flux stream, already here)
    } else if (group) {
      const float4 f4 = *reinterpret_cast<const float4*>(a.raw_flux + row + wrap(Xg - a.shift_x, a.W));
      fr[0] = f4.x, fr[1] = f4.y, fr[2] = f4.z, fr[3] = f4.w;
    } else {
#pragma unroll
      for (int i = 0; i < 4; ++i)
        if (Xg + i >= 0 && Xg + i < a.W) fr[i] = a.raw_flux[row + wrap(Xg + i - a.shift_x, a.W)];
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      any[i] = any[i] && sum[i] != 0.f;
      if (any[i]) term[i] = gather_normed_term(a, sum[i], fr[i]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i) term[i] = a.coef * sum[i];
  }
  if (a.band) {
#pragma unroll
    for (int i = 0; i < 4; ++i)
      if (Xg + i >= 0 && Xg + i < a.W) a.band[(size_t)(Y - a.y_begin) * a.W + Xg + i] = any[i] ? term[i] : 0.f;
    return;
  }
  if (a.vec && Xg >= 0 && Xg + 3 < a.W) {
    // the un-rolled column of the group is a multiple of 4 and the group does not wrap (W % 4 == 0)
    const size_t idx = row + wrap(Xg - a.shift_x, a.W);
    if (a.do_step) {
      const AdamArgs& st = a.step;  // (`pre` holds here: the loads were issued at the top of the kernel)
      if (!loaded) load_step_streams();  // (JD_GMM_GATHER_PRELOAD=0: behind the barrier, as before)
      const float4 g4 = pre_g, t4 = pre_t, f4 = pre_f, m4 = pre_m, v4 = pre_v, k4 = pre_k;
      float g[4] = {g4.x, g4.y, g4.z, g4.w};
      float th[4] = {t4.x, t4.y, t4.z, t4.w}, f[4] = {f4.x, f4.y, f4.z, f4.w};
      float m[4] = {m4.x, m4.y, m4.z, m4.w}, v[4] = {v4.x, v4.y, v4.z, v4.w};
      float mk[4] = {k4.x, k4.y, k4.z, k4.w};
#pragma unroll
      for (int k = 0; k < NA; ++k) g[0] += pre_a[k].x, g[1] += pre_a[k].y, g[2] += pre_a[k].z, g[3] += pre_a[k].w;
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        if (any[i]) g[i] += term[i];
        adam_pixel(th[i], f[i], m[i], v[i], g[i], mk[i], st);
      }
      *reinterpret_cast<float4*>(st.theta + idx) = make_float4(th[0], th[1], th[2], th[3]);
      *reinterpret_cast<float4*>(st.flux_out + idx) = make_float4(f[0], f[1], f[2], f[3]);
      if (!st.sgd) {
        *reinterpret_cast<float4*>(st.m + idx) = make_float4(m[0], m[1], m[2], m[3]);
        *reinterpret_cast<float4*>(st.v + idx) = make_float4(v[0], v[1], v[2], v[3]);
      }
    } else if (any[0] || any[1] || any[2] || any[3]) {
      float4 g4 = *reinterpret_cast<const float4*>(a.grad + idx);
      if (any[0]) g4.x += term[0];
      if (any[1]) g4.y += term[1];
      if (any[2]) g4.z += term[2];
      if (any[3]) g4.w += term[3];
      *reinterpret_cast<float4*>(a.grad + idx) = g4;
    }
    return;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {  // a group that straddles the image border (or W % 4 != 0): pixel by pixel
    const int X = Xg + i;
    if (X < 0 || X >= a.W) continue;
    const size_t idx = row + wrap(X - a.shift_x, a.W);
    if (a.do_step) {
      const AdamArgs& st = a.step;
      float g = st.grad_flux[idx];
#pragma unroll
      for (int k = 0; k < NA; ++k) g += st.addend[k][idx];
      if (any[i]) g += term[i];
      float th = st.theta[idx], f = st.flux_in[idx], m = st.sgd ? 0.f : st.m[idx], v = st.sgd ? 0.f : st.v[idx];
      const float mk = st.mask ? st.mask[idx] : 1.f;
      adam_pixel(th, f, m, v, g, mk, st);
      st.theta[idx] = th, st.flux_out[idx] = f;
      if (!st.sgd) st.m[idx] = m, st.v[idx] = v;
    } else if (any[i]) {
      a.grad[idx] += term[i];
    }
  }
}

// grad[un-rolled (Y, X)] += sum over the bands that hold row Y, in band order: the pieces of a sharded prior gradient
// (band b = rows [y_begin[b], y_end[b]) of the rolled frame, at bands + b * chunk) put back into the gradient image.
// Every rank adds the same numbers in the same order: replicas stay bit-identical.
constexpr int BANDS_MAX = 64;
template <int NB>  // band ranges a launch carries: 8, 16 or BANDS_MAX
struct AddBandsArgsT {
  float* grad;
  const float* bands;
  size_t chunk;
  int H, W, shift_y, shift_x, n_bands, y_lo, y_hi;
  const int* shift_dev;  // nullable, device [2] = {shift_y, shift_x} residues: read instead of the two members above (use_device_shift)
  int y_begin[NB], y_end[NB];
};
using AddBandsArgs = AddBandsArgsT<BANDS_MAX>;  // (what the host fills; launches copy the ranges into the size they take)

template <int NB>
static AddBandsArgsT<NB> narrow_bands(const AddBandsArgs& a) {
  AddBandsArgsT<NB> n{};
  n.grad = a.grad, n.bands = a.bands, n.chunk = a.chunk, n.H = a.H, n.W = a.W, n.shift_y = a.shift_y, n.shift_x = a.shift_x;
  n.n_bands = a.n_bands, n.y_lo = a.y_lo, n.y_hi = a.y_hi, n.shift_dev = a.shift_dev;
  for (int b = 0; b < NB; ++b) n.y_begin[b] = a.y_begin[b], n.y_end[b] = a.y_end[b];
  return n;
}

// The loop over the bands is UNROLLED over the NB ranges of the launch: indexing the by-value argument arrays with a runtime
// band number made the compiler copy the whole argument block to scratch in every thread (584 bytes per lane: the band sum +
// optimizer step of a 2048^2 image took 147 us, 46 % of a rank's share of an 8-way step; round 5), and staging the ranges in
// LDS by 64 compile-time compares compiled to 30 000 instructions (204 us).  Launches carry 8, 16 or 64 ranges.
template <int NB>
__global__ __launch_bounds__(256) void add_rolled_bands_kernel(AddBandsArgsT<NB> a) {
  use_device_shift(a);
  const int Y = a.y_lo + blockIdx.y;
  const int X = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (X >= a.W || Y >= a.y_hi) return;
  float4 sum = make_float4(0.f, 0.f, 0.f, 0.f);
  bool any = false;
  const bool vec = (a.W & 3) == 0 && (a.chunk & 3) == 0;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int yb = a.y_begin[b], ye = a.y_end[b];  // (unused ranges are empty: y_begin = y_end = 0)
    if (Y < yb || Y >= ye) continue;
    const float* row = a.bands + (size_t)b * a.chunk + (size_t)(Y - yb) * a.W + X;
    if (vec) {
      const float4 v = *reinterpret_cast<const float4*>(row);
      sum.x += v.x, sum.y += v.y, sum.z += v.z, sum.w += v.w;
    } else {
      sum.x += row[0];
      if (X + 1 < a.W) sum.y += row[1];
      if (X + 2 < a.W) sum.z += row[2];
      if (X + 3 < a.W) sum.w += row[3];
    }
    any = true;
  }
  if (!any) return;
  float* out = a.grad + (size_t)wrap(Y - a.shift_y, a.H) * a.W;
  const float v[4] = {sum.x, sum.y, sum.z, sum.w};
#pragma unroll
  for (int i = 0; i < 4; ++i)
    if (X + i < a.W) out[wrap(X + i - a.shift_x, a.W)] += v[i];
}

// The same sum, followed at once by the optimizer step of the pixel (sharded fits: the bands of the prior's gradient are
// its last term): g = grad[pixel] + sum over the bands, the additions of add_rolled_bands_kernel in the same order, then
// adam_pixel -- one pass over the gradient image and one launch less per step.  A thread owns an ALIGNED group of four
// pixels of the un-rolled image (16-byte accesses to the optimizer state; W % 4 == 0) and reads the four rolled-frame
// band values of every band that holds its row one by one.
template <int NB>
__global__ __launch_bounds__(256) void add_rolled_bands_step_kernel(AddBandsArgsT<NB> a, AdamArgs st) {
  use_device_shift(a);
  use_device_bias(st);
  const int yy = blockIdx.y;
  const int xx = (blockIdx.x * 256 + threadIdx.x) * 4;
  if (xx >= a.W) return;
  const int Y = wrap(yy + a.shift_y, a.H);  // rolled-frame row of this image row (shift in [0, H))
  float sum[4] = {0.f, 0.f, 0.f, 0.f};
  bool any = false;
  int X[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) X[i] = wrap(xx + i + a.shift_x, a.W);
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int yb = a.y_begin[b], ye = a.y_end[b];
    if (Y < yb || Y >= ye) continue;
    const float* row = a.bands + (size_t)b * a.chunk + (size_t)(Y - yb) * a.W;
#pragma unroll
    for (int i = 0; i < 4; ++i) sum[i] += row[X[i]];
    any = true;
  }
  const size_t idx = (size_t)yy * a.W + xx;
  const float4 g4 = *reinterpret_cast<const float4*>(st.grad_flux + idx);
  float g[4] = {g4.x, g4.y, g4.z, g4.w};
  const float4 t4 = *reinterpret_cast<const float4*>(st.theta + idx), f4 = *reinterpret_cast<const float4*>(st.flux_in + idx);
  float th[4] = {t4.x, t4.y, t4.z, t4.w}, f[4] = {f4.x, f4.y, f4.z, f4.w}, m[4] = {0.f, 0.f, 0.f, 0.f}, v[4] = {0.f, 0.f, 0.f, 0.f};
  float mk[4] = {1.f, 1.f, 1.f, 1.f};
  if (!st.sgd) {
    const float4 m4 = *reinterpret_cast<const float4*>(st.m + idx), v4 = *reinterpret_cast<const float4*>(st.v + idx);
    m[0] = m4.x, m[1] = m4.y, m[2] = m4.z, m[3] = m4.w, v[0] = v4.x, v[1] = v4.y, v[2] = v4.z, v[3] = v4.w;
  }
  if (st.mask) {
    const float4 k4 = *reinterpret_cast<const float4*>(st.mask + idx);
    mk[0] = k4.x, mk[1] = k4.y, mk[2] = k4.z, mk[3] = k4.w;
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    if (any) g[i] += sum[i];
    adam_pixel(th[i], f[i], m[i], v[i], g[i], mk[i], st);
  }
  *reinterpret_cast<float4*>(st.theta + idx) = make_float4(th[0], th[1], th[2], th[3]);
  *reinterpret_cast<float4*>(st.flux_out + idx) = make_float4(f[0], f[1], f[2], f[3]);
  if (!st.sgd) {
    *reinterpret_cast<float4*>(st.m + idx) = make_float4(m[0], m[1], m[2], m[3]);
    *reinterpret_cast<float4*>(st.v + idx) = make_float4(v[0], v[1], v[2], v[3]);
  }
}

template <int NA>
static void tile_launch(bool has_norm, dim3 grid, const GmmGatherArgs& ga, hipStream_t s) {
  static_assert(NA <= ADDEND_MAX, "AdamArgs::addend");
  if (has_norm) gmm_gather_tile_kernel<true, NA><<<grid, 256, 0, s>>>(ga);
  else gmm_gather_tile_kernel<false, NA><<<grid, 256, 0, s>>>(ga);
}

int launch_gather(const GmmGatherArgs& ga, hipStream_t s) {
  const bool has_norm = ga.norm.kind != NORM_IDENTITY;
  ProfScope prof(JD_KERNEL_GMM_GATHER, s);
  // option JD_GMM_GATHER_TILED = 0: the per-pixel kernel (testing)
  if (ga.stride >= 4 && opt_value(OPT_GMM_GATHER_TILED, 1) != 0) {
    // (x: the first tile starts up to 3 pixels left of the image so that the pixel groups are aligned un-rolled)
    dim3 grid((ga.W + 3 + GATHER_T - 1) / GATHER_T, (ga.y_end - ga.y_begin + GATHER_T - 1) / GATHER_T);
    int na = 0;
    while (ga.do_step && na < ADDEND_MAX && ga.step.addend[na]) ++na;
    switch (na) {
      case 0: tile_launch<0>(has_norm, grid, ga, s); break;
      case 1: tile_launch<1>(has_norm, grid, ga, s); break;
      case 2: tile_launch<2>(has_norm, grid, ga, s); break;
      case 3: tile_launch<3>(has_norm, grid, ga, s); break;
      default: tile_launch<4>(has_norm, grid, ga, s); break;
    }
  } else {
    dim3 grid((ga.W + 255) / 256, ga.y_end - ga.y_begin);
    if (has_norm) gmm_gather_kernel<true><<<grid, 256, 0, s>>>(ga);
    else gmm_gather_kernel<false><<<grid, 256, 0, s>>>(ga);
  }
  JD_LAUNCH_CHECK();
  return JD_OK;
}

}  // namespace jd

using namespace jd;

extern "C" int jd_add_rolled_bands(float* grad, int H, int W, int shift_y, int shift_x, const float* bands,
                                   size_t chunk_floats, int n_bands, const int* y_begin, const int* y_end, void* stream) {
  JD_REQUIRE(grad && bands && y_begin && y_end, "jd_add_rolled_bands: null argument");
  JD_REQUIRE(n_bands >= 1 && n_bands <= BANDS_MAX, "jd_add_rolled_bands: %d bands not in [1, %d]", n_bands, BANDS_MAX);
  AddBandsArgs a{};
  a.grad = grad, a.bands = bands, a.chunk = chunk_floats, a.H = H, a.W = W, a.n_bands = n_bands;
  a.shift_y = roll_residue(shift_y, H), a.shift_x = roll_residue(shift_x, W);
  a.y_lo = H, a.y_hi = 0;
  for (int b = 0; b < n_bands; ++b) {
    JD_REQUIRE(y_begin[b] >= 0 && y_begin[b] <= y_end[b] && y_end[b] <= H && (size_t)(y_end[b] - y_begin[b]) * W <= chunk_floats,
               "jd_add_rolled_bands: band %d rows [%d, %d) do not fit", b, y_begin[b], y_end[b]);
    a.y_begin[b] = y_begin[b], a.y_end[b] = y_end[b];
    if (y_begin[b] < y_end[b]) a.y_lo = std::min(a.y_lo, y_begin[b]), a.y_hi = std::max(a.y_hi, y_end[b]);
  }
  if (a.y_lo >= a.y_hi) return JD_OK;
  dim3 grid((W + 1023) / 1024, a.y_hi - a.y_lo);
  if (n_bands <= 8) add_rolled_bands_kernel<8><<<grid, 256, 0, as_stream(stream)>>>(narrow_bands<8>(a));
  else if (n_bands <= 16) add_rolled_bands_kernel<16><<<grid, 256, 0, as_stream(stream)>>>(narrow_bands<16>(a));
  else add_rolled_bands_kernel<BANDS_MAX><<<grid, 256, 0, as_stream(stream)>>>(a);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

extern "C" int jd_add_rolled_bands_step(int H, int W, int shift_y, int shift_x, const float* bands, size_t chunk_floats,
                                        int n_bands, const int* y_begin, const int* y_end, const jd_step* step, void* stream) {
  JD_REQUIRE(bands && y_begin && y_end && step, "jd_add_rolled_bands_step: null argument");
  JD_REQUIRE(step->theta && step->flux_in && step->flux_out && step->grad_flux, "jd_add_rolled_bands_step: null image");
  JD_REQUIRE(step->sgd || (step->exp_avg && step->exp_avg_sq), "jd_add_rolled_bands_step: Adam needs its moment images");
  JD_REQUIRE(!step->addend[0], "jd_add_rolled_bands_step: addend images are not supported (use jd_add_rolled_bands + jd_adam_step_addends)");
  JD_REQUIRE(n_bands >= 1 && n_bands <= BANDS_MAX, "jd_add_rolled_bands_step: %d bands not in [1, %d]", n_bands, BANDS_MAX);
  JD_REQUIRE(W % 4 == 0 && aligned16(step->theta) && aligned16(step->flux_in) && aligned16(step->flux_out) &&
                 aligned16(step->grad_flux) && aligned16(step->exp_avg) && aligned16(step->exp_avg_sq) && aligned16(step->mask),
             "jd_add_rolled_bands_step: needs W %% 4 == 0 and 16-byte aligned images (use jd_add_rolled_bands + jd_adam_step)");
  AddBandsArgs a{};
  a.grad = nullptr, a.bands = bands, a.chunk = chunk_floats, a.H = H, a.W = W, a.n_bands = n_bands;
  a.shift_y = roll_residue(shift_y, H), a.shift_x = roll_residue(shift_x, W);
  for (int b = 0; b < n_bands; ++b) {
    JD_REQUIRE(y_begin[b] >= 0 && y_begin[b] <= y_end[b] && y_end[b] <= H && (size_t)(y_end[b] - y_begin[b]) * W <= chunk_floats,
               "jd_add_rolled_bands_step: band %d rows [%d, %d) do not fit", b, y_begin[b], y_end[b]);
    a.y_begin[b] = y_begin[b], a.y_end[b] = y_end[b];
  }
  AdamArgs st{};
  st.theta = step->theta, st.flux_in = step->flux_in, st.flux_out = step->flux_out, st.grad_flux = const_cast<float*>(step->grad_flux);
  st.m = step->exp_avg, st.v = step->exp_avg_sq, st.mask = step->mask, st.n = (size_t)H * W;
  st.step_size = step->step_size, st.beta1 = step->beta1, st.beta2 = step->beta2, st.one_minus_beta1 = step->one_minus_beta1;
  st.one_minus_beta2 = step->one_minus_beta2, st.bias2_sqrt = step->bias2_sqrt, st.eps = step->eps, st.lr = step->lr;
  st.zero_grad = 0, st.sgd = step->sgd ? 1 : 0, st.linear = step->use_log_flux ? 0 : 1, st.bias_dev = step->bias_dev;
  dim3 grid((W + 1023) / 1024, H);
  ProfScope prof(JD_KERNEL_ADAM, as_stream(stream));
  if (n_bands <= 8) add_rolled_bands_step_kernel<8><<<grid, 256, 0, as_stream(stream)>>>(narrow_bands<8>(a), st);
  else if (n_bands <= 16) add_rolled_bands_step_kernel<16><<<grid, 256, 0, as_stream(stream)>>>(narrow_bands<16>(a), st);
  else add_rolled_bands_step_kernel<BANDS_MAX><<<grid, 256, 0, as_stream(stream)>>>(a, st);
  JD_LAUNCH_CHECK();
  return JD_OK;
}
