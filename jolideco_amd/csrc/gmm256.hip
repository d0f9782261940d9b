// GMM patch prior for 16x16 patches (D = 256) on gfx950 (CDNA4): one dense fp32 path.
//
// Per patch x (mean subtracted) and component k, as for 8x8 patches (gmm.hip):
//     y_k = x^T P'_k - m'_k ,  q_k = sum_j y_kj^2 ,  l_k = c_k - q_k / 2 ,  v = max_k l_k | logsumexp_k l_k
// with P'_k = P_k diag(sqrt w) the 256 x 256 upper triangular precision factor (pixel weights folded into the columns).
// The product runs on v_mfma_f32_16x16x4_f32 (bit-for-bit an fmaf chain in pixel order, here per 64 pixels):
//     M = whitened coordinate j (16 per MFMA), N = patch (16 per MFMA), K = pixel (4 per MFMA).
//
// Layout.  One block = 4 waves (one per SIMD) = one TILE of 16 NB patches, and the block loops over the components:
// the per-patch state stays in registers and the logsumexp is exact in one sweep.  NB = 2 (two 16-patch
// halves, two independent accumulator chains per fragment of a factor) once that gives every CU a block, else NB = 1
// (tile_halves).
//   * The 4 waves split the COLUMNS of P'_k: the factor is taken in 4 slabs of 64 columns, and in slab s wave w owns the
//     16-column block jb = 4 s + w (s even) or 4 s + 3 - w (s odd) -- with a triangular factor block jb needs the pixels
//     below 16 (jb + 1) only, and the alternation gives every wave the same 34 of the 136 non-zero 16 x 16 blocks.
//   * Nobody shares a fragment of the factor inside the block, so a slab does not go through LDS: every wave streams its
//     16-column slab from L2 straight into registers, 64 pixels x 16 columns (4 KB: four 16-byte loads per lane) at a
//     time, double buffered, prepared on the host in A-fragment order.  A chunk of 64 pixels is skipped when it lies
//     wholly below the diagonal (exact zeros: no bit changes); a non-triangular set of factors
//     takes the instantiation that skips nothing.
//   * The tile's 32 patches live in REGISTERS for the whole component loop: lane (g, n) holds pixels 4 s + g,
//     s = 0 .. 63, of patches n and 16 + n -- exactly the B operands of the 64 pixel steps (64 VGPRs per half), so the
//     hot loop reads no LDS at all; the two 16-patch halves are the two independent accumulators the 40-cycle MFMA
//     latency asks for.
//   * C puts the patch on the lane and the coordinate in the registers: a wave's share of q_k is an in-lane sum + two
//     lane swaps; the four shares meet in a 1 KB double-buffered LDS array, one barrier per component, and are added in
//     wave order.  Every wave then updates its own copy of the running (max, arg-max) | (max, sum-exp) state.
// Backward: the same tile recomputes y_k for the components it needs (max mode: the distinct winners of its patches,
// logsumexp: all K with r_k = exp(l_k - lse)), multiplies by -r_k and runs gamma += P'_k y on the matrix cores with the
// accumulators of the first product as the B operand (host-prepared fragments in that order, as in gmm.hip); a wave adds
// up its column share over all components in 64 NB accumulator registers, the four shares are added in wave order through
// LDS once per tile, the adjoint of the mean subtraction is applied and one 256-float row per patch is written.
// Overlap-add: a per-pixel gather over the up to ceil(16 / stride)^2 patches of a pixel in fixed order.
// Patch norm (template parameter PN): PN_SUBTRACT_MEAN is the x above; PN_STD standardizes, x = (p - mean) / mean
// (jolideco/utils/norms.py:106-112): a correctly rounded division in load_patches, and in the row epilogue
// dv/dp_j = (gamma_j - mean(gamma) - (gamma . x) / 256) / mean with x recomputed from the image.
#include <cmath>
#include <type_traits>
#include <vector>

#include "gmm256.h"
#include "kernels.h"

namespace jd {

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int P16 = 16;                  // patch edge
constexpr int D256 = 256;                // features per patch
constexpr int NBLK = 16;                 // 16-blocks per dimension of a factor
constexpr int FRAG_FLOATS = D256 * D256;  // per component: [jb 16][st4 16][lane 64][e 4] (forward) | [ib 16][jb 16][lane 64][r 4]
constexpr int TILE_MAX = 32;             // patches per block: 16 NB, NB = 1 | 2 halves of 16 (the N of one MFMA)
constexpr int GPITCH = 260;              // floats per patch row of the block's gradient sum in LDS (16-byte aligned rows)

enum { M_MAX = 0, M_LSE = 1, M_DENSE = 2 };
enum { PN_SUBTRACT_MEAN = 0, PN_STD = 1 };  // jd_gmm_set_patch_norm

struct Args256 {
  const float* image;    // (H, W) | M_DENSE: (n, 256) explicit patches
  const float* afrag;    // K * FRAG_FLOATS
  const float* gfrag;    // K * FRAG_FLOATS
  const float* mfrag;    // K * 256: -m'[j]
  const float* const_k;  // K constants c_k, then K residuals (gmm256_set_const_residual; read under PN_STD only)
  int K, H, W, stride, nPx, shift_y, shift_x;
  const int* shift_dev;  // nullable, device [2] = {shift_y, shift_x} residues: read instead of the two members above
  int n_end;             // number of patches
  int32_t* argmax;       // max mode: winner per patch, -1 for a filtered patch (forward writes, backward reads)
  float* vpatch;         // logsumexp per patch (forward writes, backward reads); nullable in the forward kernel
  float* dense_out;      // M_DENSE: (n, K)
  double* partials;      // one per block
  float* gpatch;         // (n, 256) gradient rows
};

__device__ __forceinline__ int wrap(int v, int n) {  // v mod n for -n <= v < 2 n
  v = v < 0 ? v + n : v;
  return v >= n ? v - n : v;
}

__device__ __forceinline__ float f4_get(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

// v(lane) + v(lane ^ 16) + v(lane ^ 32) + v(lane ^ 48) on every lane (row / half swaps: VALU only)
__device__ __forceinline__ float sum_lane_groups(float v) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  const float s = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(s), __float_as_uint(s), false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

template <int I, int N, class F>
__device__ __forceinline__ void static_for(F&& f) {
  if constexpr (I < N) {
    f(std::integral_constant<int, I>{});
    static_for<I + 1, N>(f);
  }
}

// The (slab, 64-pixel chunk) pairs of a component in the order they are visited: triangular factors need the chunks
// c <= s of slab s (10 pairs), dense ones all 16.
template <bool TRI>
struct Seq {
  static constexpr int N = TRI ? 10 : 16;
  static constexpr int slab(int i) { return TRI ? (i >= 6 ? 3 : i >= 3 ? 2 : i >= 1 ? 1 : 0) : i / 4; }
  static constexpr int chunk(int i) { return TRI ? i - slab(i) * (slab(i) + 1) / 2 : i % 4; }
};

// 16-column block wave `wave` owns in slab s
__device__ __forceinline__ int wave_block(int s, int wave) { return 4 * s + ((s & 1) ? 3 - wave : wave); }

// The 4 fragments (16 pixels x 16 columns each) of chunk c of block jb; frag = fragment array of the component + lane
__device__ __forceinline__ void load_chunk(float4 (&buf)[4], const float4* frag, int jb, int c) {
#pragma unroll
  for (int u = 0; u < 4; ++u) buf[u] = frag[(size_t)((jb * NBLK + 4 * c + u) * 64)];
}

// The tile's patches in B-operand order: x[nb][s] = pixel 4 s + g of patch tile_base + 16 nb + n16, mean subtracted;
// ok[nb]: the patch exists and passes the reference's `> -1e5` filter (all zeros otherwise).  The mean is summed in ONE
// order (64 pixels in lane order, then the four lane groups) by the forward and the backward kernel, which therefore see
// the same bits.  mean_out[nb]: that mean (the row epilogue of the standardized norm divides by it).
template <bool DENSE, int NB, int PN = PN_SUBTRACT_MEAN>
__device__ __forceinline__ void load_patches(float (&x)[NB][64], bool (&ok)[NB], const Args256& a, int tile_base, int g,
                                             int n16, float* mean_out = nullptr) {
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int n = tile_base + 16 * nb + n16;
    const bool valid = n < a.n_end;
    if (DENSE) {
#pragma unroll
      for (int s = 0; s < 64; ++s) x[nb][s] = valid ? a.image[(size_t)n * D256 + 4 * s + g] : 0.f;
      ok[nb] = valid;
      continue;
    }
    const int py = valid ? n / a.nPx : 0, px = valid ? n % a.nPx : 0;
    bool sel = true;
    float part = 0.f;
#pragma unroll
    for (int r = 0; r < P16; ++r) {
      const int yy = wrap(py * a.stride + r - a.shift_y, a.H);
      const float* row = a.image + (size_t)yy * a.W;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int xx = wrap(px * a.stride + 4 * q + g - a.shift_x, a.W);
        const float v = valid ? row[xx] : 0.f;
        x[nb][4 * r + q] = v;
        sel = sel && (v > -1e5f);  // patches/core.py:215
        part += v;
      }
    }
    const float mean = sum_lane_groups(part) * (1.f / 256.f);  // SubtractMeanPatchNorm
    int seli = sel ? 1 : 0;
    seli &= __shfl_xor(seli, 16, 64);
    seli &= __shfl_xor(seli, 32, 64);
    ok[nb] = valid && seli != 0;
    if constexpr (PN == PN_STD) {
      if (mean_out) mean_out[nb] = mean;
#pragma unroll
      for (int s = 0; s < 64; ++s) x[nb][s] = ok[nb] ? (x[nb][s] - mean) / mean : 0.f;
    } else {
#pragma unroll
      for (int s = 0; s < 64; ++s) x[nb][s] = ok[nb] ? x[nb][s] - mean : 0.f;
    }
  }
}

// y[s][nb] = -m' + P'^T x for the wave's block of slab s and the 16-patch half nb: an fmaf chain in pixel order per
// 64-pixel chunk, the chunks added in order.
// abuf[0] holds chunk 0 of component k on entry and chunk 0 of component k_next on exit.
template <bool TRI, int NB>
__device__ __forceinline__ void whiten(f32x4 (&y)[4][NB], const float (&x)[NB][64], float4 (&abuf)[2][4], const Args256& a,
                                       int k, int k_next, int lane, int wave) {
  using S = Seq<TRI>;
  const float4* af = reinterpret_cast<const float4*>(a.afrag) + (size_t)k * (FRAG_FLOATS / 4) + lane;
  const float4* af_next = reinterpret_cast<const float4*>(a.afrag) + (size_t)k_next * (FRAG_FLOATS / 4) + lane;
  const float4* mf = reinterpret_cast<const float4*>(a.mfrag) + (size_t)k * (D256 / 4) + (lane >> 4);
  static_for<0, S::N>([&](auto I) {
    constexpr int i = decltype(I)::value;
    constexpr int s = S::slab(i), c = S::chunk(i);
    if constexpr (i + 1 < S::N)
      load_chunk(abuf[(i + 1) & 1], af, wave_block(S::slab(i + 1), wave), S::chunk(i + 1));
    else
      load_chunk(abuf[0], af_next, wave_block(0, wave), 0);  // (S::N is even: the last chunk sits in abuf[1])
    // one accumulator chain per 64-pixel chunk, added to the running sum afterwards: blocked summation -- the rounding of
    // a 256-term fmaf chain showed in the logsumexp responsibilities (|l| ~ 1e4: 1 ulp = 1e-3 .. 4e-3)
    f32x4 part[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) part[nb] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
          part[nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4_get(abuf[i & 1][u], e), x[nb][16 * c + 4 * u + e], part[nb], 0, 0, 0);
    if constexpr (c == 0) {
      const float4 m = mf[wave_block(s, wave) * 4];
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) y[s][nb] = f32x4{m.x, m.y, m.z, m.w} + part[nb];
    } else {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) y[s][nb] += part[nb];
    }
  });
}

// The wave's share of q for half nb: 16 squares in register order, then the four lane groups
template <int NB>
__device__ __forceinline__ float wave_q(const f32x4 (&y)[4][NB], int nb) {
  float q = 0.f;
#pragma unroll
  for (int s = 0; s < 4; ++s)
#pragma unroll
    for (int r = 0; r < 4; ++r) q = fmaf(y[s][nb][r], y[s][nb][r], q);
  return sum_lane_groups(q);
}

// l_k of the lane's two patches: the four waves' shares of q meet in qbuf[k & 1] and are added in wave order.  One
// barrier per component: the buffer written for component k + 2 is the one read for k, and no wave gets there before
// every wave has passed the barrier of k + 1, i.e. has finished reading.
template <int NB>
__device__ __forceinline__ void exchange_q(float (&l)[NB], const f32x4 (&y)[4][NB], float (*qbuf)[4][TILE_MAX], int slot,
                                           float ck, int lane, int wave) {
  const int g = lane >> 4, n16 = lane & 15;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const float q = wave_q<NB>(y, nb);
    if (g == 0) qbuf[slot][wave][16 * nb + n16] = q;
  }
  __syncthreads();
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int p = 16 * nb + n16;
    const float q = (qbuf[slot][0][p] + qbuf[slot][1][p]) + (qbuf[slot][2][p] + qbuf[slot][3][p]);
    l[nb] = fmaf(-0.5f, q, ck);
  }
}

template <int MODE, bool TRI, int NB, int PN = PN_SUBTRACT_MEAN>
__global__ __launch_bounds__(256, 1) void gmm256_fwd_kernel(Args256 a) {
  if (a.shift_dev) a.shift_y = a.shift_dev[0], a.shift_x = a.shift_dev[1];
  __shared__ float qbuf[2][4][TILE_MAX];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, n16 = lane & 15;
  const int tile_base = blockIdx.x * (16 * NB);

  float x[NB][64];
  bool ok[NB];
  load_patches<MODE == M_DENSE, NB, PN>(x, ok, a, tile_base, g, n16);

  float best[NB], aux[NB];  // aux: arg-max (as int bits) | sum-exp
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) best[nb] = -INFINITY, aux[nb] = 0.f;
  float4 abuf[2][4];
  load_chunk(abuf[0], reinterpret_cast<const float4*>(a.afrag) + lane, wave_block(0, wave), 0);
  for (int k = 0; k < a.K; ++k) {
    f32x4 y[4][NB];
    whiten<TRI, NB>(y, x, abuf, a, k, k + 1 < a.K ? k + 1 : k, lane, wave);
    float l[NB];
    exchange_q<NB>(l, y, qbuf, k & 1, a.const_k[k], lane, wave);
    if constexpr (PN == PN_STD) {  // the residual of c_k (jd_gmm_set_const_residual): l is a small difference under this norm
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) l[nb] += a.const_k[a.K + k];
    }
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
      if (MODE == M_MAX) {
        const bool better = l[nb] > best[nb];  // strict: the lowest component wins a tie, like torch.max
        best[nb] = better ? l[nb] : best[nb];
        aux[nb] = better ? __int_as_float(k) : aux[nb];
      } else if (MODE == M_LSE) {
        const bool better = l[nb] > best[nb];
        const float e = expf(better ? best[nb] - l[nb] : l[nb] - best[nb]);
        aux[nb] = better ? fmaf(aux[nb], e, 1.f) : aux[nb] + e;
        best[nb] = better ? l[nb] : best[nb];
      } else {
        const int n = tile_base + 16 * nb + n16;
        if (wave == 0 && g == 0 && n < a.n_end) a.dense_out[(size_t)n * a.K + k] = l[nb];
      }
    }
  }
  if (MODE == M_DENSE || wave != 0) return;

  double local = 0.0;
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int n = tile_base + 16 * nb + n16;
    const float v = MODE == M_LSE ? best[nb] + logf(aux[nb]) : best[nb];
    if (g == 0 && n < a.n_end) {
      if (MODE == M_MAX && a.argmax) a.argmax[n] = ok[nb] ? __float_as_int(aux[nb]) : -1;
      if (MODE == M_LSE && a.vpatch) a.vpatch[n] = v;
      if (ok[nb]) local += (double)v;
    }
  }
  local = wave_sum(local);
  if (lane == 0) a.partials[blockIdx.x] = local;
}

template <int MODE, bool TRI, int NB, int PN = PN_SUBTRACT_MEAN>
__global__ __launch_bounds__(256, 1) void gmm256_bwd_kernel(Args256 a) {
  constexpr int TILE = 16 * NB;
  if (a.shift_dev) a.shift_y = a.shift_dev[0], a.shift_x = a.shift_dev[1];
  __shared__ float qbuf[2][4][TILE_MAX];
  __shared__ __attribute__((aligned(16))) float gs[TILE * GPITCH];
  __shared__ int klist[TILE];
  __shared__ int nlist_s;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 4, n16 = lane & 15;
  const int tile_base = blockIdx.x * TILE;

  float x[NB][64];
  bool ok[NB];
  __shared__ float pmean_s[PN == PN_STD ? TILE : 1];  // PN_STD: mean of every patch of the tile, NaN for a filtered one
  if constexpr (PN == PN_STD) {
    float pmean[NB];
    load_patches<false, NB, PN>(x, ok, a, tile_base, g, n16, pmean);
    if (wave == 0 && g == 0) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) pmean_s[16 * nb + n16] = ok[nb] ? pmean[nb] : NAN;  // (read behind the barriers below)
    }
  } else {
    load_patches<false, NB>(x, ok, a, tile_base, g, n16);
  }

  int win[NB];
  float lse[NB];
#pragma unroll
  for (int nb = 0; nb < NB; ++nb) {
    const int n = tile_base + 16 * nb + n16;
    win[nb] = -1, lse[nb] = 0.f;
    if (n < a.n_end) {
      if (MODE == M_MAX) win[nb] = a.argmax[n];
      else lse[nb] = a.vpatch[n];
    }
  }
  // components the tile needs
  int nlist = a.K;
  if (MODE == M_MAX) {
    if (threadIdx.x == 0) {
      int cnt = 0;
      for (int p = 0; p < TILE; ++p) {
        const int n = tile_base + p;
        const int w = n < a.n_end ? a.argmax[n] : -1;
        bool seen = w < 0 || w >= a.K;
        for (int i = 0; i < cnt && !seen; ++i) seen = klist[i] == w;
        if (!seen) klist[cnt++] = w;
      }
      nlist_s = cnt;
    }
    __syncthreads();
    nlist = nlist_s;
  }

  f32x4 acc[NBLK][NB];
#pragma unroll
  for (int ib = 0; ib < NBLK; ++ib)
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) acc[ib][nb] = f32x4{0.f, 0.f, 0.f, 0.f};

  using S = Seq<TRI>;
  float4 abuf[2][4];
  if (nlist > 0)
    load_chunk(abuf[0], reinterpret_cast<const float4*>(a.afrag) + (size_t)(MODE == M_MAX ? klist[0] : 0) * (FRAG_FLOATS / 4) + lane,
               wave_block(0, wave), 0);
  for (int idx = 0; idx < nlist; ++idx) {
    const int inext = idx + 1 < nlist ? idx + 1 : idx;
    const int k = MODE == M_MAX ? klist[idx] : idx, k_next = MODE == M_MAX ? klist[inext] : inext;
    // gamma fragments [ib][jb][lane][r]: chunk c of block jb = row blocks ib = 4 c .. 4 c + 3
    const float4* gf = reinterpret_cast<const float4*>(a.gfrag) + (size_t)k * (FRAG_FLOATS / 4) + lane;
    auto load_g = [&](float4(&buf)[4], int jb, int c) {
#pragma unroll
      for (int u = 0; u < 4; ++u) buf[u] = gf[(size_t)(((4 * c + u) * NBLK + jb) * 64)];
    };
    float4 gbuf[2][4];
    load_g(gbuf[0], wave_block(0, wave), 0);

    f32x4 y[4][NB];
    whiten<TRI, NB>(y, x, abuf, a, k, k_next, lane, wave);
    float r[NB];
    if (MODE == M_MAX) {
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) r[nb] = win[nb] == k ? 1.f : 0.f;
    } else {
      float l[NB];
      exchange_q<NB>(l, y, qbuf, idx & 1, a.const_k[k], lane, wave);
      if constexpr (PN == PN_STD) {  // (the forward kernel's l)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) l[nb] += a.const_k[a.K + k];
      }
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) r[nb] = ok[nb] ? expf(l[nb] - lse[nb]) : 0.f;
    }
#pragma unroll
    for (int s = 0; s < 4; ++s)
#pragma unroll
      for (int nb = 0; nb < NB; ++nb) y[s][nb] *= -r[nb];
    // gamma[16 ib + .][n] += P'[16 ib + ., 16 jb + .] y[16 jb + .][n]: the accumulators of the first product are the B
    // operand (lane group g holds coordinate 16 jb + 4 g + r in register r; the fragments are laid out to match)
    static_for<0, S::N>([&](auto I) {
      constexpr int i = decltype(I)::value;
      constexpr int s = S::slab(i), c = S::chunk(i);
      if constexpr (i + 1 < S::N) load_g(gbuf[(i + 1) & 1], wave_block(S::slab(i + 1), wave), S::chunk(i + 1));
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int rr = 0; rr < 4; ++rr)
#pragma unroll
          for (int nb = 0; nb < NB; ++nb)
            acc[4 * c + u][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4_get(gbuf[i & 1][u], rr), y[s][nb][rr],
                                                                      acc[4 * c + u][nb], 0, 0, 0);
    });
  }

  // ---- the four column shares, added in wave order ----------------------------------------------
  for (int w = 0; w < 4; ++w) {
    if (wave == w) {
#pragma unroll
      for (int ib = 0; ib < NBLK; ++ib)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb) {
          float4* p = reinterpret_cast<float4*>(gs + (16 * nb + n16) * GPITCH + 16 * ib + 4 * g);
          float4 v = make_float4(acc[ib][nb][0], acc[ib][nb][1], acc[ib][nb][2], acc[ib][nb][3]);
          if (w > 0) {
            const float4 o = *p;
            v = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
          }
          *p = v;
        }
    }
    __syncthreads();
  }
  // ---- adjoint of the mean subtraction, one row per patch --------------------------------------
  for (int p = wave * (TILE / 4); p < (wave + 1) * (TILE / 4); ++p) {
    const int n = tile_base + p;
    const float4 v = *reinterpret_cast<const float4*>(gs + p * GPITCH + 4 * lane);
    const float mean = wave_sum((v.x + v.y) + (v.z + v.w)) * (1.f / 256.f);
    if constexpr (PN == PN_STD) {
      // lane holds gamma of pixels 4 lane .. 4 lane + 3: row lane / 4, columns 4 (lane % 4) ..
      if (n >= a.n_end) continue;  // (wave-uniform)
      const float m = pmean_s[p];
      float4 out = make_float4(0.f, 0.f, 0.f, 0.f);  // a filtered patch: an exact zero row
      if (m == m) {
        const int py = n / a.nPx, px = n % a.nPx;
        const float* row = a.image + (size_t)wrap(py * a.stride + (lane >> 2) - a.shift_y, a.H) * a.W;
        const float vv[4] = {v.x, v.y, v.z, v.w};
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < 4; ++j)
          dot = fmaf(vv[j], (row[wrap(px * a.stride + 4 * (lane & 3) + j - a.shift_x, a.W)] - m) / m, dot);
        const float c = mean + wave_sum(dot) * (1.f / 256.f);
        out = make_float4((v.x - c) / m, (v.y - c) / m, (v.z - c) / m, (v.w - c) / m);
      }
      *reinterpret_cast<float4*>(a.gpatch + (size_t)n * D256 + 4 * lane) = out;
    } else if (n < a.n_end)
      *reinterpret_cast<float4*>(a.gpatch + (size_t)n * D256 + 4 * lane) =
          make_float4(v.x - mean, v.y - mean, v.z - mean, v.w - mean);
  }
}

// Overlap-add of the gradient rows: pixel (Y, X) of the rolled frame sums the rows of the patches that cover it, patch
// rows ascending, then patch columns (one order: run-to-run identical), and adds the ROUNDED product coef * sum (times
// n'(raw flux) under an image norm) at the un-rolled position.  Nothing for a pixel no patch covers or whose sum is 0.
template <bool NORM>
__global__ __launch_bounds__(256) void gmm256_gather_kernel(GmmGatherArgs a) {
#pragma clang fp contract(off)
  if (a.shift_dev) a.shift_y = a.shift_dev[0], a.shift_x = a.shift_dev[1];
  const int Y = blockIdx.y;
  const int X = blockIdx.x * 256 + threadIdx.x;
  if (X >= a.W || Y >= a.y_end) return;
  int py_hi = Y / a.stride;
  int py_lo = Y - (P16 - 1) < 0 ? 0 : (Y - (P16 - 1) + a.stride - 1) / a.stride;
  if (py_hi > a.nPy - 1) py_hi = a.nPy - 1;
  int px_hi = X / a.stride;
  int px_lo = X - (P16 - 1) < 0 ? 0 : (X - (P16 - 1) + a.stride - 1) / a.stride;
  if (px_hi > a.nPx - 1) px_hi = a.nPx - 1;
  float sum = 0.f;
  bool any = false;
  for (int py = py_lo; py <= py_hi; ++py) {
    const int r = Y - py * a.stride;
    for (int px = px_lo; px <= px_hi; ++px) {
      const int cc = X - px * a.stride;
      sum += a.gpatch[((size_t)py * a.nPx + px) * D256 + r * P16 + cc];
      any = true;
    }
  }
  if (!any || sum == 0.f) return;
  const int yy = wrap(Y - a.shift_y, a.H), xx = wrap(X - a.shift_x, a.W);
  const size_t idx = (size_t)yy * a.W + xx;
  if (NORM) a.grad[idx] += gather_normed_term(a, sum, a.raw_flux[idx]);
  else a.grad[idx] += a.coef * sum;
}

template <typename Tp>
int grow(Tp** ptr, size_t* cap, size_t need) {
  if (need <= *cap) return JD_OK;
  if (*ptr) (void)hipFree(*ptr);
  *ptr = nullptr;
  *cap = 0;
  JD_HIP(hipMalloc(ptr, need * sizeof(Tp)));
  *cap = need;
  return JD_OK;
}

}  // namespace

struct Gmm256 {
  int K = 0;
  int n_cu = 256;
  bool triangular = true;
  float* afrag = nullptr;
  float* gfrag = nullptr;
  float* mfrag = nullptr;
  float* const_k = nullptr;
  // workspaces (grown on demand)
  int32_t* argmax = nullptr;
  size_t argmax_cap = 0;
  float* vpatch = nullptr;
  size_t vpatch_cap = 0;
  float* gpatch = nullptr;
  size_t gpatch_cap = 0;
  double* partials = nullptr;
  size_t partials_cap = 0;
};

void gmm256_destroy(Gmm256* g) {
  if (!g) return;
  for (float* p : {g->afrag, g->gfrag, g->mfrag, g->const_k, g->vpatch, g->gpatch})
    if (p) (void)hipFree(p);
  if (g->argmax) (void)hipFree(g->argmax);
  if (g->partials) (void)hipFree(g->partials);
  delete g;
}

bool gmm256_is_triangular(const Gmm256* g) { return g->triangular; }

int gmm256_set_const_residual(Gmm256* g, const float* residual) {
  JD_HIP(hipDeviceSynchronize());  // (no pass of this handle is reading the constants)
  JD_HIP(hipMemcpy(g->const_k + g->K, residual, (size_t)g->K * sizeof(float), hipMemcpyHostToDevice));
  return JD_OK;
}

int gmm256_create(int K, const float* prec_chol, const float* mu_prec, const float* const_k, const float* pixel_w,
                  Gmm256** out) {
  Gmm256* g = new (std::nothrow) Gmm256();
  if (!g) return fail(JD_ERR_ALLOC, "jd_gmm_create: out of host memory");
  g->K = K;
  const size_t kf = (size_t)K * FRAG_FLOATS;
  auto alloc = [&](float** dst, size_t n) { return hipMalloc(dst, n * sizeof(float)) == hipSuccess; };
  if (!alloc(&g->afrag, kf) || !alloc(&g->gfrag, kf) || !alloc(&g->mfrag, (size_t)K * D256) || !alloc(&g->const_k, 2 * (size_t)K)) {
    gmm256_destroy(g);
    return fail(JD_ERR_ALLOC, "jd_gmm_create: hipMalloc of the D = 256 fragments (%zu MB) failed", 2 * kf * sizeof(float) >> 20);
  }
  // one component at a time through a host buffer (a 200-component mixture is 52 MB per fragment set)
  std::vector<float> prow((size_t)FRAG_FLOATS), af((size_t)FRAG_FLOATS), gf((size_t)FRAG_FLOATS), mrow(D256);
  double sw[D256];
  for (int j = 0; j < D256; ++j) sw[j] = std::sqrt((double)pixel_w[j]);
  bool tri = true;
  for (int k = 0; k < K; ++k) {
    const float* Pk = prec_chol + (size_t)k * FRAG_FLOATS;
    for (int i = 0; i < D256; ++i)
      for (int j = 0; j < D256; ++j) {
        prow[(size_t)i * D256 + j] = (float)((double)Pk[(size_t)i * D256 + j] * sw[j]);  // P'[i][j] = P[i][j] * sqrt(w_j)
        if (i > j && Pk[(size_t)i * D256 + j] != 0.f) tri = false;
      }
    for (int j = 0; j < D256; ++j) mrow[j] = -(float)((double)mu_prec[(size_t)k * D256 + j] * sw[j]);
    // forward A fragments [jb][st4][lane][e]: P'[pixel 16 st4 + 4 e + (lane >> 4)][16 jb + (lane & 15)]
    for (int jb = 0; jb < NBLK; ++jb)
      for (int st4 = 0; st4 < NBLK; ++st4)
        for (int lane = 0; lane < 64; ++lane)
          for (int e = 0; e < 4; ++e) {
            const int pix = 16 * st4 + 4 * e + (lane >> 4), j = 16 * jb + (lane & 15);
            af[(size_t)((jb * NBLK + st4) * 64 + lane) * 4 + e] = prow[(size_t)pix * D256 + j];
          }
    // backward A fragments [ib][jb][lane][r]: P'[16 ib + (lane & 15)][16 jb + 4 (lane >> 4) + r]
    for (int ib = 0; ib < NBLK; ++ib)
      for (int jb = 0; jb < NBLK; ++jb)
        for (int lane = 0; lane < 64; ++lane)
          for (int r = 0; r < 4; ++r) {
            const int pix = 16 * ib + (lane & 15), j = 16 * jb + 4 * (lane >> 4) + r;
            gf[(size_t)((ib * NBLK + jb) * 64 + lane) * 4 + r] = prow[(size_t)pix * D256 + j];
          }
    if (hipMemcpy(g->afrag + (size_t)k * FRAG_FLOATS, af.data(), FRAG_FLOATS * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(g->gfrag + (size_t)k * FRAG_FLOATS, gf.data(), FRAG_FLOATS * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
        hipMemcpy(g->mfrag + (size_t)k * D256, mrow.data(), D256 * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
      gmm256_destroy(g);
      return fail(JD_ERR_HIP, "jd_gmm_create: upload of the D = 256 fragments failed");
    }
  }
  if (hipMemcpy(g->const_k, const_k, (size_t)K * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(g->const_k + K, 0, (size_t)K * sizeof(float)) != hipSuccess) {  // (the residuals: zero until set)
    gmm256_destroy(g);
    return fail(JD_ERR_HIP, "jd_gmm_create: upload of the D = 256 constants failed");
  }
  g->triangular = tri;
  int dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) g->n_cu = prop.multiProcessorCount;
  *out = g;
  return JD_OK;
}

static Args256 base_args(const Gmm256* g) {
  Args256 a{};
  a.afrag = g->afrag, a.gfrag = g->gfrag, a.mfrag = g->mfrag, a.const_k = g->const_k, a.K = g->K;
  return a;
}

// Patches per block: 32 (two 16-patch halves: every fragment of a factor feeds two MFMAs) once that gives every CU a
// block, else 16 -- a block's time is the K components one after the other whatever the grid, so below one 32-patch
// tile per CU the halves are better spent on the CUs that would idle (512^2, K = 200, stride 8: 3969 patches;
// profiles/gmm16/README.md has both timed).
// Factors that are not triangular skip nothing (16 chunks per slab sweep) and always take 16 patches: their 32-patch
// backward instantiation needs more registers than a wave has and would spill.
static int tile_halves(long n, int n_cu, bool tri) { return tri && (n + TILE_MAX - 1) / TILE_MAX >= n_cu ? 2 : 1; }

template <int MODE, int PN = PN_SUBTRACT_MEAN>
static void launch_fwd256(const Args256& a, bool tri, int nb, unsigned tiles, hipStream_t s) {
  if (!tri) gmm256_fwd_kernel<MODE, false, 1, PN><<<tiles, 256, 0, s>>>(a);
  else if (nb == 2) gmm256_fwd_kernel<MODE, true, 2, PN><<<tiles, 256, 0, s>>>(a);
  else gmm256_fwd_kernel<MODE, true, 1, PN><<<tiles, 256, 0, s>>>(a);
}

template <int MODE, int PN = PN_SUBTRACT_MEAN>
static void launch_bwd256(const Args256& a, bool tri, int nb, unsigned tiles, hipStream_t s) {
  if (!tri) gmm256_bwd_kernel<MODE, false, 1, PN><<<tiles, 256, 0, s>>>(a);
  else if (nb == 2) gmm256_bwd_kernel<MODE, true, 2, PN><<<tiles, 256, 0, s>>>(a);
  else gmm256_bwd_kernel<MODE, true, 1, PN><<<tiles, 256, 0, s>>>(a);
}

int gmm256_prior(Gmm256* g, const float* image, const float* raw_flux, const ImageNormArgs& norm, int H, int W, int stride,
                 int shift_y, int shift_x, int marginalize, float value_scale, float* value_out, int accumulate_value,
                 float grad_coef, float* grad_flux_accum, int32_t* argmax_out, const int* shift_dev, hipStream_t s,
                 int patch_norm) {
  const bool std_norm = patch_norm == PN_STD;
  JD_REQUIRE(H >= P16 && W >= P16, "jd_gmm_prior_fwd_bwd: image (%d, %d) smaller than a 16x16 patch (D = 256)", H, W);
  JD_REQUIRE(stride >= 1 && stride <= P16, "jd_gmm_prior_fwd_bwd: stride = %d not in [1, 16] (D = 256)", stride);
  const int nPy = (H - P16) / stride + 1, nPx = (W - P16) / stride + 1;
  JD_REQUIRE((long)nPy * nPx < (1L << 31) - TILE_MAX, "jd_gmm_prior_fwd_bwd: too many patches");
  const int n = nPy * nPx;
  const int nb = tile_halves(n, g->n_cu, g->triangular);
  const unsigned tiles = (unsigned)((n + 16 * nb - 1) / (16 * nb));
  shift_y = roll_residue(shift_y, H), shift_x = roll_residue(shift_x, W);
  int rc;
  if ((rc = grow(&g->partials, &g->partials_cap, (size_t)tiles))) return rc;
  Args256 a = base_args(g);
  a.image = image, a.H = H, a.W = W, a.stride = stride, a.nPx = nPx, a.shift_y = shift_y, a.shift_x = shift_x;
  a.shift_dev = shift_dev, a.n_end = n, a.partials = g->partials;
  if (marginalize) {
    if (grad_flux_accum && (rc = grow(&g->vpatch, &g->vpatch_cap, (size_t)n))) return rc;
    a.vpatch = grad_flux_accum ? g->vpatch : nullptr;
  } else {
    a.argmax = argmax_out;
    if (grad_flux_accum && !argmax_out) {
      if ((rc = grow(&g->argmax, &g->argmax_cap, (size_t)n))) return rc;
      a.argmax = g->argmax;
    }
  }
  {
    ProfScope prof(JD_KERNEL_GMM_FWD, s);
    if (marginalize && std_norm) launch_fwd256<M_LSE, PN_STD>(a, g->triangular, nb, tiles, s);
    else if (marginalize) launch_fwd256<M_LSE>(a, g->triangular, nb, tiles, s);
    else if (std_norm) launch_fwd256<M_MAX, PN_STD>(a, g->triangular, nb, tiles, s);
    else launch_fwd256<M_MAX>(a, g->triangular, nb, tiles, s);
    JD_LAUNCH_CHECK();
    if ((rc = launch_finalize_sum(g->partials, (int)tiles, (double)value_scale, 0.0, value_out, accumulate_value, s))) return rc;
  }
  if (!grad_flux_accum) return JD_OK;

  if ((rc = grow(&g->gpatch, &g->gpatch_cap, (size_t)n * D256))) return rc;
  a.gpatch = g->gpatch;
  {
    ProfScope prof(JD_KERNEL_GMM_BWD, s);
    if (marginalize && std_norm) launch_bwd256<M_LSE, PN_STD>(a, g->triangular, nb, tiles, s);
    else if (marginalize) launch_bwd256<M_LSE>(a, g->triangular, nb, tiles, s);
    else if (std_norm) launch_bwd256<M_MAX, PN_STD>(a, g->triangular, nb, tiles, s);
    else launch_bwd256<M_MAX>(a, g->triangular, nb, tiles, s);
    JD_LAUNCH_CHECK();
  }
  GmmGatherArgs ga{};
  ga.gpatch = g->gpatch, ga.grad = grad_flux_accum, ga.H = H, ga.W = W, ga.stride = stride, ga.nPx = nPx, ga.nPy = nPy;
  ga.shift_y = shift_y, ga.shift_x = shift_x, ga.shift_dev = shift_dev, ga.row_begin = 0, ga.row_end = nPy;
  ga.y_begin = 0, ga.y_end = (nPy - 1) * stride + P16;
  ga.coef = grad_coef, ga.norm = norm, ga.raw_flux = raw_flux;
  {
    ProfScope prof(JD_KERNEL_GMM_GATHER, s);
    dim3 grid((W + 255) / 256, ga.y_end);
    if (norm.kind != NORM_IDENTITY) gmm256_gather_kernel<true><<<grid, 256, 0, s>>>(ga);
    else gmm256_gather_kernel<false><<<grid, 256, 0, s>>>(ga);
    JD_LAUNCH_CHECK();
  }
  return JD_OK;
}

int gmm256_estimate_log_prob(Gmm256* g, const float* x, int n, float* out, hipStream_t s) {
  JD_REQUIRE((long)n < (1L << 31) - TILE_MAX, "jd_gmm_estimate_log_prob: too many rows");
  Args256 a = base_args(g);
  a.image = x, a.n_end = n, a.dense_out = out;
  const int nb = tile_halves(n, g->n_cu, g->triangular);
  launch_fwd256<M_DENSE>(a, g->triangular, nb, (unsigned)((n + 16 * nb - 1) / (16 * nb)), s);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

}  // namespace jd
