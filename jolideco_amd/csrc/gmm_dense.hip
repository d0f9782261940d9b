// GMM patch prior on gfx950 (CDNA4).
//
// Forward: for every overlapping 8x8 patch x (mean subtracted) and every mixture component k
//     y_k = x^T P_k - m_k ,  q_k = sum_j w_j y_kj^2 ,  l_k = c_k - q_k / 2 ,  v = max_k l_k | logsumexp_k l_k
// (jolideco/priors/patches/gmm.py:262-281, priors/patches/core.py:189-246).  Per component this is a
// 64 x 64 matrix applied to every patch: a dense contraction, FLOP-bound on the fp32 roof.  It runs on
// the exact-fp32 matrix cores (v_mfma_f32_16x16x4_f32: bit-for-bit an fmaf chain in pixel order):
//   M = whitened coordinate j (four 16-blocks), N = patch (16 per MFMA), K = pixel (4 per MFMA).
//   * P_k = (L_k^-1)^T is UPPER TRIANGULAR (jolideco/utils/numpy.py:16-34), so y_j only needs pixels
//     i <= j: 16-block jb of the whitened coordinates needs pixel steps 0 .. 4 (jb + 1) - 1.  Skipping
//     the all-zero blocks removes 24 of the 64 MFMAs per (component, 16 patches) and changes no bit of
//     the result (the skipped terms are exact zeros at the END of each fmaf chain).  jd_gmm_create checks
//     the structure; a non-triangular matrix set takes the dense variant of the same kernel;
//   * A operand = P'_k = P_k diag(sqrt w) fragments (pixel weights folded into the columns, fragment
//     order prepared once on the host), streamed from L2, register double-buffered across components;
//   * B operand = mean-subtracted patches, staged once per block in LDS in fragment order;
//   * the accumulators start at -m'_k so the mean shift costs nothing;
//   * C layout puts the patch on the lane (n = lane & 15) and the whitened coordinate in the registers,
//     so sum_j y_j^2 is an in-lane sum + two VALU lane swaps; (Np, K) never leaves the CU.
// One block = 4 waves (one per SIMD) shares TB tiles of 32 patches and splits the K components four
// ways; the partial (max, arg-max) | (max, sum-exp) results are merged through LDS in component order.
// Backward (max mode): the patches are bucketed by arg-max component; one wave takes 32 patches that
// share P'_k and runs y = x^T P' - m' and gamma = -P' y on the matrix cores (same block skipping);
// the overlap-add is done race-free and in a fixed order by a gather pass.
// Patch norm (template parameter PN of the kernels that cut patches out of the image): PATCH_NORM_SUBTRACT_MEAN is the
// x above; PATCH_NORM_STD standardizes, x = (p - mean) / mean (jolideco/utils/norms.py:106-112) -- a correctly rounded
// division in the staging and standardized_row_offset in the row epilogues; everything between is the same code.
#include "gmm_internal.h"

namespace jd {

template <int TB, int MODE, bool TRI, int PN = PATCH_NORM_SUBTRACT_MEAN>
__global__ __launch_bounds__(256, 1) void gmm_fwd_kernel(GmmFwdArgs a) {
  use_device_shift(a);
  if (a.run_flag && *a.run_flag != a.run_gen) return;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xs = lds;                                          // TB * 2048 floats
  float* state = lds + TB * 2048;                           // [4 waves][TB][2][32 patches]
  int* okf = reinterpret_cast<int*>(state + 4 * TB * 64);  // [TB * 32]
  __shared__ double red[4];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int tile_base = a.n_begin + blockIdx.x * (TB * 32);

  // ---- stage the block's patches (mean subtracted) in MFMA B-operand order ------------------
  {
    const int h = lane >> 5, c = lane & 31;  // lane (h, c) gathers pixels 32 h .. 32 h + 31 of patch c
    for (int t = wave; t < TB; t += 4) {
      const int n = tile_base + 32 * t + c;
      const bool valid = n < a.n_end;
      float x[32];
      bool sel = true;
      if (MODE == MODE_DENSE) {
#pragma unroll
        for (int s = 0; s < 32; ++s) x[s] = valid ? a.flux[(size_t)n * D + 32 * h + s] : 0.f;
      } else {
        const int py = valid ? n / a.nPx : 0, px = valid ? n % a.nPx : 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int yy = wrap(py * a.stride + 4 * h + r - a.shift_y, a.H);
          const float* row = a.flux + (size_t)yy * a.W;
#pragma unroll
          for (int cc = 0; cc < 8; ++cc) {
            const int xx = wrap(px * a.stride + cc - a.shift_x, a.W);
            const float v = valid ? row[xx] : 0.f;
            x[8 * r + cc] = v;
            sel = sel && (v > -1e5f);  // patches/core.py:215
          }
        }
        const float mean = patch_mean_halves(x);  // SubtractMeanPatchNorm, utils/norms.py:100-103
#pragma unroll
        for (int s = 0; s < 32; ++s) x[s] = PN == PATCH_NORM_STD ? (x[s] - mean) / mean : x[s] - mean;
        // NOT `sel && shfl(...)`: the short circuit would keep the lanes with sel == false out of the exchange and the
        // other half of the patch would read a stale register
        const int sel_other = __shfl_xor((int)sel, 32, 64);
        sel = sel && sel_other != 0;
      }
#pragma unroll
      for (int s = 0; s < 32; ++s) xs[xs_index(t, c, 32 * h + s)] = x[s];
      if (h == 0) okf[t * 32 + c] = (valid && sel) ? 1 : 0;
    }
  }
  __syncthreads();

  // ---- this wave's share of the components over all TB tiles ------------------------------------
  const int g = lane >> 4, n16 = lane & 15;
  float* st_lane = state + wave * (TB * 64) + n16;
  if (lane < 32) {
#pragma unroll
    for (int t = 0; t < TB; ++t) state[wave * (TB * 64) + t * 64 + lane] = -INFINITY, state[wave * (TB * 64) + t * 64 + 32 + lane] = 0.f;
  }
  const int k0 = (a.K * wave) / 4, k1 = (a.K * (wave + 1)) / 4;
  const float4* af = reinterpret_cast<const float4*>(a.afrag) + lane;
  const float4* mf = reinterpret_cast<const float4*>(a.mfrag) + g;
  const float* xs_lane = xs + (g * 16 + n16) * 4;
  const int n_lane = tile_base + n16;
  if (k0 < k1) {
    FragBuf f0, f1;
    load_frags<TRI>(f0, af, mf, k0);
    for (int k = k0; k < k1; k += 2) {
      // prefetch is unconditional (clamped): a branch would force a full vmcnt(0) drain
      load_frags<TRI>(f1, af, mf, k + 1 < k1 ? k + 1 : k);
      sweep_tiles<TB, MODE, TRI, PN>(f0, xs_lane, st_lane, a.const_k[k], k, a, n_lane, g == 0);
      load_frags<TRI>(f0, af, mf, k + 2 < k1 ? k + 2 : k);
      if (k + 1 < k1) sweep_tiles<TB, MODE, TRI, PN>(f1, xs_lane, st_lane, a.const_k[k + 1], k + 1, a, n_lane, g == 0);
    }
  }
  if (MODE == MODE_DENSE) return;

  // ---- merge the four component ranges per patch (wave order = component order) ---------------
  __syncthreads();
  double local = 0.0;
  for (int p = threadIdx.x; p < TB * 32; p += 256) {
    const int n = tile_base + p;
    float b = -INFINITY, x1 = 0.f;
    int ar = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const float bw = state[w * (TB * 64) + (p >> 5) * 64 + (p & 31)];
      const float sw = state[w * (TB * 64) + (p >> 5) * 64 + 32 + (p & 31)];
      if (MODE == MODE_MAX) {
        if (bw > b) b = bw, ar = __float_as_int(sw);
      } else if (sw > 0.f) {  // online logsumexp merge of (max, sum exp) pairs
        if (bw > b) {
          x1 = x1 * expf(b - bw) + sw;
          b = bw;
        } else {
          x1 += sw * expf(bw - b);
        }
      }
    }
    const float v = MODE == MODE_LSE ? b + logf(x1) : b;
    const bool ok = okf[p] != 0;
    if (n < a.n_end) {
      if (MODE == MODE_MAX && a.argmax_out) a.argmax_out[n] = ok ? ar : -1;
      if (MODE == MODE_MAX && a.best_out) a.best_out[n] = ok ? best_key(b, ar) : 0ull;
      if (a.value_patch) a.value_patch[n] = ok ? v : NAN;
      if (ok) local += (double)v;
    }
  }
  local = wave_sum(local);
  if (lane == 0) red[wave] = local;
  __syncthreads();
  if (threadIdx.x == 0) a.partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// ------------------------------------------------------------------------------------------
// Backward, max mode: per patch  gamma = -P'_k* (xbar^T P'_k* - m'_k*),  gbar = gamma - mean(gamma).
// Every patch uses the matrix of ITS arg-max component, so the patches are first bucketed by
// component (counting sort: LDS histograms + one global atomic per bin and block; the order inside a
// bucket does not influence any result); buckets are padded to 32 slots.  One wave then takes a
// 32-slot group, i.e. 32 patches that share P'_k, and runs both products on the matrix cores:
//   Y^T = P'^T Xbar^T - m'      (as in the forward kernel)
//   G^T = P' Y^T                (the Y accumulators ARE the B operand: lane group g holds
//                                Y[16 jb + 4 g + r] in register r of block jb, and the A fragments of
//                                this product are laid out on the host in exactly that order, so no
//                                lane movement / LDS is needed; blocks jb < ib are zero and skipped)
// ------------------------------------------------------------------------------------------
template <bool TRI, int PN = PATCH_NORM_SUBTRACT_MEAN>
__global__ __launch_bounds__(256) void gmm_bwd_max_kernel(GmmBwdArgs a) {
  use_device_shift(a);
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, n16 = lane & 15;
  const int wave_global = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int n_waves = gridDim.x * 4;
  const int n_groups = a.offsets[a.K] >> 5;
  for (int grp = wave_global; grp < n_groups; grp += n_waves) {
    // slot 0 of a group is always occupied (padding sits at the end of a bucket)
    const int k = __builtin_amdgcn_readfirstlane(a.argmax[__builtin_amdgcn_readfirstlane(a.order[32 * grp])]);
    const int slot_end = __builtin_amdgcn_readfirstlane(a.offsets[k] + a.counts[k]);
    int n[2];
    bool valid[2];
    // ---- B operand: x[nb][st] = pixel 4 st + g of patch 16 nb + n16, mean subtracted ------------
    float x[2][16];
    StdPatch sp[2];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const int slot = 32 * grp + 16 * nb + n16;
      valid[nb] = slot < slot_end;
      n[nb] = valid[nb] ? a.order[slot] : -1;
      const int py = valid[nb] ? n[nb] / a.nPx : 0, px = valid[nb] ? n[nb] % a.nPx : 0;
#pragma unroll
      for (int st = 0; st < 16; ++st) {
        const int p = 4 * st + g;  // pixel index: row p / 8, column p % 8
        const int yy = wrap(py * a.stride + (p >> 3) - a.shift_y, a.H);
        const int xx = wrap(px * a.stride + (p & 7) - a.shift_x, a.W);
        x[nb][st] = valid[nb] ? a.flux[(size_t)yy * a.W + xx] : 0.f;
      }
      const float mean = patch_mean_groups(x[nb]);
#pragma unroll
      for (int st = 0; st < 16; ++st) x[nb][st] = PN == PATCH_NORM_STD ? (x[nb][st] - mean) / mean : x[nb][st] - mean;
      sp[nb] = StdPatch{py, px, mean};
    }

    f32x4 y[4][2];
    whiten_columns<TRI>(y, x, a.afrag, a.mfrag, k, lane);
    float* rows[2] = {a.gpatch + (size_t)(valid[0] ? n[0] - a.n_begin : 0) * D, a.gpatch + (size_t)(valid[1] ? n[1] - a.n_begin : 0) * D};
    if constexpr (PN == PATCH_NORM_STD)
      patch_gradient_rows<TRI, PN>(y, a.gfrag, k, lane, valid, rows, &a, sp);
    else
      patch_gradient_rows<TRI>(y, a.gfrag, k, lane, valid, rows);
  }
}

// ------------------------------------------------------------------------------------------
// Backward, marginalized (logsumexp) mode: d v / d xbar = sum_k r_k gamma_k with the responsibilities
// r_k = exp(l_k - v) (v = logsumexp from the forward pass) and gamma_k = -P'_k y_k.  One wave owns
// GRP groups of 32 patches and walks over ALL components: Y as in the forward kernel, the columns
// of Y scaled by r_k (per patch = per lane), then G += P'_k (r_k Y) accumulated over k in registers.
// Twice the matrix work of the forward pass; fragments are streamed from L2, register double-buffered.
// ------------------------------------------------------------------------------------------
struct GFrag {
  float4 a[4][4];  // [ib][jb]
};

template <bool TRI>
__device__ __forceinline__ void load_gfrags(GFrag& f, const float4* gf, int k) {
  const float4* gk = gf + (size_t)k * (AFRAG_FLOATS / 4);
#pragma unroll
  for (int ib = 0; ib < 4; ++ib)
#pragma unroll
    for (int jb = 0; jb < 4; ++jb)
      if (!TRI || jb >= ib) f.a[ib][jb] = gk[(ib * 4 + jb) * 64];
}

// One component of the logsumexp pass (value AND gradient in one sweep over the components, the way an online softmax
// is accumulated): y = P'^T xbar - m', l = c_k - |y|^2 / 2; the running maximum m of the patch rises to max(m, l), the sum
// S and the gradient accumulator G are rescaled by exp(m_old - m_new) -- a wave-uniform branch, taken only while some
// patch of the wave still sees its maximum rise -- and the component enters with the weight e = exp(l - m):
// S += e, G += P' (e y).  At the end v = m + log S and the gradient row is G / S.
// PN = PATCH_NORM_STD: l takes the residual ck_lo of c_k as well (finish_tile: the same l as the forward kernel's).
template <bool TRI, int GRP, int PN = PATCH_NORM_SUBTRACT_MEAN>
__device__ __forceinline__ void lse_component(const FragBuf& f, const GFrag& gfr, float ck, const float4 (&x)[GRP][8],
                                              float (&m)[GRP][2], float (&S)[GRP][2], f32x4 (&G)[GRP][4][2], float ck_lo = 0.f) {
#pragma unroll
  for (int gi = 0; gi < GRP; ++gi) {
    f32x4 y[4][2];
    mfma_tile<TRI>(y, f, x[gi]);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      float l = fmaf(-0.5f, sum_lane_groups(sum_squares(y, nb)), ck);
      if constexpr (PN == PATCH_NORM_STD) l += ck_lo;
      const bool rises = l > m[gi][nb];
      if (__ballot(rises) != 0ull) {
        const float m_new = rises ? l : m[gi][nb];
        const float scale = rises ? expf(m[gi][nb] - m_new) : 1.f;  // (exp(-inf) = 0 the first time: S and G are 0 anyway)
        m[gi][nb] = m_new;
        S[gi][nb] *= scale;
#pragma unroll
        for (int ib = 0; ib < 4; ++ib)
#pragma unroll
          for (int e = 0; e < 4; ++e) G[gi][ib][nb][e] *= scale;
      }
      const float w = expf(l - m[gi][nb]);  // (a NaN l -- a non-finite pixel -- never rises and poisons S: NaN out)
      S[gi][nb] += w;
#pragma unroll
      for (int jb = 0; jb < 4; ++jb)
#pragma unroll
        for (int e = 0; e < 4; ++e) y[jb][nb][e] *= w;
    }
#pragma unroll
    for (int ib = 0; ib < 4; ++ib)
#pragma unroll
      for (int jb = TRI ? ib : 0; jb < 4; ++jb)
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
          for (int nb = 0; nb < 2; ++nb)
            G[gi][ib][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4_get(gfr.a[ib][jb], e), y[jb][nb][e], G[gi][ib][nb], 0, 0, 0);
  }
}

// Logsumexp value and gradient rows of all patches in ONE pass over the components (dense path of marginalize = True
// with a gradient, and the gated fallback of the screened one): per patch v = logsumexp_k l_k -> one fp64 partial sum
// per block, gamma = -sum_k r_k P'_k y_k minus its mean -> gpatch.  (Until late in round 3 a forward kernel computed v
// first and this kernel evaluated every l_k a second time to form r_k = exp(l_k - v): three matrix products per
// component instead of two.)
template <bool TRI, int GRP, int PN = PATCH_NORM_SUBTRACT_MEAN>
__global__ __launch_bounds__(256, 1) void gmm_bwd_lse_kernel(GmmBwdLseArgs a) {
  use_device_shift(a);
  const bool everything = !a.mark || *a.run_flag == a.run_gen;
  __shared__ double red[4];
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, n16 = lane & 15;
  const int wave_global = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int n_waves = gridDim.x * 4;
  const int n_groups = (a.n_end - a.n_begin + 31) / 32;
  const float4* af = reinterpret_cast<const float4*>(a.afrag) + lane;
  const float4* mf = reinterpret_cast<const float4*>(a.mfrag) + g;
  const float4* gf = reinterpret_cast<const float4*>(a.gfrag) + lane;
  double local = 0.0;
  const int n_listed = everything ? 0 : *a.list_count;
  const int n_steps = everything ? n_groups : (n_listed + 31) / 32;
  for (int grp0 = wave_global * GRP; grp0 < n_steps; grp0 += n_waves * GRP) {
    int n[GRP][2];
    bool valid[GRP][2], sel[GRP][2], mine[GRP][2];
    float m[GRP][2], S[GRP][2];
    float pmean[GRP][2];  // (PATCH_NORM_STD: the patch means, for the row epilogue)
    float4 x[GRP][8];
    f32x4 G[GRP][4][2];
#pragma unroll
    for (int gi = 0; gi < GRP; ++gi)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const int idx = (grp0 + gi) * 32 + nb * 16 + n16;
        if (everything) {
          n[gi][nb] = a.n_begin + idx;
          valid[gi][nb] = n[gi][nb] < a.n_end;
        } else {
          valid[gi][nb] = idx < n_listed;
          n[gi][nb] = valid[gi][nb] ? a.list[idx] : a.n_begin;
        }
        mine[gi][nb] = valid[gi][nb];
      }
#pragma unroll
    for (int gi = 0; gi < GRP; ++gi)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        m[gi][nb] = -INFINITY, S[gi][nb] = 0.f;
        const int py = valid[gi][nb] ? n[gi][nb] / a.nPx : 0, px = valid[gi][nb] ? n[gi][nb] % a.nPx : 0;
        float xv[16];
        int keep = 1;
#pragma unroll
        for (int st = 0; st < 16; ++st) {
          const int p = 4 * st + g;
          const int yy = wrap(py * a.stride + (p >> 3) - a.shift_y, a.H);
          const int xx = wrap(px * a.stride + (p & 7) - a.shift_x, a.W);
          xv[st] = valid[gi][nb] ? a.flux[(size_t)yy * a.W + xx] : 0.f;
          keep &= xv[st] > -1e5f ? 1 : 0;  // patches/core.py:215
        }
        keep &= __shfl_xor(keep, 16, 64);  // the four lane groups hold 16 pixels of the patch each
        keep &= __shfl_xor(keep, 32, 64);
        sel[gi][nb] = valid[gi][nb] && keep != 0;
        const float mean = patch_mean_groups(xv);
        pmean[gi][nb] = mean;
        if (PN == PATCH_NORM_STD) {
#pragma unroll
          for (int st = 0; st < 16; ++st) xv[st] = (xv[st] - mean) / mean;
        } else {
#pragma unroll
          for (int st = 0; st < 16; ++st) xv[st] -= mean;
        }
#pragma unroll
        for (int st4 = 0; st4 < 4; ++st4) x[gi][nb * 4 + st4] = make_float4(xv[4 * st4], xv[4 * st4 + 1], xv[4 * st4 + 2], xv[4 * st4 + 3]);
#pragma unroll
        for (int ib = 0; ib < 4; ++ib) G[gi][ib][nb] = f32x4{0.f, 0.f, 0.f, 0.f};
      }

    FragBuf f0, f1;
    GFrag g0, g1;
    load_frags<TRI>(f0, af, mf, 0);
    load_gfrags<TRI>(g0, gf, 0);
    for (int k = 0; k < a.K; k += 2) {
      const int kn = k + 1 < a.K ? k + 1 : k;
      load_frags<TRI>(f1, af, mf, kn);
      load_gfrags<TRI>(g1, gf, kn);
      if constexpr (PN == PATCH_NORM_STD)
        lse_component<TRI, GRP, PN>(f0, g0, a.const_k[k], x, m, S, G, a.const_k[a.K + k]);
      else
        lse_component<TRI, GRP>(f0, g0, a.const_k[k], x, m, S, G);
      const int kn2 = k + 2 < a.K ? k + 2 : k;
      load_frags<TRI>(f0, af, mf, kn2);
      load_gfrags<TRI>(g0, gf, kn2);
      if constexpr (PN == PATCH_NORM_STD) {
        if (k + 1 < a.K) lse_component<TRI, GRP, PN>(f1, g1, a.const_k[k + 1], x, m, S, G, a.const_k[a.K + k + 1]);
      } else {
        if (k + 1 < a.K) lse_component<TRI, GRP>(f1, g1, a.const_k[k + 1], x, m, S, G);
      }
    }

    // v = m + log S; gamma = -G / S, minus its mean over the 64 pixels (adjoint of the patch-mean subtraction); a
    // filtered patch has no value and no gradient
#pragma unroll
    for (int gi = 0; gi < GRP; ++gi)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        const float inv = sel[gi][nb] ? 1.f / S[gi][nb] : 0.f;
        float sum = 0.f;
#pragma unroll
        for (int ib = 0; ib < 4; ++ib) {
          G[gi][ib][nb] *= inv;
          sum += (G[gi][ib][nb][0] + G[gi][ib][nb][1]) + (G[gi][ib][nb][2] + G[gi][ib][nb][3]);
        }
        const float mean = sum_lane_groups(sum) * (1.f / 64.f);
        float c = mean, inv_m = 1.f;  // PATCH_NORM_STD: the row is (c - G) / m (a filtered patch: an exact zero row)
        if constexpr (PN == PATCH_NORM_STD) {
          const float pm = pmean[gi][nb];
          const int py = valid[gi][nb] ? n[gi][nb] / a.nPx : 0, px = valid[gi][nb] ? n[gi][nb] % a.nPx : 0;
          c = standardized_row_offset(a, py, px, g, pm, mean, [&](int ib, int e) { return G[gi][ib][nb][e]; });
          inv_m = 1.f / pm;
        }
        if (mine[gi][nb]) {
          float4* out = reinterpret_cast<float4*>(a.gpatch + (size_t)(n[gi][nb] - a.n_begin) * D);
          if constexpr (PN == PATCH_NORM_STD) {
#pragma unroll
            for (int ib = 0; ib < 4; ++ib)
              out[4 * ib + g] = sel[gi][nb] ? make_float4((c - G[gi][ib][nb][0]) * inv_m, (c - G[gi][ib][nb][1]) * inv_m,
                                                          (c - G[gi][ib][nb][2]) * inv_m, (c - G[gi][ib][nb][3]) * inv_m)
                                            : make_float4(0.f, 0.f, 0.f, 0.f);
          } else {
#pragma unroll
            for (int ib = 0; ib < 4; ++ib)
              out[4 * ib + g] = make_float4(mean - G[gi][ib][nb][0], mean - G[gi][ib][nb][1], mean - G[gi][ib][nb][2],
                                            mean - G[gi][ib][nb][3]);
          }
          const float v = sel[gi][nb] ? m[gi][nb] + logf(S[gi][nb]) : 0.f;
          if (g == 0 && a.vpatch) a.vpatch[n[gi][nb]] = v;
          if (g == 0 && sel[gi][nb]) local += (double)v;
        }
      }
  }
  if (a.vpatch) return;  // (the values are summed by gmm_lse_value_kernel)
  local = wave_sum(local);
  if (lane == 0) red[threadIdx.x >> 6] = local;
  __syncthreads();
  if (threadIdx.x == 0) a.partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// Tiles per block: the choice that minimises (rounds over the CUs) x (tiles per block); ties go to
// the larger block (fewer fragment re-reads).
static int pick_block_tiles(long n_patches, int n_cu) {
  {  // tuning override
    const int t = opt_value(OPT_GMM_BLOCK_TILES, 0);
    if (t == 4 || t == 8 || t == 16) return t;
  }
  const long nt = (n_patches + 31) / 32;
  int best_tb = 16;
  long best_cost = -1;
  for (int tb : {16, 8, 4}) {
    const long blocks = (nt + tb - 1) / tb;
    const long cost = ((blocks + n_cu - 1) / n_cu) * tb;
    if (best_cost < 0 || cost < best_cost) best_cost = cost, best_tb = tb;
  }
  return best_tb;
}

template <int TB, int MODE, bool TRI, int PN>
static int launch_fwd_tb(const GmmFwdArgs& a, unsigned blocks, hipStream_t s) {
  const size_t lds = (size_t)(TB * 2048 + 4 * TB * 64 + TB * 32) * sizeof(float);
  static bool configured = false;
  if (!configured) {
    JD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&gmm_fwd_kernel<TB, MODE, TRI, PN>),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    configured = true;
  }
  gmm_fwd_kernel<TB, MODE, TRI, PN><<<blocks, 256, lds, s>>>(a);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

// tiles per block -> instantiation
template <int MODE, bool TRI, int PN>
static int launch_fwd_tiles(int tb, const GmmFwdArgs& a, unsigned blocks, hipStream_t s) {
  switch (tb) {
    case 16: return launch_fwd_tb<16, MODE, TRI, PN>(a, blocks, s);
    case 8: return launch_fwd_tb<8, MODE, TRI, PN>(a, blocks, s);
    default: return launch_fwd_tb<4, MODE, TRI, PN>(a, blocks, s);
  }
}
template <int MODE, int PN = PATCH_NORM_SUBTRACT_MEAN>
static int launch_fwd_mode(bool tri, int tb, const GmmFwdArgs& a, unsigned blocks, hipStream_t s) {
  return tri ? launch_fwd_tiles<MODE, true, PN>(tb, a, blocks, s) : launch_fwd_tiles<MODE, false, PN>(tb, a, blocks, s);
}

int launch_fwd_blocks(int mode, const GmmFwdArgs& a, bool tri, int n_cu, hipStream_t s, int* n_partials, int patch_norm) {
  const long n = a.n_end - a.n_begin;
  const int tb = pick_block_tiles(n, n_cu);
  const unsigned blocks = (unsigned)((n + 32L * tb - 1) / (32L * tb));
  *n_partials = (int)blocks;
  if (patch_norm == PATCH_NORM_STD && mode != MODE_DENSE)
    return mode == MODE_MAX ? launch_fwd_mode<MODE_MAX, PATCH_NORM_STD>(tri, tb, a, blocks, s)
                            : launch_fwd_mode<MODE_LSE, PATCH_NORM_STD>(tri, tb, a, blocks, s);
  switch (mode) {
    case MODE_MAX: return launch_fwd_mode<MODE_MAX>(tri, tb, a, blocks, s);
    case MODE_LSE: return launch_fwd_mode<MODE_LSE>(tri, tb, a, blocks, s);
    default: return launch_fwd_mode<MODE_DENSE>(tri, tb, a, blocks, s);
  }
}

int launch_fwd(int mode, const GmmFwdArgs& a, bool tri, int n_cu, hipStream_t s, int* n_partials, int patch_norm) {
  if (opt_is_set(OPT_GMM_DENSE)) tri = false;  // tuning / testing: force the dense variant
  ProfScope prof(JD_KERNEL_GMM_FWD, s);
  return launch_fwd_blocks(mode, a, tri, n_cu, s, n_partials, patch_norm);
}

void launch_bwd_max(const GmmBwdArgs& b, bool tri, unsigned blocks, hipStream_t s, int patch_norm) {
  if (patch_norm == PATCH_NORM_STD) {
    if (tri)
      gmm_bwd_max_kernel<true, PATCH_NORM_STD><<<blocks, 256, 0, s>>>(b);
    else
      gmm_bwd_max_kernel<false, PATCH_NORM_STD><<<blocks, 256, 0, s>>>(b);
  } else if (tri)
    gmm_bwd_max_kernel<true><<<blocks, 256, 0, s>>>(b);
  else
    gmm_bwd_max_kernel<false><<<blocks, 256, 0, s>>>(b);
}

void launch_bwd_lse(const GmmBwdLseArgs& b, bool tri, unsigned blocks, hipStream_t s, int patch_norm) {
  if (patch_norm == PATCH_NORM_STD) {
    if (tri)
      gmm_bwd_lse_kernel<true, 2, PATCH_NORM_STD><<<blocks, 256, 0, s>>>(b);
    else
      // one group per wave: with two, the factors that skip nothing and the means of this norm do not fit the registers
      // (the kernel strides over the groups whatever the grid was sized for)
      gmm_bwd_lse_kernel<false, 1, PATCH_NORM_STD><<<blocks, 256, 0, s>>>(b);
  } else if (tri)
    gmm_bwd_lse_kernel<true, 2><<<blocks, 256, 0, s>>>(b);
  else
    gmm_bwd_lse_kernel<false, 2><<<blocks, 256, 0, s>>>(b);
}

}  // namespace jd

using namespace jd;

extern "C" int jd_gmm_estimate_log_prob(jd_gmm* g, const float* x, int n, float* out, void* stream) {
  JD_REQUIRE(g && x && out && n > 0, "jd_gmm_estimate_log_prob: null argument or n <= 0");
  hipStream_t s = as_stream(stream);
  if (g->d256) return gmm256_estimate_log_prob(g->d256, x, n, out, s);
  int rc;
  if ((rc = g->dense.partials.reserve((size_t)((n + 31) / 32 + 4)))) return rc;
  GmmFwdArgs a{};
  a.flux = x, a.afrag = g->dense.afrag.ptr, a.mfrag = g->dense.mfrag.ptr, a.const_k = g->dense.const_k.ptr;
  a.K = g->K, a.n_begin = 0, a.n_end = n, a.value_patch = out, a.partials = g->dense.partials.ptr;
  int n_waves = 0;
  return launch_fwd(MODE_DENSE, a, g->triangular, g->n_cu, s, &n_waves);
}
