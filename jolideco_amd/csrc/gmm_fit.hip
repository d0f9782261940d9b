// EM for a full-covariance Gaussian mixture of image patches on gfx950 (CDNA4): the device half of one EM step.
//
// For patches x_n (n, D) and the current parameters (mu_k, upper triangular precision factors P_k, constants
// c_k = log w_k + log det P_k - D/2 log 2 pi) one launch produces, per component k,
//     S0_k = sum_n r_nk ,   S1_k = sum_n r_nk d_nk ,   S2_k = sum_n r_nk d_nk d_nk^T ,   d_nk = x_n - mu_k
// and L = sum_n lse_n, with l_nk = c_k - |P_k^T d_nk|^2 / 2, lse_n = logsumexp_k l_nk, r_nk = exp(l_nk - lse_n).  The
// moments are taken about the CURRENT mean, so the host's float64 finish (jolideco_amd/priors/patches/gmm.py `fit`)
// corrects the mean by the small S1_k / S0_k instead of subtracting two large sums.
//
// One block (4 waves) owns a contiguous range of patches and walks it in chunks of at most FIT_CHUNK patches:
//   phase 1  for every component, for every 64-patch tile of the chunk: the tile is staged in LDS already centred
//            (x - mu_k), every wave whitens 16 of its patches on v_mfma_f32_16x16x4_f32 (M = whitened coordinate,
//            N = patch, K = feature; the all-zero 16x16 blocks of the triangular P_k are skipped) and the owner lane
//            of a patch updates its running (max, sum exp) in LDS: a max-shifted, online logsumexp;
//   phase 2  the same sweep once more; now r_nk = exp(l_nk - lse_n) (a component hundreds below the maximum gives an
//            exact 0) goes to LDS, and wave w accumulates rows 16 (4 panel + w) .. + 15 of S2_k on the matrix cores
//            (M = feature i, N = feature j, K = patch: A = r d_i, B = d_j, both read from the staged tile), S1_k and S0_k
//            beside them on the VALU, in float64 as well.  D = 256 takes four panels of 64 rows; the responsibilities
//            of the chunk are kept in LDS from the first panel.
// S2 IS ACCUMULATED IN FLOAT64, on v_mfma_f64_16x16x4_f64 with the exact products r d_i and the float32 d_j widened.  On
// v_mfma_f32_16x16x4_f32 every fmaf of the chain rounds, and what that leaves in a covariance is noise of about 1e-7 of
// its largest entry in EVERY direction -- also in those where the patches vary little or, for mean-free patches, not at
// all and only the ridge reg_covar keeps the matrix positive definite.  Measured with float32 accumulators (over 2048 and
// over 256 patches): the covariances of 8x8 patches of a Gamma(20) image, variance 20, under the default ridge 1e-6 had
// negative eigenvalues after the first step, and on unit-variance patches the lower bound wandered by 2e-3 from step to
// step, more than the default tolerance of the fit.  With float64 sums S2 is a sum of exact positive semi-definite terms.
// The f64 MFMA runs at half the rate of the f32 one; the whitening, which is a likelihood and not a difference of large
// numbers, stays on the f32 form.
// At the end of a chunk every thread adds its share to the block's OWN float64 partial sums in device memory (the same
// thread owns the same address for the whole launch: no atomics, a fixed order).  A second launch adds the blocks'
// partials in block order in float64.  Two runs on the same input give the same bits.  The workspace is the partials
// (blocks x K x (D^2 + D + 1) doubles, blocks <= the CU count and <= FIT_WORKSPACE_BYTES); nothing of size n is held.
// x is read with 4-byte loads only: any float-aligned pointer is accepted and changes no bit.
#include <memory>

#include "gmm_internal.h"

namespace jd {

using f64x4 = __attribute__((ext_vector_type(4))) double;

// Patches of a chunk: the running logsumexp state and the responsibilities of a component live in LDS for that many; a
// multiple of the 64-patch tile.
constexpr int FIT_CHUNK = 2048;
constexpr int FIT_TILE = 64;
constexpr int FIT_BLOCK_MIN = 256;  // patches a block takes at least: below that more blocks only add partial sums
constexpr size_t FIT_WORKSPACE_BYTES = size_t(8) << 30;

struct GmmFitArgs {
  const float* x;      // (n, D)
  const float* mu;     // (K, D)
  const float* prec;   // (K, D, D) upper triangular P_k, row major
  const float* const_k;  // K
  double* partials;    // [block][k][D * D second | D first | 1 zeroth]
  double* lse_partials;  // [block]
  long long n;
  long long per_block;  // patches per block, multiple of FIT_TILE
  int K;
};

// LDS row pitch of the staged tile: + 16 floats puts the four patches of a Gram step on disjoint banks
template <int DD>
constexpr int fit_pitch() { return DD + 16; }

// the tile [n0, n0 + 64) of patches, centred on mu_k, zero rows past n_hi; thread t serves feature t % DD throughout
template <int DD>
__device__ __forceinline__ void fit_stage(float* xs, const float* x, long long n0, long long n_hi, float mu_f) {
  constexpr int LD = fit_pitch<DD>();
  const int f = threadIdx.x % DD;
#pragma unroll 4
  for (int i = threadIdx.x; i < FIT_TILE * DD; i += 256) {
    const int p = i / DD;
    const long long n = n0 + p;
    xs[p * LD + f] = n < n_hi ? gld(x + (size_t)n * DD + f) - mu_f : 0.f;
  }
}

// One 16 x 16 block of the factor against 16 features of 16 patches: MFMA step e contracts over the features
// 16 q + 4 g + e, g = lane group, so the B operand of the four steps is one 16-byte LDS read.
template <int DD>
__device__ __forceinline__ void fit_whiten_block(f32x4& acc0, f32x4& acc1, const float* xrow, const float* pcol, int q) {
  const float4 xv = *reinterpret_cast<const float4*>(xrow + 16 * q);
  const float* pr = pcol + (size_t)(16 * q) * DD;
  const float a0 = gld(pr), a1 = gld(pr + DD), a2 = gld(pr + 2 * DD), a3 = gld(pr + 3 * DD);
  acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a0, xv.x, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a1, xv.y, acc1, 0, 0, 0);
  acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(a2, xv.z, acc0, 0, 0, 0);
  acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(a3, xv.w, acc1, 0, 0, 0);
}

// v(lane) + v(lane ^ 16) + v(lane ^ 32) + v(lane ^ 48) in a fixed order, on every lane
__device__ __forceinline__ double fit_sum_lane_groups(double v) {
  v += __shfl_xor(v, 16, 64);
  return v + __shfl_xor(v, 32, 64);
}

__device__ __forceinline__ float fit_add_squares(float qsum, const f32x4& y) {
  return fmaf(y[3], y[3], fmaf(y[2], y[2], fmaf(y[1], y[1], fmaf(y[0], y[0], qsum))));
}

// |P_k^T d|^2 of patch 16 wave + (lane & 15) of the staged tile, on every lane of its column.  Whitened coordinates
// 16 jb .. 16 jb + 15 need the features below 16 (jb + 1) only: the other blocks of an upper triangular P_k are zero.
// Two accumulator chains per coordinate block: the dependent latency of the MFMA exceeds its issue interval.
// D = 64: the ten blocks are unrolled and their factor loads are in flight together; D = 256 has 136, taken two at a time.
template <int DD>
__device__ __forceinline__ float fit_whiten(const float* xs, const float* pk, int wave, int lane) {
  constexpr int LD = fit_pitch<DD>(), NJ = DD / 16;
  const int g = lane >> 4, n16 = lane & 15;
  const float* xrow = xs + (16 * wave + n16) * LD + 4 * g;
  const float* pcol = pk + (size_t)(4 * g) * DD + n16;
  float qsum = 0.f;
  if constexpr (NJ <= 4) {
#pragma unroll
    for (int jb = 0; jb < NJ; ++jb) {
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q <= jb; ++q) fit_whiten_block<DD>(acc0, acc1, xrow, pcol + 16 * jb, q);
      qsum = fit_add_squares(qsum, acc0 + acc1);
    }
  } else {
    for (int jb = 0; jb < NJ; ++jb) {
      f32x4 acc0 = {0.f, 0.f, 0.f, 0.f}, acc1 = {0.f, 0.f, 0.f, 0.f};
      int q = 0;
      for (; q + 1 <= jb; q += 2) {
        fit_whiten_block<DD>(acc0, acc1, xrow, pcol + 16 * jb, q);
        fit_whiten_block<DD>(acc0, acc1, xrow, pcol + 16 * jb, q + 1);
      }
      if (q <= jb) fit_whiten_block<DD>(acc0, acc1, xrow, pcol + 16 * jb, q);
      qsum = fit_add_squares(qsum, acc0 + acc1);
    }
  }
  return sum_lane_groups(qsum);
}

template <int DD>
__global__ __launch_bounds__(256) void gmm_fit_kernel(GmmFitArgs a) {
  constexpr int LD = fit_pitch<DD>(), NJ = DD / 16, PANELS = DD / 64, STRIDE = DD * DD + DD + 1;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xs = lds;                      // FIT_TILE * LD
  float* mrun = xs + FIT_TILE * LD;     // FIT_CHUNK: running maximum (phase 1) | responsibilities of the component (phase 2)
  float* srun = mrun + FIT_CHUNK;       // FIT_CHUNK: running sum exp, then lse
  __shared__ double red[4];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, n16 = lane & 15;
  const long long b_lo = (long long)blockIdx.x * a.per_block;
  const long long b_hi = b_lo + a.per_block < a.n ? b_lo + a.per_block : a.n;
  double* part = a.partials + (size_t)blockIdx.x * a.K * STRIDE;
  double lse_local = 0.0;

  for (long long c0 = b_lo; c0 < b_hi; c0 += FIT_CHUNK) {
    const long long c1 = c0 + FIT_CHUNK < b_hi ? c0 + FIT_CHUNK : b_hi;
    const int n_tiles = (int)((c1 - c0 + FIT_TILE - 1) / FIT_TILE);
    const bool first = c0 == b_lo;
    for (int i = threadIdx.x; i < FIT_CHUNK; i += 256) mrun[i] = -INFINITY, srun[i] = 0.f;

    // ---- phase 1: lse_n over all components ------------------------------------------------------------------
    for (int k = 0; k < a.K; ++k) {
      const float mu_f = gld(a.mu + (size_t)k * DD + threadIdx.x % DD);
      const float ck = gld(a.const_k + k);
      const float* pk = a.prec + (size_t)k * DD * DD;
      for (int t = 0; t < n_tiles; ++t) {
        __syncthreads();  // (the previous tile's readers are done; the first time: the initialisation above has landed)
        fit_stage<DD>(xs, a.x, c0 + (long long)t * FIT_TILE, c1, mu_f);
        __syncthreads();
        const float l = fmaf(-0.5f, fit_whiten<DD>(xs, pk, wave, lane), ck);
        if (g == 0) {  // the owner lane of the patch: the same one for every component
          const int i = t * FIT_TILE + 16 * wave + n16;
          const float m = mrun[i], s = srun[i];
          const bool rises = l > m;
          const float e = expf(rises ? m - l : l - m);  // (exp(-inf) = 0 the first time)
          mrun[i] = rises ? l : m;
          srun[i] = rises ? fmaf(s, e, 1.f) : s + e;
        }
      }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < FIT_CHUNK; i += 256) {
      const float v = mrun[i] + logf(srun[i]);
      srun[i] = v;
      if (c0 + i < c1) lse_local += (double)v;
    }

    // ---- phase 2: responsibilities and the weighted moments about mu_k ---------------------------------------
    for (int k = 0; k < a.K; ++k) {
      const float mu_f = gld(a.mu + (size_t)k * DD + threadIdx.x % DD);
      const float ck = gld(a.const_k + k);
      const float* pk = a.prec + (size_t)k * DD * DD;
      double* dst = part + (size_t)k * STRIDE;
      for (int panel = 0; panel < PANELS; ++panel) {
        const int ib = 4 * panel + wave;
        f64x4 acc[NJ];
#pragma unroll
        for (int jb = 0; jb < NJ; ++jb) acc[jb] = f64x4{0.0, 0.0, 0.0, 0.0};
        double s0 = 0.0, s1 = 0.0;
        for (int t = 0; t < n_tiles; ++t) {
          __syncthreads();
          fit_stage<DD>(xs, a.x, c0 + (long long)t * FIT_TILE, c1, mu_f);
          __syncthreads();
          if (panel == 0) {
            const float l = fmaf(-0.5f, fit_whiten<DD>(xs, pk, wave, lane), ck);
            const int i = t * FIT_TILE + 16 * wave + n16;
            if (g == 0) mrun[i] = c0 + i < c1 ? expf(l - srun[i]) : 0.f;
            __syncthreads();
          }
          const float* rt = mrun + t * FIT_TILE + g;
          const float* xg = xs + g * LD + n16;
#pragma unroll 4
          for (int s = 0; s < FIT_TILE / 4; ++s) {  // patches 4 s + g of the tile
            const float rr = rt[4 * s];
            const float* row = xg + 4 * s * LD;
            const float di = row[16 * ib];
            const double av = (double)rr * (double)di;  // exact
            s0 += (double)rr, s1 += av;
#pragma unroll
            for (int jb = 0; jb < NJ; ++jb) acc[jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, (double)row[16 * jb], acc[jb], 0, 0, 0);
          }
        }
        // ---- the chunk's sums of (k, panel) join the block's partials: lane (g, j) holds S2[16 ib + g + 4 r][16 jb + j] (the
        // C layout of the f64 MFMA: its rows are interleaved over the registers, unlike the f32 form's)
#pragma unroll
        for (int jb = 0; jb < NJ; ++jb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double* p = dst + (size_t)(16 * ib + g + 4 * r) * DD + 16 * jb + n16;
            *p = first ? acc[jb][r] : *p + acc[jb][r];
          }
        const double t1 = fit_sum_lane_groups(s1), t0 = fit_sum_lane_groups(s0);
        if (g == 0) {
          double* p = dst + DD * DD + 16 * ib + n16;
          *p = first ? t1 : *p + t1;
        }
        if (panel == 0 && threadIdx.x == 0) {
          double* p = dst + DD * DD + DD;
          *p = first ? t0 : *p + t0;
        }
      }
    }
    __syncthreads();  // (the next chunk re-initialises the running state)
  }

  lse_local = wave_sum(lse_local);
  if (lane == 0) red[wave] = lse_local;
  __syncthreads();
  if (threadIdx.x == 0) a.lse_partials[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}

// The moments of HARD assignments, r_nk = [labels[n] == k] (the k-means start of the fit): phase 2 of the kernel above with
// the labels of the chunk in LDS in place of the responsibilities and no whitening.  A tile that holds no patch of the
// component is skipped (a block-uniform vote), so a component costs its own patches' tiles and not all of them.  A label is
// only ever COMPARED with k: one outside [0, K) matches no component and contributes nothing.  The lse slot is 0.
template <int DD>
__global__ __launch_bounds__(256) void gmm_fit_labels_kernel(GmmFitArgs a, const int* labels) {
  constexpr int LD = fit_pitch<DD>(), NJ = DD / 16, PANELS = DD / 64, STRIDE = DD * DD + DD + 1;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xs = lds;                                            // FIT_TILE * LD
  int* labs = reinterpret_cast<int*>(xs + FIT_TILE * LD);     // FIT_CHUNK

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, n16 = lane & 15;
  const long long b_lo = (long long)blockIdx.x * a.per_block;
  const long long b_hi = b_lo + a.per_block < a.n ? b_lo + a.per_block : a.n;
  double* part = a.partials + (size_t)blockIdx.x * a.K * STRIDE;

  for (long long c0 = b_lo; c0 < b_hi; c0 += FIT_CHUNK) {
    const long long c1 = c0 + FIT_CHUNK < b_hi ? c0 + FIT_CHUNK : b_hi;
    const int n_tiles = (int)((c1 - c0 + FIT_TILE - 1) / FIT_TILE);
    const bool first = c0 == b_lo;
    __syncthreads();  // (the previous chunk's readers are done)
    for (int i = threadIdx.x; i < FIT_CHUNK; i += 256) labs[i] = c0 + i < c1 ? labels[c0 + i] : -1;
    __syncthreads();

    for (int k = 0; k < a.K; ++k) {
      const float mu_f = gld(a.mu + (size_t)k * DD + threadIdx.x % DD);
      double* dst = part + (size_t)k * STRIDE;
      for (int panel = 0; panel < PANELS; ++panel) {
        const int ib = 4 * panel + wave;
        f64x4 acc[NJ];
#pragma unroll
        for (int jb = 0; jb < NJ; ++jb) acc[jb] = f64x4{0.0, 0.0, 0.0, 0.0};
        double s0 = 0.0, s1 = 0.0;
        bool present = false;
        for (int t = 0; t < n_tiles; ++t) {
          // (a barrier as well: the previous tile's readers are done)
          if (!__syncthreads_or(threadIdx.x < FIT_TILE && labs[t * FIT_TILE + threadIdx.x] == k)) continue;
          present = true;
          fit_stage<DD>(xs, a.x, c0 + (long long)t * FIT_TILE, c1, mu_f);
          __syncthreads();
          const int* lt = labs + t * FIT_TILE + g;
          const float* xg = xs + g * LD + n16;
#pragma unroll 4
          for (int s = 0; s < FIT_TILE / 4; ++s) {  // patches 4 s + g of the tile
            const bool hit = lt[4 * s] == k;
            const float* row = xg + 4 * s * LD;
            const double av = hit ? (double)row[16 * ib] : 0.0;  // (selected, not multiplied: a patch that is not the
            s0 += hit ? 1.0 : 0.0, s1 += av;                      //  component's may hold anything, NaN included)
#pragma unroll
            for (int jb = 0; jb < NJ; ++jb)
              acc[jb] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, hit ? (double)row[16 * jb] : 0.0, acc[jb], 0, 0, 0);
          }
        }
        if (!first && !present) continue;  // (block-uniform: nothing to add)
#pragma unroll
        for (int jb = 0; jb < NJ; ++jb)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            double* p = dst + (size_t)(16 * ib + g + 4 * r) * DD + 16 * jb + n16;
            *p = first ? acc[jb][r] : *p + acc[jb][r];
          }
        const double t1 = fit_sum_lane_groups(s1), t0 = fit_sum_lane_groups(s0);
        if (g == 0) {
          double* p = dst + DD * DD + 16 * ib + n16;
          *p = first ? t1 : *p + t1;
        }
        if (panel == 0 && threadIdx.x == 0) {
          double* p = dst + DD * DD + DD;
          *p = first ? t0 : *p + t0;
        }
      }
    }
  }
  if (threadIdx.x == 0) a.lse_partials[blockIdx.x] = 0.0;
}

// out = [S0 (K) | S1 (K, D) | S2 (K, D, D) | L]: the blocks' partials added in block order in float64
__global__ __launch_bounds__(256) void gmm_fit_reduce_kernel(const double* partials, const double* lse_partials, int blocks, int K,
                                                             int DD, double* out) {
  const size_t stride = (size_t)DD * DD + DD + 1, total = (size_t)K * stride;
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e < total) {
    const size_t k = e / stride, j = e % stride;
    double sum = 0.0;
    for (int b = 0; b < blocks; ++b) sum += partials[(size_t)b * total + e];
    const size_t d2 = (size_t)DD * DD;
    const size_t at = j < d2 ? (size_t)K * (1 + DD) + k * d2 + j : j < d2 + DD ? (size_t)K + k * DD + (j - d2) : k;
    out[at] = sum;
  }
  if (e == 0) {
    double sum = 0.0;
    for (int b = 0; b < blocks; ++b) sum += lse_partials[b];
    out[total] = sum;
  }
}

template <int DD>
static int launch_fit(const GmmFitArgs& a, unsigned blocks, hipStream_t s) {
  const size_t lds = (size_t)(FIT_TILE * fit_pitch<DD>() + 2 * FIT_CHUNK) * sizeof(float);
  static bool configured = false;
  if (!configured) {
    JD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&gmm_fit_kernel<DD>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    configured = true;
  }
  gmm_fit_kernel<DD><<<blocks, 256, lds, s>>>(a);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

}  // namespace jd

using namespace jd;

struct jd_gmm_fit {
  int D = 0, K = 0;
  int max_blocks = 1;  // partial-sum sets the workspace may hold
  DevBuf<double> partials, lse_partials;
};

extern "C" int jd_gmm_fit_create(int D, int K, int max_blocks, jd_gmm_fit** fit_out) {
  JD_REQUIRE(fit_out, "jd_gmm_fit_create: null argument");
  *fit_out = nullptr;
  JD_REQUIRE(D == 64 || D == 256, "jd_gmm_fit_create: D = 64 or D = 256 only, got D = %d", D);
  JD_REQUIRE(K >= 1 && K <= 1024, "jd_gmm_fit_create: 1 <= K <= 1024, got K = %d", K);
  JD_REQUIRE(max_blocks >= 0, "jd_gmm_fit_create: max_blocks = %d is negative (0 selects the default)", max_blocks);
  std::unique_ptr<jd_gmm_fit> f(new jd_gmm_fit());
  f->D = D, f->K = K;
  int n_cu = 256, dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n_cu = prop.multiProcessorCount;
  const size_t set_bytes = (size_t)K * ((size_t)D * D + D + 1) * sizeof(double);
  const size_t fit = FIT_WORKSPACE_BYTES / set_bytes;
  f->max_blocks = (int)std::max<size_t>(1, std::min<size_t>((size_t)n_cu, fit));
  if (max_blocks > 0) f->max_blocks = std::min(f->max_blocks, max_blocks);
  *fit_out = f.release();
  return JD_OK;
}

extern "C" int jd_gmm_fit_destroy(jd_gmm_fit* fit) {
  delete fit;
  return JD_OK;
}

namespace jd {
template <int DD>
static int launch_fit_labels(const GmmFitArgs& a, const int* labels, unsigned blocks, hipStream_t s) {
  const size_t lds = (size_t)(FIT_TILE * fit_pitch<DD>() + FIT_CHUNK) * sizeof(float);
  static bool configured[64] = {};  // (per device: the attribute belongs to the device's copy of the kernel)
  int dev = 0;
  JD_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= 64 || !configured[dev]) {
    JD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&gmm_fit_labels_kernel<DD>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
    if (dev >= 0 && dev < 64) configured[dev] = true;
  }
  gmm_fit_labels_kernel<DD><<<blocks, 256, lds, s>>>(a, labels);
  JD_LAUNCH_CHECK();
  return JD_OK;
}
}  // namespace jd

// What the soft and the hard step share, so that the two cannot drift apart: the split of the patches into blocks with
// the partial sums it needs (their layout is a contract between the step kernels and the reduce kernel), and the reduction.
static int fit_split(jd_gmm_fit* fit, long long n, GmmFitArgs& a, unsigned& blocks_out) {
  const long long want = (n + FIT_BLOCK_MIN - 1) / FIT_BLOCK_MIN;
  long long blocks = std::min<long long>(want, fit->max_blocks);
  const long long per_block = ((n + blocks - 1) / blocks + FIT_TILE - 1) / FIT_TILE * FIT_TILE;
  blocks = (n + per_block - 1) / per_block;
  const size_t stride = (size_t)fit->D * fit->D + fit->D + 1;
  int rc;
  if ((rc = fit->partials.reserve((size_t)blocks * fit->K * stride))) return rc;
  if ((rc = fit->lse_partials.reserve((size_t)blocks))) return rc;
  a.partials = fit->partials.ptr, a.lse_partials = fit->lse_partials.ptr;
  a.n = n, a.per_block = per_block, a.K = fit->K;
  blocks_out = (unsigned)blocks;
  return JD_OK;
}

static int fit_reduce(jd_gmm_fit* fit, unsigned blocks, double* sums_out, hipStream_t s) {
  const size_t total = (size_t)fit->K * ((size_t)fit->D * fit->D + fit->D + 1);
  gmm_fit_reduce_kernel<<<(unsigned)((total + 255) / 256), 256, 0, s>>>(fit->partials.ptr, fit->lse_partials.ptr, (int)blocks, fit->K,
                                                                         fit->D, sums_out);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

extern "C" int jd_gmm_fit_step(jd_gmm_fit* fit, const float* x, long long n, const float* means, const float* prec_chol,
                               const float* const_k, double* sums_out, void* stream) {
  JD_REQUIRE(fit, "jd_gmm_fit_step: null handle");
  JD_REQUIRE(x && means && prec_chol && const_k && sums_out, "jd_gmm_fit_step: null argument");
  JD_REQUIRE(n >= 1 && n <= 2147483647LL / fit->D, "jd_gmm_fit_step: 1 <= n <= (2^31 - 1) / D, got n = %lld with D = %d", n, fit->D);
  JD_REQUIRE((reinterpret_cast<uintptr_t>(x) & 3) == 0, "jd_gmm_fit_step: x is not aligned to a float");
  hipStream_t s = as_stream(stream);
  GmmFitArgs a{};
  unsigned blocks = 0;
  int rc;
  if ((rc = fit_split(fit, n, a, blocks))) return rc;
  a.x = x, a.mu = means, a.prec = prec_chol, a.const_k = const_k;
  if ((rc = fit->D == 64 ? launch_fit<64>(a, blocks, s) : launch_fit<256>(a, blocks, s))) return rc;
  return fit_reduce(fit, blocks, sums_out, s);
}

extern "C" int jd_gmm_fit_step_labels(jd_gmm_fit* fit, const float* x, long long n, const float* means, const int* labels,
                                      double* sums_out, void* stream) {
  JD_REQUIRE(fit, "jd_gmm_fit_step_labels: null handle");
  JD_REQUIRE(x && means && labels && sums_out, "jd_gmm_fit_step_labels: null argument");
  JD_REQUIRE(n >= 1 && n <= 2147483647LL / fit->D, "jd_gmm_fit_step_labels: 1 <= n <= (2^31 - 1) / D, got n = %lld with D = %d", n,
             fit->D);
  JD_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(labels)) & 3) == 0,
             "jd_gmm_fit_step_labels: x or labels is not aligned to 4 bytes");
  hipStream_t s = as_stream(stream);
  GmmFitArgs a{};
  unsigned blocks = 0;
  int rc;
  if ((rc = fit_split(fit, n, a, blocks))) return rc;
  a.x = x, a.mu = means;
  if ((rc = fit->D == 64 ? launch_fit_labels<64>(a, labels, blocks, s) : launch_fit_labels<256>(a, labels, blocks, s))) return rc;
  return fit_reduce(fit, blocks, sums_out, s);
}
