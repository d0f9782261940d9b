// k-means (Lloyd) on image patches for gfx950 (CDNA4): the device half of one Lloyd step, the start of the mixture fit
// (jolideco_amd/priors/patches/kmeans.py; csrc/gmm_fit.hip takes over from the clusters).
//
// For patches x_n (n, D) and centres c_k (K, D) one call produces
//     labels[n] = argmin_k s_nk ,  s_nk = |c_k|^2 - 2 x_n . c_k    (lowest k on a tie; -1 where a score is not finite)
//     count_k = #{n : labels[n] = k} ,  sum_k = sum_{labels[n] = k} x_n  (float64) ,
//     inertia = sum_n max(|x_n|^2 + s_n,label, 0) ,  changed = #{n : labels[n] differs from its value on entry} ,  unassigned.
// Two kernels share one split of the patches into blocks (4 waves each, contiguous ranges, multiples of the tile):
//   assign  a tile of 64 NT patches is staged once in LDS (4-byte loads: any float-aligned x), every wave keeps the MFMA B
//           fragments of its 16 NT patches in registers and walks the centres in tiles of 16: v_mfma_f32_16x16x4_f32 with
//           M = centre, N = patch, K = feature; the A operand is one 16-byte load per four MFMAs straight from the centres
//           (K D floats: they stay in L2).  Lane (g, j) sees the scores of patch j against centres 16 kt + 4 g + r in
//           ascending k, keeps its minimum with a strict <, and the four lane groups are merged with the lower k winning
//           a tie.  The inertia is NOT taken from the float32 score: |x|^2 + |c|^2 - 2 x.c of the winner is summed again in
//           float64 from the staged tile, one wave reduction per patch.
//   sums    blockIdx.y selects KG centre tiles; the tile is staged again, its labels come from the first kernel, and
//           sum_k is the product onehot(K x patches) . x on v_mfma_f64_16x16x4_f64 (M = centre, N = feature, K = patch; A
//           is exactly 0 or 1 and B the float32 value widened: every product is exact).  Wave w owns the features
//           [D/4 w, D/4 (w + 1)); the accumulators live in registers for the block's whole range and are stored once.
//           A label outside [0, K) matches no centre: labels are compared, never used as an index.
// No atomics: every address of a block's partial sums has one owner thread, and a third launch adds the blocks' partials
// in block order in float64.  Two calls on the same input give the same bits.
#include <memory>

#include "gmm_internal.h"

namespace jd {

using f64x4 = __attribute__((ext_vector_type(4))) double;

constexpr int KM_K_MAX = 1024;
constexpr int KM_DEVICES_MAX = 64;  // devices whose kernel attributes are remembered (beyond: set at every call)
constexpr int KM_BLOCK_MIN = 512;  // patches a block takes at least
constexpr size_t KM_WORKSPACE_BYTES = size_t(2) << 30;

template <int DD>
struct KmCfg {
  static constexpr int NT = DD == 64 ? 2 : 1;   // 16-patch MFMA tiles per wave in the assignment
  static constexpr int TILE = 64 * NT;          // patches staged at once
  static constexpr int LD = DD + 4;             // LDS row pitch: the 16-byte fragment reads of 16 rows cover all banks
  static constexpr int FT = DD / 64;            // 16-feature tiles per wave in the sums
  static constexpr int KG = DD == 64 ? 8 : 4;   // centre tiles per block of the sums: KG FT accumulators of 4 doubles
  static constexpr size_t LDS_BYTES = (size_t)(TILE * LD + KM_K_MAX + TILE) * sizeof(float);
};

struct KmeansArgs {
  const float* x;    // (n, D)
  const float* c;    // (K, D)
  int* labels;       // n
  double* partials;  // [block][count (K) | sum x (K, D) | inertia | changed | unassigned]
  long long n;
  long long per_block;  // patches per block, multiple of the tile
  int K;
};

// the tile [n0, n0 + TILE) of patches, zero rows past n_hi
template <int DD>
__device__ __forceinline__ void km_stage(float* xs, const float* x, long long n0, long long n_hi) {
  constexpr int LD = KmCfg<DD>::LD, TILE = KmCfg<DD>::TILE;
  const int f = threadIdx.x % DD;
#pragma unroll 4
  for (int i = threadIdx.x; i < TILE * DD; i += 256) {
    const int p = i / DD;
    const long long n = n0 + p;
    xs[p * LD + f] = n < n_hi ? gld(x + (size_t)n * DD + f) : 0.f;
  }
}

template <int DD>
__global__ __launch_bounds__(256) void kmeans_assign_kernel(KmeansArgs a) {
  using C = KmCfg<DD>;
  constexpr int NT = C::NT, TILE = C::TILE, LD = C::LD, NQ = DD / 16;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xs = lds;                                      // TILE * LD
  float* cn = xs + TILE * LD;                           // KM_K_MAX: |c_k|^2
  int* labs = reinterpret_cast<int*>(cn + KM_K_MAX);    // TILE
  __shared__ double red[3][4];

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, n16 = lane & 15;
  const int K = a.K, KT = (K + 15) / 16;
  const long long b_lo = (long long)blockIdx.x * a.per_block;
  const long long b_hi = b_lo + a.per_block < a.n ? b_lo + a.per_block : a.n;

  for (int k = threadIdx.x; k < K; k += 256) {  // (float64 sum, rounded once)
    double s = 0.0;
    for (int f = 0; f < DD; ++f) {
      const double v = (double)gld(a.c + (size_t)k * DD + f);
      s += v * v;
    }
    cn[k] = (float)s;
  }

  double inertia = 0.0;
  int changed = 0, unassigned = 0;
  for (long long t0 = b_lo; t0 < b_hi; t0 += TILE) {
    __syncthreads();  // (the previous tile's readers are done; the first time: cn has landed)
    km_stage<DD>(xs, a.x, t0, b_hi);
    __syncthreads();

    // ---- B fragments: features 16 q + 4 g + e of patch 16 (NT wave + j) + n16
    float4 xf[NT][NQ];
#pragma unroll
    for (int j = 0; j < NT; ++j)
#pragma unroll
      for (int q = 0; q < NQ; ++q)
        xf[j][q] = *reinterpret_cast<const float4*>(xs + (16 * (NT * wave + j) + n16) * LD + 4 * g + 16 * q);
    float best[NT];
    int best_k[NT];
    bool bad[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) best[j] = INFINITY, best_k[j] = -1, bad[j] = false;

    for (int kt = 0; kt < KT; ++kt) {
      const bool row_ok = 16 * kt + n16 < K;  // (a centre tile past K: zero rows, scores not looked at)
      const float* crow = a.c + (size_t)(row_ok ? 16 * kt + n16 : 0) * DD + 4 * g;
      f32x4 acc[NT][2];
#pragma unroll
      for (int j = 0; j < NT; ++j) acc[j][0] = acc[j][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        float4 av = gld4u(crow + 16 * q);
        if (!row_ok) av = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
        for (int j = 0; j < NT; ++j) {
          acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.x, xf[j][q].x, acc[j][0], 0, 0, 0);
          acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.y, xf[j][q].y, acc[j][1], 0, 0, 0);
          acc[j][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.z, xf[j][q].z, acc[j][0], 0, 0, 0);
          acc[j][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(av.w, xf[j][q].w, acc[j][1], 0, 0, 0);
        }
      }
      // lane (g, n16) holds x . c of patch n16 and centres 16 kt + 4 g + r
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = 16 * kt + 4 * g + r;
        if (k < K) {
          const float ck = cn[k];
#pragma unroll
          for (int j = 0; j < NT; ++j) {
            const float s = fmaf(-2.f, acc[j][0][r] + acc[j][1][r], ck);
            if (!(fabsf(s) < INFINITY)) bad[j] = true;
            else if (s < best[j]) best[j] = s, best_k[j] = k;
          }
        }
      }
    }
    // ---- the four lane groups of a patch: the smaller score, on a tie the lower k
#pragma unroll
    for (int j = 0; j < NT; ++j) {
#pragma unroll
      for (int off = 16; off <= 32; off <<= 1) {
        const float os = __shfl_xor(best[j], off, 64);
        const int ok = __shfl_xor(best_k[j], off, 64);
        const int ob = __shfl_xor((int)bad[j], off, 64);
        if (ok >= 0 && (best_k[j] < 0 || os < best[j] || (os == best[j] && ok < best_k[j]))) best[j] = os, best_k[j] = ok;
        bad[j] = bad[j] || ob != 0;
      }
      if (g == 0) {
        const int p = 16 * (NT * wave + j) + n16;
        const long long n = t0 + p;
        int label = -1;
        if (n < b_hi) {
          label = bad[j] ? -1 : best_k[j];
          const int old = a.labels[n];
          a.labels[n] = label;
          changed += old != label;
          unassigned += label < 0;
        }
        labs[p] = label;
      }
    }
    __syncthreads();

    // ---- inertia of the wave's patches in float64: sum_f x^2 + c (c - 2 x) = |x|^2 + s with the winner's s
    for (int pp = 0; pp < 16 * NT; ++pp) {
      const int p = 16 * NT * wave + pp;
      const int label = labs[p];  // (wave uniform; in [0, K) or -1)
      if (label < 0) continue;
      double v = 0.0;
#pragma unroll
      for (int f = lane; f < DD; f += 64) {
        const double xv = (double)xs[p * LD + f], cv = (double)gld(a.c + (size_t)label * DD + f);
        v += xv * xv + cv * (cv - 2.0 * xv);
      }
      v = wave_sum(v);
      if (lane == 0) inertia += v > 0.0 ? v : 0.0;
    }
  }

  const double s_in = wave_sum(inertia), s_ch = wave_sum((double)changed), s_un = wave_sum((double)unassigned);
  if (lane == 0) red[0][wave] = s_in, red[1][wave] = s_ch, red[2][wave] = s_un;
  __syncthreads();
  if (threadIdx.x < 3) {
    const size_t stride = (size_t)K * (DD + 1) + 3;
    const double* r = red[threadIdx.x];
    a.partials[(size_t)blockIdx.x * stride + (size_t)K * (DD + 1) + threadIdx.x] = (r[0] + r[1]) + (r[2] + r[3]);
  }
}

// count_k and sum_k of the centre tiles [KG blockIdx.y, KG (blockIdx.y + 1)) over the block's patches
template <int DD>
__global__ __launch_bounds__(256) void kmeans_sums_kernel(KmeansArgs a) {
  using C = KmCfg<DD>;
  constexpr int TILE = C::TILE, LD = C::LD, FT = C::FT, KG = C::KG;
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* xs = lds;
  int* labs = reinterpret_cast<int*>(xs + TILE * LD + KM_K_MAX);

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int g = lane >> 4, n16 = lane & 15;
  const int K = a.K, KT = (K + 15) / 16, kt0 = KG * blockIdx.y;
  const long long b_lo = (long long)blockIdx.x * a.per_block;
  const long long b_hi = b_lo + a.per_block < a.n ? b_lo + a.per_block : a.n;

  f64x4 acc[KG][FT];
  int cnt[KG];
#pragma unroll
  for (int i = 0; i < KG; ++i) {
    cnt[i] = 0;
#pragma unroll
    for (int jf = 0; jf < FT; ++jf) acc[i][jf] = f64x4{0.0, 0.0, 0.0, 0.0};
  }

  for (long long t0 = b_lo; t0 < b_hi; t0 += TILE) {
    __syncthreads();
    km_stage<DD>(xs, a.x, t0, b_hi);
    if (threadIdx.x < TILE) labs[threadIdx.x] = t0 + threadIdx.x < b_hi ? a.labels[t0 + threadIdx.x] : -1;
    __syncthreads();
#pragma unroll 2
    for (int s = 0; s < TILE / 4; ++s) {  // patches 4 s + g of the tile
      const int label = labs[4 * s + g];
      const float* row = xs + (4 * s + g) * LD + 16 * FT * wave + n16;
      double b[FT];
#pragma unroll
      for (int jf = 0; jf < FT; ++jf) b[jf] = label < 0 ? 0.0 : (double)row[16 * jf];  // (0 x NaN: an unassigned patch is in no sum)
#pragma unroll
      for (int i = 0; i < KG; ++i) {
        if (kt0 + i < KT) {
          const bool hit = label == 16 * (kt0 + i) + n16;
          cnt[i] += hit;
          const double av = hit ? 1.0 : 0.0;
#pragma unroll
          for (int jf = 0; jf < FT; ++jf) acc[i][jf] = __builtin_amdgcn_mfma_f64_16x16x4f64(av, b[jf], acc[i][jf], 0, 0, 0);
        }
      }
    }
  }

  // lane (g, j) holds sum[16 kt + g + 4 r][16 ft + j] (the C layout of the f64 MFMA)
  double* part = a.partials + (size_t)blockIdx.x * ((size_t)K * (DD + 1) + 3);
#pragma unroll
  for (int i = 0; i < KG; ++i) {
    const int kt = kt0 + i;
    if (kt >= KT) continue;
#pragma unroll
    for (int jf = 0; jf < FT; ++jf)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k = 16 * kt + g + 4 * r;
        if (k < K) part[(size_t)K + (size_t)k * DD + 16 * (FT * wave + jf) + n16] = acc[i][jf][r];
      }
    int c = cnt[i];
    c += __shfl_xor(c, 16, 64);
    c += __shfl_xor(c, 32, 64);
    if (wave == 0 && g == 0 && 16 * kt + n16 < K) part[16 * kt + n16] = (double)c;
  }
}

// out = [count (K) | sum x (K, D) | inertia | changed | unassigned]: the blocks' partials added in block order
__global__ __launch_bounds__(256) void kmeans_reduce_kernel(const double* partials, int blocks, size_t stride, double* out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= stride) return;
  double sum = 0.0;
  for (int b = 0; b < blocks; ++b) sum += partials[(size_t)b * stride + e];
  out[e] = sum;
}

template <int DD>
static int launch_kmeans(const KmeansArgs& a, unsigned blocks, hipStream_t s) {
  using C = KmCfg<DD>;
  static bool configured[KM_DEVICES_MAX] = {};  // (per device: the attribute belongs to the device's copy of the kernel)
  int dev = 0;
  JD_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= KM_DEVICES_MAX || !configured[dev]) {
    JD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&kmeans_assign_kernel<DD>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)C::LDS_BYTES));
    JD_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(&kmeans_sums_kernel<DD>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)C::LDS_BYTES));
    if (dev >= 0 && dev < KM_DEVICES_MAX) configured[dev] = true;
  }
  kmeans_assign_kernel<DD><<<blocks, 256, C::LDS_BYTES, s>>>(a);
  JD_LAUNCH_CHECK();
  const unsigned groups = (unsigned)(((a.K + 15) / 16 + C::KG - 1) / C::KG);
  kmeans_sums_kernel<DD><<<dim3(blocks, groups), 256, C::LDS_BYTES, s>>>(a);
  JD_LAUNCH_CHECK();
  return JD_OK;
}

}  // namespace jd

using namespace jd;

struct jd_kmeans {
  int D = 0, K = 0;
  int max_blocks = 1;  // partial-sum sets the workspace may hold
  DevBuf<double> partials;
};

extern "C" int jd_kmeans_create(int D, int K, int max_blocks, jd_kmeans** kmeans_out) {
  JD_REQUIRE(kmeans_out, "jd_kmeans_create: null argument");
  *kmeans_out = nullptr;
  JD_REQUIRE(D == 64 || D == 256, "jd_kmeans_create: D = 64 or D = 256 only, got D = %d", D);
  JD_REQUIRE(K >= 1 && K <= KM_K_MAX, "jd_kmeans_create: 1 <= K <= 1024, got K = %d", K);
  JD_REQUIRE(max_blocks >= 0, "jd_kmeans_create: max_blocks = %d is negative (0 selects the default)", max_blocks);
  std::unique_ptr<jd_kmeans> h(new jd_kmeans());
  h->D = D, h->K = K;
  int n_cu = 256, dev = 0;
  hipDeviceProp_t prop;
  if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess) n_cu = prop.multiProcessorCount;
  const size_t set_bytes = ((size_t)K * (D + 1) + 3) * sizeof(double);
  h->max_blocks = (int)std::max<size_t>(1, std::min<size_t>((size_t)2 * n_cu, KM_WORKSPACE_BYTES / set_bytes));
  if (max_blocks > 0) h->max_blocks = std::min(h->max_blocks, max_blocks);
  *kmeans_out = h.release();
  return JD_OK;
}

extern "C" int jd_kmeans_destroy(jd_kmeans* kmeans) {
  delete kmeans;
  return JD_OK;
}

extern "C" int jd_kmeans_step(jd_kmeans* kmeans, const float* x, long long n, const float* centres, int* labels, double* sums_out,
                              void* stream) {
  JD_REQUIRE(kmeans, "jd_kmeans_step: null handle");
  JD_REQUIRE(x && centres && labels && sums_out, "jd_kmeans_step: null argument");
  const int D = kmeans->D, K = kmeans->K;
  JD_REQUIRE(n >= 1 && n <= 2147483647LL / D, "jd_kmeans_step: 1 <= n <= (2^31 - 1) / D, got n = %lld with D = %d", n, D);
  JD_REQUIRE(((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(centres) | reinterpret_cast<uintptr_t>(labels)) & 3) == 0,
             "jd_kmeans_step: x, centres or labels is not aligned to 4 bytes");
  JD_REQUIRE((reinterpret_cast<uintptr_t>(sums_out) & 7) == 0, "jd_kmeans_step: sums_out is not aligned to a double");
  hipStream_t s = as_stream(stream);
  const int tile = D == 64 ? KmCfg<64>::TILE : KmCfg<256>::TILE;
  const long long want = (n + KM_BLOCK_MIN - 1) / KM_BLOCK_MIN;
  long long blocks = std::min<long long>(want, kmeans->max_blocks);
  const long long per_block = ((n + blocks - 1) / blocks + tile - 1) / tile * tile;
  blocks = (n + per_block - 1) / per_block;
  const size_t stride = (size_t)K * (D + 1) + 3;
  int rc;
  if ((rc = kmeans->partials.reserve((size_t)blocks * stride))) return rc;
  KmeansArgs a{};
  a.x = x, a.c = centres, a.labels = labels, a.partials = kmeans->partials.ptr;
  a.n = n, a.per_block = per_block, a.K = K;
  if ((rc = D == 64 ? launch_kmeans<64>(a, (unsigned)blocks, s) : launch_kmeans<256>(a, (unsigned)blocks, s))) return rc;
  kmeans_reduce_kernel<<<(unsigned)((stride + 255) / 256), 256, 0, s>>>(kmeans->partials.ptr, (int)blocks, stride, sums_out);
  JD_LAUNCH_CHECK();
  return JD_OK;
}
