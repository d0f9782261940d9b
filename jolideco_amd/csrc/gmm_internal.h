// What the units of the 8x8 GMM patch prior share (gmm.hip, gmm_dense.hip, gmm_sort.hip, gmm_screen.hip, gmm_gather.hip):
// constants, the device helpers inlined into more than one unit's kernels, every kernel's argument block, the handle, and
// the launch functions one unit calls in another.  The method: gmm_dense.hip (dense kernels), gmm_screen.hip (screen).
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>
#include <vector>

#include "jd_common.h"
#include "kernels.h"
#include "jd_adam.h"
#include "gmm_image_norm.h"
#include "gmm256.h"

namespace jd {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int P = 8;   // patch edge
constexpr int D = 64;  // features per patch
// per component: A fragments [jb 4][st4 4][lane 64][e 4] (P'[pixel 16 st4 + 4 e + (lane >> 4)][16 jb + (lane & 15)])
constexpr int AFRAG_FLOATS = 4 * 4 * 64 * 4;

enum { MODE_MAX = 0, MODE_LSE = 1, MODE_DENSE = 2 };
// patch norm of a pass (jd_gmm_set_patch_norm): x = p - mean(p) | x = (p - mean(p)) / mean(p); a compile-time parameter
// of the dense kernels, which fuse it
enum { PATCH_NORM_SUBTRACT_MEAN = 0, PATCH_NORM_STD = 1, PATCH_NORM_COUNT = 2 };

__host__ __device__ inline unsigned long long best_key(float l, int k) {
  unsigned u = 0;
#if defined(__HIP_DEVICE_COMPILE__)
  u = __float_as_uint(l);
#else
  memcpy(&u, &l, 4);
#endif
  u = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // monotonic map float -> uint
  return ((unsigned long long)u << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)k);
}
__device__ inline float best_value(unsigned long long key) {
  unsigned u = (unsigned)(key >> 32);
  u = (u & 0x80000000u) ? (u & 0x7FFFFFFFu) : ~u;
  return __uint_as_float(u);
}
__device__ inline int best_component(unsigned long long key) { return (int)(0xFFFFFFFFu - (unsigned)(key & 0xFFFFFFFFu)); }

struct GmmFwdArgs {
  const float* flux;     // (H, W) image  | MODE_DENSE: (n, 64) explicit patches
  const float* afrag;    // K * AFRAG_FLOATS
  const float* mfrag;    // K * 64: [jb 4][g 4][r 4] = -m'[16 jb + 4 g + r]
  const float* const_k;  // K constants c_k, then K residuals (jd_gmm_set_const_residual; read under PATCH_NORM_STD only)
  int K, H, W, stride, nPx, shift_y, shift_x;
  const int* shift_dev;  // nullable, device [2] = {shift_y, shift_x} residues: read instead of the two members above (use_device_shift)
  int n_begin, n_end;    // linear patch index range (row-major over the patch grid)
  int32_t* argmax_out;   // nullable (MODE_MAX)
  float* value_patch;    // nullable: per patch v | MODE_DENSE: (n, K) out
  double* partials;      // one per block
  const int* run_flag;   // nullable: the kernel returns at once unless *run_flag == run_gen (fallback of the
  int run_gen;           //           screened path, see GmmScreenArgs::flag)
  unsigned long long* best_out;  // nullable (MODE_MAX): per patch (max, arg-max) key, 0 for a filtered patch
};

// v mod n for -n <= v < 2 n: the host normalises the cycle-spin shifts to [0, n), so every coordinate
// (pixel inside the image) - shift is in (-n, n); an integer division here costs ~20 instructions per pixel and
// made the gather the bottleneck of the bucketed kernels.
// The cycle-spin shift of a pass from DEVICE memory (captured hipGraphs replay with the shifts of the step they run for:
// the host uploads them, the launch arguments never change): overwrites the by-value members of the kernel's own copy
// of its arguments.
template <class A>
__device__ __forceinline__ void use_device_shift(A& a) {
  if (a.shift_dev) a.shift_y = a.shift_dev[0], a.shift_x = a.shift_dev[1];
}

__device__ __forceinline__ int wrap(int v, int n) {
  v = v < 0 ? v + n : v;
  return v >= n ? v - n : v;
}

__device__ __forceinline__ float f4_get(const float4& v, int e) { return e == 0 ? v.x : e == 1 ? v.y : e == 2 ? v.z : v.w; }

// v(lane) + v(lane ^ 16) + v(lane ^ 32) + v(lane ^ 48) on every lane with the gfx950 row / half swaps
// (VALU only; no LDS round trip like ds_bpermute)
__device__ __forceinline__ float sum_lane_groups(float v) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  const float s = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(s), __float_as_uint(s), false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}

// Patch mean with ONE summation order shared by the forward staging and the backward kernels:
//   S_g = (sum of pixels 4 st + g, st = 0..7 in order) + (the same for st = 8..15),  g = 0..3
//   mean = ((S_0 + S_1) + (S_2 + S_3)) / 64
// y = xbar^T P' is sensitive to the mean at the 1e-4 level (the columns of P' do not sum to zero), so
// the backward kernels must subtract the same bits or the recomputed log-likelihoods (and with them
// the logsumexp responsibilities) would not match the forward pass.
// Backward form: lane group g holds x[st] = pixel 4 st + g of its patch.
__device__ __forceinline__ float patch_mean_groups(const float (&x)[16]) {
  float lo = x[0], hi = x[8];
#pragma unroll
  for (int st = 1; st < 8; ++st) lo += x[st], hi += x[8 + st];
  return sum_lane_groups(lo + hi) * (1.f / 64.f);
}
// Forward staging form: lane half h holds x[s] = pixel 32 h + s, i.e. steps st = 8 h .. 8 h + 7 of every g.
__device__ __forceinline__ float patch_mean_halves(const float (&x)[32]) {
  float t[4];
#pragma unroll
  for (int g = 0; g < 4; ++g) {
    float sg = x[g];
#pragma unroll
    for (int k = 1; k < 8; ++k) sg += x[4 * k + g];
    t[g] = sg + __shfl_xor(sg, 32, 64);
  }
  return ((t[0] + t[1]) + (t[2] + t[3])) * (1.f / 64.f);
}

// Backward of the standardized patch norm x = (p - m) / m, m = mean(p): with gamma = dv/dx the row is
//   dv/dp_j = (gamma_j - mean(gamma) - (gamma . x) / 64) / m .
// The row epilogues hold G = -gamma with pixel 16 ib + 4 g + e in register e of block ib (G(ib, e)); x is recomputed
// there from the image and the mean m of the staging (the same bits), so the component loops carry nothing for it.
// Returns mean(G) + (G . x) / 64 given mean(G): the row is (that - G_j) / m.
template <class A, class F>
__device__ __forceinline__ float standardized_row_offset(const A& a, int py, int px, int g, float m, float mean_g, F&& G) {
  float dot = 0.f;
#pragma unroll
  for (int ib = 0; ib < 4; ++ib) {
    const int yy = wrap(py * a.stride + 2 * ib + (g >> 1) - a.shift_y, a.H);
    const float* row = a.flux + (size_t)yy * a.W;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int xx = wrap(px * a.stride + 4 * (g & 1) + e - a.shift_x, a.W);
      dot = fmaf(G(ib, e), (row[xx] - m) / m, dot);
    }
  }
  return mean_g + sum_lane_groups(dot) * (1.f / 64.f);
}

// Fragments of one component held by a lane: A[jb][st4] covers pixel steps 4 st4 .. 4 st4 + 3 of
// coordinate block jb (only st4 <= jb is non-zero for a triangular P), M[jb] the accumulator init.
struct FragBuf {
  float4 a[4][4];
  float4 m[4];
};

template <bool TRI>
__device__ __forceinline__ void load_frags(FragBuf& f, const float4* af, const float4* mf, int k) {
  const float4* ak = af + (size_t)k * (AFRAG_FLOATS / 4);
  const float4* mk = mf + (size_t)k * 16;
#pragma unroll
  for (int jb = 0; jb < 4; ++jb) {
#pragma unroll
    for (int st4 = 0; st4 < 4; ++st4)
      if (!TRI || st4 <= jb) f.a[jb][st4] = ak[(jb * 4 + st4) * 64];
    f.m[jb] = mk[jb * 4];
  }
}

// x[nb * 4 + st4]: B fragments of tile t (two 16-patch halves nb) for pixel steps 4 st4 .. 4 st4 + 3
__device__ __forceinline__ void load_x(float4 (&x)[8], const float* xs_lane, int t) {
#pragma unroll
  for (int q = 0; q < 8; ++q) x[q] = *reinterpret_cast<const float4*>(xs_lane + (t * 8 + q) * 256);
}

// acc[jb][nb] = -m' + sum over the pixel steps of P'^T x  (pixel order = fmaf chain order)
template <bool TRI>
__device__ __forceinline__ void mfma_tile(f32x4 (&acc)[4][2], const FragBuf& f, const float4 (&x)[8]) {
#pragma unroll
  for (int jb = 0; jb < 4; ++jb)
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) acc[jb][nb] = f32x4{f.m[jb].x, f.m[jb].y, f.m[jb].z, f.m[jb].w};
#pragma unroll
  for (int st = 0; st < 16; ++st) {
#pragma unroll
    for (int jb = TRI ? st / 4 : 0; jb < 4; ++jb)
#pragma unroll
      for (int nb = 0; nb < 2; ++nb)
        acc[jb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4_get(f.a[jb][st >> 2], st & 3),
                                                           f4_get(x[nb * 4 + (st >> 2)], st & 3), acc[jb][nb], 0, 0, 0);
  }
}

// Sum of the 16 squared whitened coordinates a lane holds for 16-patch half nb, on v_pk_fma_f32: fp32
// MFMA and fp32 VALU share the SIMD's FMA lanes (tools/mfma_valu_overlap.hip: every v_fma_f32 beside a
// v_mfma_f32_16x16x4_f32 costs ~5.3 cycles of the wave, a packed one ~6.3 for two fmas), so the epilogue is
// priced per instruction and packing halves its biggest part.  Same summation order in forward and
// backward kernels (the logsumexp responsibilities rely on identical log-likelihoods).
using f32x2 = __attribute__((ext_vector_type(2))) float;

__device__ __forceinline__ float sum_squares(const f32x4 (&acc)[4][2], int nb) {
  f32x2 q = {0.f, 0.f};
#pragma unroll
  for (int jb = 0; jb < 4; ++jb) {
    const f32x2 lo = {acc[jb][nb][0], acc[jb][nb][1]}, hi = {acc[jb][nb][2], acc[jb][nb][3]};
    q = __builtin_elementwise_fma(lo, lo, q);
    q = __builtin_elementwise_fma(hi, hi, q);
  }
  return q[0] + q[1];
}

// Running state of the two 16-patch halves of a tile in LDS: st[nb * 16 + n] = max,
// st[32 + nb * 16 + n] = arg-max | sum-exp.  It is read BEFORE the MFMAs of the stage are issued so that
// the LDS latency is off the critical path of finish_tile.
struct TileState {
  float b[2], s[2];
};

template <int MODE>
__device__ __forceinline__ TileState read_state(const float* st) {
  TileState ts;
  if (MODE != MODE_DENSE) {
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) ts.b[nb] = st[nb * 16], ts.s[nb] = st[32 + nb * 16];
  }
  return ts;
}

// l = c_k - q / 2 for the two 16-patch halves of a tile, then the branch-free update of the state.
// PN = PATCH_NORM_STD: plus the residual of c_k (const_k[K + k], jd_gmm_set_const_residual) -- standardized patches are
// small, l is the difference of two numbers several times its size, and the rounding of a float32 c_k shows in it.
template <int MODE, int PN = PATCH_NORM_SUBTRACT_MEAN>
__device__ __forceinline__ void finish_tile(const f32x4 (&acc)[4][2], const TileState& ts, float* st, float ck, int k,
                                            const GmmFwdArgs& a, int n_first, bool writer) {
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    float l = fmaf(-0.5f, sum_lane_groups(sum_squares(acc, nb)), ck);  // gmm.py:276-281
    if constexpr (PN == PATCH_NORM_STD) l += a.const_k[a.K + k];
    float* s0 = st + nb * 16;
    if (MODE == MODE_MAX) {
      const bool better = l > ts.b[nb];  // strict: the lowest component wins a tie, like torch.max
      s0[0] = better ? l : ts.b[nb];
      s0[32] = better ? __int_as_float(k) : ts.s[nb];
    } else if (MODE == MODE_LSE) {
      const float b = ts.b[nb], sm = ts.s[nb];
      const bool better = l > b;
      const float e = expf(better ? b - l : l - b);
      s0[0] = better ? l : b;
      s0[32] = better ? fmaf(sm, e, 1.f) : sm + e;
    } else {
      const int n = n_first + nb * 16;
      if (writer && n < a.n_end) a.value_patch[(size_t)n * a.K + k] = l;
    }
  }
}

// One component over the block's TB tiles, software pipelined by hand: while the MFMAs of tile t
// issue, the wave has the B operands of tile t+1 in flight from LDS and finishes tile t-1 in the VALU
// shadow of the matrix pipe.  Every stage is one basic block (no branches), TB is even and >= 4.
template <int TB, int MODE, bool TRI, int PN = PATCH_NORM_SUBTRACT_MEAN>
__device__ __forceinline__ void sweep_tiles(const FragBuf& f, const float* xs_lane, float* st_lane, float ck, int k,
                                            const GmmFwdArgs& a, int n_lane, bool writer) {
  static_assert(TB >= 4 && TB % 2 == 0, "TB must be even and >= 4");
  float4 x0[8], x1[8];
  f32x4 acc0[4][2], acc1[4][2];
  load_x(x0, xs_lane, 0);
  load_x(x1, xs_lane, 1);
  mfma_tile<TRI>(acc0, f, x0);
  for (int t = 1; t < TB - 1; t += 2) {
    const TileState s0 = read_state<MODE>(st_lane + (t - 1) * 64);
    load_x(x0, xs_lane, t + 1);
    mfma_tile<TRI>(acc1, f, x1);
    finish_tile<MODE, PN>(acc0, s0, st_lane + (t - 1) * 64, ck, k, a, n_lane + 32 * (t - 1), writer);
    const TileState s1 = read_state<MODE>(st_lane + t * 64);
    load_x(x1, xs_lane, t + 2);  // t + 2 <= TB - 1
    mfma_tile<TRI>(acc0, f, x0);
    finish_tile<MODE, PN>(acc1, s1, st_lane + t * 64, ck, k, a, n_lane + 32 * t, writer);
  }
  const TileState s0 = read_state<MODE>(st_lane + (TB - 2) * 64);
  const TileState s1 = read_state<MODE>(st_lane + (TB - 1) * 64);
  mfma_tile<TRI>(acc1, f, x1);
  finish_tile<MODE, PN>(acc0, s0, st_lane + (TB - 2) * 64, ck, k, a, n_lane + 32 * (TB - 2), writer);
  finish_tile<MODE, PN>(acc1, s1, st_lane + (TB - 1) * 64, ck, k, a, n_lane + 32 * (TB - 1), writer);
}

// LDS index (in floats) of pixel p of patch c of tile t in B-fragment order:
// [t][nb = c / 16][st4 = p / 16][g = p % 4][n = c % 16][e = (p % 16) / 4]
__device__ __forceinline__ int xs_index(int t, int c, int p) {
  return (((((t * 2 + (c >> 4)) * 4 + (p >> 4)) * 4 + (p & 3)) * 16 + (c & 15)) << 2) + ((p & 15) >> 2);
}

struct GmmBucketArgs {
  const int32_t* argmax;  // global patch index -> component or -1
  int n_begin, n_end, K;
  int* counts;    // K      bin totals (written by the binscan kernel)
  int* offsets;   // K + 1  exclusive scan of the padded counts; offsets[K] = total slots
  int32_t* order; // slot -> global patch index; the slots offsets[k] + counts[k] .. offsets[k + 1] are padding (undefined)
  int32_t* order_n;  // nullable (record sort): slot -> patch of the record, so that the exact kernel needs one hop less
  float* gpatch;  // rows of filtered patches (argmax < 0) are zeroed here (nullable)
  // screened forward pass only (seg_cnt != nullptr): the elements are candidate records in per-wave segments of
  // seg_cap slots of which the first seg_cnt[segment] are used; a record counts only if its upper bound still
  // reaches the final lower bound of its patch
  const int* seg_cnt;
  int seg_cap;
  const int32_t* rec_n;
  const float* rec_ub;
  const float* lfinal;
  // [K][gridDim.x] (bin major: the binscan kernel walks along a bin): per-block bin counts (count kernel), turned
  // into the block's offset inside each bin (binscan)
  int* blk_counts;
  int chunk;    // elements per chunk (multiple of 256): 1024 patches | one record segment (seg_cap)
  int* flag;    // nullable: the scan kernel stores `gen` here (fallback, see GmmScreenArgs) when the padded buckets
  int gen;      //           need more than slot_cap slots
  int slot_cap;
  int* korder;  // nullable: the scan kernel also ranks the bins by size (order of the components for the next screen)
  // logsumexp screen: records count while their upper bound reaches lfinal - margin (0 in max mode), and the scatter
  // kernel also lists every patch's records: ptab[patch * ptab_rows + j] = bucket slot, j < pcount[patch] (more than
  // ptab_rows records of one patch raise the fallback flag)
  float margin;
  int* pcount;
  int32_t* ptab;
  int ptab_rows;
  const int* dense_mark;  // records of marked patches do not count (the dense kernel evaluates those patches)
};

constexpr int BUCKET_CHUNK = 1024;  // patches per chunk of the backward sort
constexpr int BUCKET_MAX_K = 4096;  // LDS histogram capacity

// First half of the arg-max backward pass: Y^T = P'^T_k Xbar^T - m'_k for the 2 x 16 patch columns of a wave
// (x[nb][st] = pixel 4 st + g of patch 16 nb + n16, mean subtracted), fragments streamed from L2.
template <bool TRI>
__device__ __forceinline__ void whiten_columns(f32x4 (&y)[4][2], const float (&x)[2][16], const float* afrag,
                                               const float* mfrag, int k, int lane) {
  const float4* ak = reinterpret_cast<const float4*>(afrag) + (size_t)k * (AFRAG_FLOATS / 4) + lane;
  const float4* mk = reinterpret_cast<const float4*>(mfrag) + (size_t)k * 16 + (lane >> 4);
#pragma unroll
  for (int jb = 0; jb < 4; ++jb) {
    const float4 m = mk[jb * 4];
    y[jb][0] = y[jb][1] = f32x4{m.x, m.y, m.z, m.w};
#pragma unroll
    for (int st4 = 0; st4 < 4; ++st4) {
      if (TRI && st4 > jb) continue;
      const float4 A = ak[(jb * 4 + st4) * 64];
#pragma unroll
      for (int e = 0; e < 4; ++e)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
          y[jb][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4_get(A, e), x[nb][4 * st4 + e], y[jb][nb], 0, 0, 0);
    }
  }
}

// Second half of the arg-max backward pass, shared by the bucketed kernel, the fused exact kernel and the fallback:
// G^T = P'_k Y^T (k-step (jb, r) feeds lane group g the value y[jb][nb][r]), gamma = -G, minus its mean over the 64
// pixels (adjoint of the mean subtraction); lane (g, n16) writes pixels 16 ib + 4 g + (0..3) of patch (nb, n16) to
// rows[nb] where valid[nb].  The columns (patches) of the MFMA are independent: zero columns change nothing.
// PN = PATCH_NORM_STD: the adjoint of the standardized norm instead (standardized_row_offset), with the kernel's
// arguments `a` and the patches' grid positions and means `sp`.
struct StdPatch {
  int py, px;
  float mean;
};

template <bool TRI, int PN = PATCH_NORM_SUBTRACT_MEAN, class Args = void>
__device__ __forceinline__ void patch_gradient_rows(const f32x4 (&y)[4][2], const float* gfrag, int k, int lane,
                                                    const bool (&valid)[2], float* const (&rows)[2], const Args* a = nullptr,
                                                    const StdPatch* sp = nullptr) {
  const int g = lane >> 4;
  f32x4 gacc[4][2];
  const float4* gk = reinterpret_cast<const float4*>(gfrag) + (size_t)k * (AFRAG_FLOATS / 4) + lane;
#pragma unroll
  for (int ib = 0; ib < 4; ++ib) {
    gacc[ib][0] = gacc[ib][1] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int jb = 0; jb < 4; ++jb) {
      if (TRI && jb < ib) continue;
      const float4 A = gk[(ib * 4 + jb) * 64];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int nb = 0; nb < 2; ++nb)
          gacc[ib][nb] = __builtin_amdgcn_mfma_f32_16x16x4f32(f4_get(A, r), y[jb][nb][r], gacc[ib][nb], 0, 0, 0);
    }
  }
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    float sum = 0.f;
#pragma unroll
    for (int ib = 0; ib < 4; ++ib) sum += (gacc[ib][nb][0] + gacc[ib][nb][1]) + (gacc[ib][nb][2] + gacc[ib][nb][3]);
    const float mean = sum_lane_groups(sum) * (1.f / 64.f);
    if constexpr (PN == PATCH_NORM_STD) {
      const float m = sp[nb].mean;
      const float c = standardized_row_offset(*a, sp[nb].py, sp[nb].px, g, m, mean, [&](int ib, int e) { return gacc[ib][nb][e]; });
      if (valid[nb]) {
        float4* out = reinterpret_cast<float4*>(rows[nb]);
#pragma unroll
        for (int ib = 0; ib < 4; ++ib)
          out[4 * ib + g] = make_float4((c - gacc[ib][nb][0]) / m, (c - gacc[ib][nb][1]) / m, (c - gacc[ib][nb][2]) / m,
                                        (c - gacc[ib][nb][3]) / m);
      }
    } else if (valid[nb]) {
      float4* out = reinterpret_cast<float4*>(rows[nb]);
#pragma unroll
      for (int ib = 0; ib < 4; ++ib)
        out[4 * ib + g] = make_float4(mean - gacc[ib][nb][0], mean - gacc[ib][nb][1], mean - gacc[ib][nb][2],
                                      mean - gacc[ib][nb][3]);
    }
  }
}

struct GmmBwdArgs {
  const float* flux;
  const float* afrag;  // as in the forward kernel
  const float* mfrag;
  const float* gfrag;  // K * [ib 4][jb 4][lane 64][r 4] = P'[16 ib + (lane & 15)][16 jb + 4 (lane >> 4) + r]
  const int32_t* argmax;
  const int32_t* order;
  const int* offsets;  // offsets[K] = total slots
  const int* counts;   // elements of bucket k: the slots behind them up to offsets[k + 1] are padding
  float* gpatch;       // (n_end - n_begin) * 64
  int K, H, W, stride, nPx, shift_y, shift_x, n_begin, n_end;
  const int* shift_dev;  // nullable, device [2] = {shift_y, shift_x} residues: read instead of the two members above (use_device_shift)
};

// Fallback of the fused backward pass (the screen gave up: *flag == gen, otherwise the kernel returns at once): the
// patches in their natural order, 32 per group; the components of a group differ, so the wave serves one distinct
// component after the other with the other patches' columns zeroed.  Per patch the arithmetic is that of
// gmm_bwd_max_kernel (MFMA columns are independent), i.e. the same bits; slow, but so is the dense forward kernel
// that has just run.  Filtered patches (argmax < 0) get a zero row.
struct GmmBwdFallbackArgs {
  const float* flux;
  const float* afrag;
  const float* mfrag;
  const float* gfrag;
  const int32_t* argmax;  // global patch index -> component or -1
  float* gpatch;          // (n_end - n_begin) * 64
  const int* flag;
  int gen;
  int K, H, W, stride, nPx, shift_y, shift_x, n_begin, n_end;
  const int* shift_dev;  // nullable, device [2] = {shift_y, shift_x} residues: read instead of the two members above (use_device_shift)
};

// the groups grp_begin, grp_begin + grp_step, ... < grp_end of 32 patches (group 0 starts at a.n_begin), one wave each
template <bool TRI>
__device__ __forceinline__ void bwd_fallback_groups(const GmmBwdFallbackArgs& a, int grp_begin, int grp_end, int grp_step) {
  const int lane = threadIdx.x & 63;
  const int g = lane >> 4, n16 = lane & 15;
  for (int grp = grp_begin; grp < grp_end; grp += grp_step) {
    int n[2], kk[2];
    bool pending[2];
    float x[2][16];
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const int idx = a.n_begin + 32 * grp + 16 * nb + n16;
      const bool in = idx < a.n_end;
      n[nb] = in ? idx : a.n_begin;
      kk[nb] = in ? a.argmax[idx] : -1;
      pending[nb] = kk[nb] >= 0;
      const int py = n[nb] / a.nPx, px = n[nb] % a.nPx;
#pragma unroll
      for (int st = 0; st < 16; ++st) {
        const int p = 4 * st + g;  // pixel index: row p / 8, column p % 8
        const int yy = wrap(py * a.stride + (p >> 3) - a.shift_y, a.H);
        const int xx = wrap(px * a.stride + (p & 7) - a.shift_x, a.W);
        x[nb][st] = pending[nb] ? a.flux[(size_t)yy * a.W + xx] : 0.f;
      }
      const float mean = patch_mean_groups(x[nb]);
#pragma unroll
      for (int st = 0; st < 16; ++st) x[nb][st] -= mean;
      if (in && !pending[nb]) {
        float4* out = reinterpret_cast<float4*>(a.gpatch + (size_t)(idx - a.n_begin) * D);
#pragma unroll
        for (int ib = 0; ib < 4; ++ib) out[4 * ib + g] = make_float4(0.f, 0.f, 0.f, 0.f);
      }
    }
    for (;;) {
      const unsigned long long b0 = __ballot(pending[0]), b1 = __ballot(pending[1]);
      if ((b0 | b1) == 0ull) break;
      const int k = __builtin_amdgcn_readfirstlane(b0 ? __shfl(kk[0], __ffsll((long long)b0) - 1) : __shfl(kk[1], __ffsll((long long)b1) - 1));
      bool act[2];
      float xm[2][16];
#pragma unroll
      for (int nb = 0; nb < 2; ++nb) {
        act[nb] = pending[nb] && kk[nb] == k;
#pragma unroll
        for (int st = 0; st < 16; ++st) xm[nb][st] = act[nb] ? x[nb][st] : 0.f;
      }
      f32x4 y[4][2];
      whiten_columns<TRI>(y, xm, a.afrag, a.mfrag, k, lane);
      float* rows[2] = {a.gpatch + (size_t)(n[0] - a.n_begin) * D, a.gpatch + (size_t)(n[1] - a.n_begin) * D};
      patch_gradient_rows<TRI>(y, a.gfrag, k, lane, act, rows);
      pending[0] = pending[0] && !act[0];
      pending[1] = pending[1] && !act[1];
    }
  }
}

struct GmmBwdLseArgs {
  const float* flux;
  const float* afrag;
  const float* mfrag;
  const float* gfrag;
  const float* const_k;
  double* partials;          // one per block: the sum of the logsumexp values of its patches
  float* gpatch;             // (n_end - n_begin) * 64
  int K, H, W, stride, nPx, shift_y, shift_x, n_begin, n_end;
  const int* shift_dev;  // nullable, device [2] = {shift_y, shift_x} residues: read instead of the two members above (use_device_shift)
  // Behind the logsumexp screen (mark != nullptr): the kernel evaluates the 32-patch groups that hold a marked patch
  // (more candidates than a patch may keep: smooth patches, where most components are within the margin) -- or, after a
  // fallback of the pass (*run_flag == run_gen), all of them -- and leaves v per patch in vpatch (0 for a filtered
  // patch) instead of the partial sums; rows and values of unmarked patches of a visited group are NOT written (the
  // combine kernel owns them).
  const int* run_flag;
  int run_gen;
  const int* mark;
  float* vpatch;
  const int32_t* list;       // the marked patches, compacted (gmm_lse_list_kernel), and their number: a wave works on 64
  const int* list_count;     // of THEM at a time, so that the launch takes as long as their share of the image
};

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int SCREEN_T = 4;        // tiles of 32 patches per wave
constexpr int SCREEN_CAP = 4096;   // candidate records a wave can hold (128 patches: 32 per patch); multiple of BUCKET_CHUNK
constexpr int A16_BLOCKS = 6;      // non-zero (32 coordinates x 16 pixels) blocks of an upper triangular P'
constexpr float SCREEN_EPS = 0.001f;  // two fp16 roundings 2^-10 + 2^-22, two fp32 accumulations of 64 terms, slack
constexpr int KORDER_MAX_K = 1024;  // the popularity order of the components is maintained up to this K

struct GmmScreenArgs {
  const float* flux;
  const uint4* afrag16;  // K * A16_BLOCKS * 64 lanes * 8 fp16 of P'_k / s_k
  const float* const_k;  // K
  const float* efro_k;   // K: SCREEN_EPS * |P'_k|_F (rounded up)
  const float* sk2_k;    // K: s_k^2, the squared power-of-two scale of the fp16 fragments
  const float* mnorm_k;  // K: 1.001 |m'_k| (0 for a zero-mean component)
  int K, H, W, stride, nPx, shift_y, shift_x, n_begin, n_end;
  const int* shift_dev;  // nullable, device [2] = {shift_y, shift_x} residues: read instead of the two members above (use_device_shift)
  const int* korder;         // K: the order in which the components are visited (most popular first)
  const uint4* xfrag;        // staged patches (gmm_stage_kernel): fp16 B fragments [tile][pixel step][lane],
  const float* xn;           //   1.0001 |xbar|, s_x^2 and validity per [tile * 32 + c]
  const float* xs2;
  const int* ok;
  float* lfinal;             // per patch: max_k (ltilde - B), a lower bound of the true maximum
  int32_t* rec_n;            // [waves][SCREEN_CAP] candidate records: patch (global index),
  int32_t* rec_k;            //                     component,
  float* rec_ub;             //                     upper bound ltilde + B
  int* seg_cnt;              // [waves] records used
  // Fallback flag: a pass that gives up stores its generation number `gen` (> 0, different for consecutive passes
  // of a handle) here; every later kernel of the pass compares the flag with gen.  Nothing ever has to clear it.
  int* flag;
  int gen;
  int* dense_mark;           // logsumexp screen: per patch (global index), zeroed by the staging kernel; set to 1 for a
                             // patch with more candidates than a patch may keep -- its records are dropped and the
                             // dense kernel evaluates it
  // CLOCK instantiation (jd_gmm_screen_clock): block b < clock_cap leaves the shader-clock ticks and the 100 MHz reference
  // ticks between its first and its last instruction at [2 b], [2 b + 1]: the clock the board holds INSIDE this kernel
  unsigned long long* clock_stamps;
  int clock_cap;
};

// Arguments of gmm_stage_kernel (gmm_screen.hip): the patch staging of the screen
struct GmmStageArgs {
  const float* flux;
  int H, W, stride, nPx, shift_y, shift_x, n_begin, n_end, n_tiles;
  const int* shift_dev;  // nullable, device [2] = {shift_y, shift_x} residues: read instead of the two members above (use_device_shift)
  uint4* xfrag;              // [tile][pixel step 4][lane 64] = 8 fp16 of xbar / s_x (B fragment of the 32x32x16 MFMA)
  float* xn;                 // [tile * 32 + c] 1.0001 |xbar|
  float* xs2;                // s_x^2
  int* ok;                   // patch takes part (inside the shard, passes the -1e5 filter)
  unsigned long long* best;  // per patch (global index): initialised here
  int* pcount;               // nullable (logsumexp screen): records per patch (global index), zeroed here
  int* dense_mark;           //   and the "evaluate densely" mark of the patch
  int* dense_count;          //   and (one int) the length of the list of marked patches
};

constexpr int SCREEN_KC_MAX = 512;  // components whose per-component constants are staged in LDS in visiting order

struct GmmExactArgs {
  const float* flux;
  const float* afrag;
  const float* mfrag;
  const float* const_k;
  const int32_t* order_n; // bucket slot -> patch of the record (only the first counts[k] slots of a bucket are written)
  const int* counts;      // K
  const int* offsets;     // K + 1, offsets[K] = total (padded) bucket slots
  const int* flag;
  int gen;                // the pass has fallen back to the dense kernel when *flag == gen
  unsigned long long* best;
  int K, H, W, stride, nPx, shift_y, shift_x;
  const int* shift_dev;  // nullable, device [2] = {shift_y, shift_x} residues: read instead of the two members above (use_device_shift)
  // fused backward pass (grec != nullptr): the gradient row of EVERY surviving record is written to grec[bucket slot]
  // and the key carries the bucket slot instead of the component (slots ascend with the component, so ties still go
  // to the lowest component); gmm_best_kernel turns the winning key into the row the gather kernel reads
  const float* gfrag;
  float* grec;
  float* lrec;  // nullable (logsumexp screen): l of every surviving record by bucket slot, instead of the max merge
#ifdef JD_EXACT_STAMPS  // diagnostic build only (make VARIANT=stamps EXTRA=-DJD_EXACT_STAMPS=1): s_memtime per phase of a group
  unsigned long long* stamps;  // [group][8]
#endif
};

struct GmmBestArgs {
  const unsigned long long* best;
  int n_begin, n_end;
  int32_t* argmax_out;  // nullable
  double* partials;     // one per block
  // fused backward pass (winner != nullptr): unless the pass fell back (*flag == gen), the low word of a key is the
  // bucket slot of the winning record -> winner[n] (-1: no gradient); the component is looked up only if asked for.
  // After a fallback the keys carry components (dense kernel): they go to argmax_fb for the fallback backward pass of this kernel (fb).
  const int* flag;
  int gen;
  int32_t* winner;
  int32_t* argmax_fb;
  const int32_t* rec_k;
  const int32_t* rec_order;
  // the block that finishes last turns the partial sums into the prior value (what finalize_sum_kernel would do in a
  // launch of its own, same summation order): value_out = [value_out +] scale * sum(partials)
  int* ticket;  // zero between launches
  double scale;
  float* value_out;
  int accumulate;
  // what the NEXT call's host code wants to know, stored into host-mapped memory by the finishing block (no copy, no
  // synchronisation: the host reads whatever pass has landed): {generation, fell back, bucket slots used, patches}
  int* host_stats;          // nullable
  const int* slots_used;    // offsets[K] of the record sort
  // fused backward pass after a fallback (fb.gpatch != nullptr and *flag == gen): every block produces the gradient
  // rows of its own 1024 patches from the components it has just decoded -- the work of a kernel of its own that in the
  // normal case was a 4.6 us launch returning at once
  GmmBwdFallbackArgs fb;
};

struct GmmLseCombineArgs {
  const int* pcount;      // records per patch (global index)
  const int32_t* ptab;    // [patch][rows] bucket slots
  int rows;
  const float* lrec;      // l by bucket slot
  const float* grec;      // gradient rows by bucket slot
  float* gpatch;          // (n_end - n_begin) * 64: the combined rows
  float* vpatch;          // v per patch (global index); 0 for a filtered patch
  const int* mark;        // patches the dense kernel evaluates: not touched here
  int n_begin, n_end;
  const int* flag;
  int gen;
};

// The geometry every kernel that cuts patches out of the image takes: one assignment for all argument blocks (the
// source is a PatchGrid or another argument block that has the members).
struct PatchGrid {
  int H, W, stride, nPx, shift_y, shift_x;
  const int* shift_dev;
};
template <class A, class G>
void set_patch_grid(A& a, const G& g) {
  a.H = g.H, a.W = g.W, a.stride = g.stride, a.nPx = g.nPx, a.shift_y = g.shift_y, a.shift_x = g.shift_x, a.shift_dev = g.shift_dev;
}

// Owning device array, grown on demand: the contents are NOT kept across a reserve (free, then hipMalloc).
template <class T>
struct DevBuf {
  T* ptr = nullptr;
  size_t cap = 0;  // elements
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { if (ptr) (void)hipFree(ptr); }
  int reserve(size_t n) {
    if (n <= cap) return JD_OK;
    if (ptr) (void)hipFree(ptr);
    ptr = nullptr, cap = 0;
    JD_HIP(hipMalloc(&ptr, n * sizeof(T)));
    cap = n;
    return JD_OK;
  }
};

// Four ints of host-mapped memory {generation, fell back, bucket slots used, patches}: what the last block of a screened
// pass leaves for the NEXT call's host code (optional: without it the record buffer keeps its initial capacity).
struct MappedStats {
  int* host = nullptr;  // hipHostMalloc (mapped)
  int* dev = nullptr;   // its device address
  MappedStats() = default;
  MappedStats(const MappedStats&) = delete;
  MappedStats& operator=(const MappedStats&) = delete;
  ~MappedStats() { if (host) (void)hipHostFree(host); }
};

constexpr int SCREEN_CLOCK_CAP = 4096;  // blocks of a screen launch that leave clock stamps

struct GmmPass {  // a pass between its two phases (gmm_prior_impl): what the gather must find unchanged
  bool valid = false;
  int H = 0, W = 0, stride = 0, shift_y = 0, shift_x = 0, row_begin = 0, row_end = 0, marginalize = 0;
  bool fused = false, lse_screened = false;
  int gen = 0;
  const int* shift_dev = nullptr;
  ImageNormArgs norm{};  // image norm of its phase 1 (the gather's chain rule must be that norm's)
  int patch_norm = PATCH_NORM_SUBTRACT_MEAN;  // patch norm of its phase 1 (the rows are that norm's)
};

}  // namespace jd

// The handle.  Every device array is a DevBuf: `delete` frees them all.  Fields are grouped by the stage that owns them.
struct jd_gmm {
  jd::Gmm256* d256 = nullptr;  // a D = 256 handle: everything but the image norm lives in gmm256.hip
  jd::GmmPass pass;
  jd::ImageNormArgs norm{};  // image norm the next prior call takes (jd_gmm_set_image_norm; kind 0 = identity)
  int patch_norm = jd::PATCH_NORM_SUBTRACT_MEAN;  // patch norm the next prior call takes (jd_gmm_set_patch_norm)
  // The image a pass cuts its patches from where that is not the flux: n(flux), (H, W), under an image norm; the staged
  // image S of a staged pass (gmm_subpix.hip: (H, W); gmm_jitter.hip: (n_y P, n_x P)), which is normed already.
  jd::DevBuf<float> normed;
  jd::DevBuf<float> staged_grad;  // staged passes: G, the gradient of the inner pass with respect to S, the shape of S
  int reserve_staged(size_t n, bool want_grad) {  // S and, for a gradient, G of a staged pass of n pixels
    if (const int rc = normed.reserve(n)) return rc;
    return want_grad ? staged_grad.reserve(n) : JD_OK;
  }
  struct PriorImage {  // jd_gmm_prior_image (gmm_prior_image.hip): winner and mean per patch, the value its forward pass leaves
    jd::DevBuf<int32_t> winner;
    jd::DevBuf<float> mean;
    jd::DevBuf<float> value;
  } prior_image;
  int K = 0;
  bool triangular = true;  // every P_k upper triangular -> zero blocks are skipped
  int n_cu = 256;
  struct Dense {  // the mixture in fp32 MFMA fragment order and the workspaces of the dense kernels (grown on demand)
    jd::DevBuf<float> afrag, mfrag, const_k, gfrag;
    jd::DevBuf<int32_t> argmax;
    jd::DevBuf<float> gpatch;
    jd::DevBuf<double> partials;
  } dense;
  struct Sort {  // counting sort by component: of the patches (bucketed backward pass) and of the screen's records
    jd::DevBuf<int> bucket;  // counts (K) | unused (K) | offsets (K + 1)
    jd::DevBuf<int32_t> order;
    jd::DevBuf<int> blk_counts;  // per-block bin counts
  } sort;
  struct Screen {  // screened arg-max (upper triangular mixtures): fp16 fragments, bound constants, work space
    bool ok = false;
    jd::DevBuf<uint4> afrag16;
    jd::DevBuf<float> efro_k, sk2_k, mnorm_k;
    jd::DevBuf<int> korder;  // K: visiting order of the components (most survivors in the previous call first)
    jd::DevBuf<int> ctl;     // [0] fallback flag (generation stamped) | counts (K) | unused (K) | offsets (K + 1) | ticket
    int gen = 0;             // generation of the current screened pass (1 .. 2^30, never 0)
    jd::DevBuf<unsigned long long> best;
    jd::DevBuf<float> lfinal;
    jd::DevBuf<uint4> xfrag;  // staged patches of the screen: fp16 fragments, norms | scales (floats), validity
    jd::DevBuf<float> xstat;
    jd::DevBuf<int> xok;
    jd::DevBuf<int32_t> rec;  // candidate records: patch | component | upper bound (as float), `slots` each
    jd::DevBuf<int32_t> rec_order;
    jd::DevBuf<int32_t> rec_order_n;  // bucket slot -> patch of the record
    jd::DevBuf<int> seg_cnt;
    jd::DevBuf<unsigned long long> clock_stamps;  // jd_gmm_screen_clock: 2 x SCREEN_CLOCK_CAP ticks, zero = not written
  } screen;
  struct Lse {  // logsumexp screen: l per bucket slot, records per patch and their bucket slots, the partial sums
    jd::DevBuf<float> lrec;
    jd::DevBuf<int> pcount;
    jd::DevBuf<int32_t> ptab;
    jd::DevBuf<double> partials;
    jd::DevBuf<int> dense_mark;      // patches the dense kernel evaluates (too many candidates)
    jd::DevBuf<int> marked;          // their number per block of the value kernel
    jd::DevBuf<int32_t> dense_list;  // the marked patches, compacted (+ one int in front: their number)
    jd::DevBuf<float> vpatch;        // logsumexp per patch
    // Where (nearly) all components are within the margin of the maximum -- smooth images under a mixture with similar
    // constants -- the screen cannot pay: every pass overflows a record list and falls back to the dense kernels after 0.5 ms.
    // After such a pass with the record buffer at its largest the next `skip` passes go dense; then the screen is tried again.
    int skip = 0;
    int seen_gen = 0;
    bool last_pass = false;
  } lse;
  struct Fused {  // fused backward pass of the screened path
    jd::DevBuf<float> grec;      // gradient rows of the surviving records, by bucket slot
    jd::DevBuf<int32_t> winner;  // patch -> bucket slot of its winning record
    // Gradient rows per patch the record buffer has room for (x 256 B x patches).  Starts at 4; a pass that fell back
    // because it needed more, or filled more than 60 % of it, doubles it for the following passes (up to 32) -- known
    // from the host-mapped statistics the last block of gmm_best_kernel leaves behind, read without synchronisation.
    int rows_per_patch = 4;
    jd::MappedStats stats;
    int stats_seen_gen = 0;
  } fused;
};

namespace jd {

// ---- launch functions one unit calls in another ---------------------------------------------------------------------
// gmm_dense.hip.  launch_fwd: gmm_fwd_kernel in mode MODE_MAX | MODE_LSE | MODE_DENSE, one fp64 partial sum per block
// (*n_partials = number of blocks), under its own profile scope; launch_fwd_blocks: the same launch without the scope
// and without the JD_GMM_DENSE override (the gated fallback of the screened path).
// patch_norm: PATCH_NORM_* of the pass (MODE_DENSE takes finished patches and has none).
int launch_fwd(int mode, const GmmFwdArgs& a, bool tri, int n_cu, hipStream_t s, int* n_partials,
               int patch_norm = PATCH_NORM_SUBTRACT_MEAN);
int launch_fwd_blocks(int mode, const GmmFwdArgs& a, bool tri, int n_cu, hipStream_t s, int* n_partials,
                      int patch_norm = PATCH_NORM_SUBTRACT_MEAN);
void launch_bwd_max(const GmmBwdArgs& b, bool tri, unsigned blocks, hipStream_t s, int patch_norm = PATCH_NORM_SUBTRACT_MEAN);
void launch_bwd_lse(const GmmBwdLseArgs& b, bool tri, unsigned blocks, hipStream_t s, int patch_norm = PATCH_NORM_SUBTRACT_MEAN);
// gmm_sort.hip: count -> binscan -> scatter over `chunks` blocks
void launch_bucket_sort(const GmmBucketArgs& bk, unsigned chunks, hipStream_t s);
// gmm_screen.hip (see there)
int screened_forward(jd_gmm* g, const GmmFwdArgs& a, hipStream_t s, int* n_partials, bool fused, int32_t* fallback_argmax,
                     double value_scale, float* value_out, int accumulate_value, bool lse = false);
// gmm_gather.hip: out = n(in) per pixel; the overlap-add of the gradient rows (tile kernel | per-pixel kernel)
int launch_image_norm(const float* in, float* out, size_t n, const ImageNormArgs& nm, int n_cu, hipStream_t s);
int launch_gather(const GmmGatherArgs& ga, hipStream_t s);
// gmm.hip: the whole prior of an image under the image norm `norm` -- both patch sizes, both phases, no shard; otherwise the
// contract of jd_gmm_prior_fwd_bwd, which is this under the handle's norm.  The staged passes run it on their staged
// image under the identity.
int gmm_prior_whole(jd_gmm* g, const ImageNormArgs& norm, const float* flux, int H, int W, int stride, int shift_y, int shift_x,
                    int marginalize, float value_scale, float* value_out, int accumulate_value, float grad_coef,
                    float* grad_flux_accum, int32_t* argmax_out, const int* shift_dev, void* stream);

// f(std::bool_constant<A>{}, std::bool_constant<B>{}): the host's way to one of the four instantiations of a kernel with
// two switches (the adjoint kernels of the staged passes: NORM, VEC)
template <class F>
void dispatch_bools(bool a, bool b, F&& f) {
  if (a) b ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
  else b ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}

}  // namespace jd
