// Index arithmetic of the jittered patch grid of the GMM patch prior (jolideco/utils/torch.py:278-334,
// `view_as_random_overlapping_patches_torch`), shared by the two kernels of gmm_jitter.hip and the entry's host checks.
// Plain integer functions, host and device, so that the CPU suite compiles and checks them (tests/native/jitter_check.cpp).
//
// Along one axis of length n, patch size P, stride s, overlap = P - s:
//   base   = arange(overlap, n - s - overlap, s)           count = len(base)
//   pos_i  = overlap + i s + clamp(draw_i, -overlap, overlap)     i s <= pos_i <= i s + 2 overlap
// The axis is SAFE when every position a draw can give keeps its patch inside: max(base) + overlap <= n - P.
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define JD_JITTER_HD __host__ __device__ __forceinline__
#else
#define JD_JITTER_HD inline
#endif

namespace jd {

// v mod n in [0, n) for every int v (n > 0)
JD_JITTER_HD int jitter_mod(int v, int n) {
  const int r = v % n;
  return r < 0 ? r + n : r;
}

// len(arange(overlap, n - s - overlap, s)); 0 where the range is empty
JD_JITTER_HD int jitter_count(int n, int P, int s) {
  const int overlap = P - s, span = n - s - 2 * overlap;
  return span > 0 ? (span + s - 1) / s : 0;
}

// at least one patch, and the last base position plus the largest draw keeps the patch inside the axis
JD_JITTER_HD bool jitter_safe(int n, int P, int s) {
  const int count = jitter_count(n, P, s), overlap = P - s;
  return count > 0 && overlap + (count - 1) * s + overlap <= n - P;
}

// position of patch i; a draw outside [-overlap, overlap] is clamped (the arrays live on the device: not validated)
JD_JITTER_HD int jitter_pos(int i, int P, int s, int draw) {
  const int overlap = P - s;
  const int d = draw < -overlap ? -overlap : (draw > overlap ? overlap : draw);
  return overlap + i * s + d;
}

// the patches that CAN cover pixel Y (0 <= Y): i in [lo, hi] (empty when lo > hi), from i s <= pos_i <= i s + 2 overlap:
// lo = ceil((Y - 2 overlap - P + 1) / s), hi = floor(Y / s), both cut to [0, count - 1]
JD_JITTER_HD void jitter_window(int Y, int P, int s, int count, int* lo, int* hi) {
  const int num = Y - 2 * (P - s) - P + 1;
  const int top = Y / s;
  *lo = num > 0 ? (num + s - 1) / s : 0;
  *hi = top < count - 1 ? top : count - 1;
}

// upper bound of hi - lo + 1 for any Y: what a pixel's cover list can hold
JD_JITTER_HD int jitter_window_max(int P, int s) { return (2 * (P - s) + P - 1) / s + 1; }

// The patches that DO cover pixel Y, i ascending: out[c] = i P + (Y - pos_i), the row (column) of the staged image that
// holds pixel Y of patch i.  Returns their number (<= jitter_window_max); writes nothing beyond it.
JD_JITTER_HD int jitter_cover(int Y, int P, int s, int count, const int* draws, int* out, int out_stride) {
  int lo, hi, c = 0;
  jitter_window(Y, P, s, count, &lo, &hi);
  for (int i = lo; i <= hi; ++i) {
    const int a = Y - jitter_pos(i, P, s, draws[i]);
    if (a >= 0 && a < P) out[(c++) * out_stride] = i * P + a;
  }
  return c;
}

}  // namespace jd
