// Host check of csrc/jd_jitter.h (tests/test_gmm_jitter_host.py): reads records "n P s roll count draw_0 ... draw_{count-1}"
// from standard input and prints, per record, "axis n P s count safe maxc" and, per un-rolled pixel p, "p Y lo hi k idx_0 ...
// idx_{k-1}": the rolled position, the candidate window and the rows of the staged image that hold the pixel.
#include <cstdio>
#include <vector>

#include "jd_jitter.h"

int main() {
  int n, P, s, roll, count;
  while (std::scanf("%d %d %d %d %d", &n, &P, &s, &roll, &count) == 5) {
    std::vector<int> draws(count > 0 ? count : 1);
    for (int i = 0; i < count; ++i)
      if (std::scanf("%d", &draws[i]) != 1) return 2;
    const int maxc = jd::jitter_window_max(P, s);
    std::printf("axis %d %d %d %d %d %d\n", n, P, s, jd::jitter_count(n, P, s), (int)jd::jitter_safe(n, P, s), maxc);
    if (jd::jitter_count(n, P, s) != count) continue;
    std::vector<int> out(maxc + 1, -1);
    for (int p = 0; p < n; ++p) {
      const int Y = jd::jitter_mod(p + roll, n);
      int lo, hi;
      jd::jitter_window(Y, P, s, count, &lo, &hi);
      const int k = jd::jitter_cover(Y, P, s, count, draws.data(), out.data(), 1);
      if (k > maxc || out[maxc] != -1) return 3;  // (a list longer than its bound)
      std::printf("%d %d %d %d %d", p, Y, lo, hi, k);
      for (int c = 0; c < k; ++c) std::printf(" %d", out[c]);
      std::printf("\n");
    }
  }
  return 0;
}
