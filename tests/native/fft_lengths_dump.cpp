// Prints what csrc/jd_fftcore.h decides for every n up to 9216: the padded length of a row of n points, of a column of n
// points, and the radix schedule of n (empty: not a supported length).  tests/test_fft_length_cases_host.py compares the
// plain-Python mirror of tests/fft_length_cases.py with these lines.
#include <cstdio>
#include <initializer_list>

#include "jd_fftcore.h"

int main() {
  for (int n = 1; n <= 9216; ++n) {
    const jdfft::Radices f = jdfft::factorize(n);
    std::printf("%d %d %d :", n, jdfft::next_length(n), jdfft::next_length(n, false));
    for (int s = 0; s < f.n; ++s) std::printf(" %d", f.r[s]);
    std::printf("\n");
  }
  return 0;
}
