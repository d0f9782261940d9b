// CPU check of csrc/jd_fftcore.h at the lengths of the wide images (rows up to 9216 points on the 768-thread row kernels,
// columns of 4096 and 4608 points on four waves): the radix schedules, run butterfly by butterfly on the host, against a
// float64 DFT at the bound of fftcore_check.cpp, and the padded lengths those images get.  Build + run (plain and under
// the address / undefined-behaviour sanitizers): tests/test_fft_wide_host.py.
#include <cmath>
#include <complex>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "jd_fftcore.h"

using namespace jdfft;

template <int DIR>
static void run_pass(int R, const float2* x, float2* y, int N, int p, const float2* tw) {
  for (int b = 0; b < N / R; ++b) switch (R) {
      case 16: pass_one<16, DIR>(x, y, N, p, tw, b); break;
      case 8: pass_one<8, DIR>(x, y, N, p, tw, b); break;
      case 4: pass_one<4, DIR>(x, y, N, p, tw, b); break;
      case 2: pass_one<2, DIR>(x, y, N, p, tw, b); break;
      case 9: pass_one<9, DIR>(x, y, N, p, tw, b); break;
      case 3: pass_one<3, DIR>(x, y, N, p, tw, b); break;
      default: std::abort();
    }
}

// float64 DFT of a sequence by two stages N = A * B (A = 64: every length here is a multiple of it): exact arithmetic of
// the Cooley-Tukey split in double precision -- 9216^2 complex exponentials per direction would take the test's time
static void dft64(const std::vector<std::complex<double>>& in, std::vector<std::complex<double>>& out, int N, int dir) {
  const int A = 64, B = N / A;
  std::vector<std::complex<double>> w(N), mid((size_t)A * B);
  for (int m = 0; m < N; ++m) w[m] = std::polar(1.0, dir * 2.0 * M_PI * m / N);
  // n = A n1 + n2, k = k1 + B k2:  X[k] = sum_n2 w_N^(n2 k1) w_A^(n2 k2) sum_n1 w_B^(n1 k1) x[A n1 + n2]
  for (int n2 = 0; n2 < A; ++n2)
    for (int k1 = 0; k1 < B; ++k1) {
      std::complex<double> s = 0.0;
      for (int n1 = 0; n1 < B; ++n1) s += in[A * n1 + n2] * w[(size_t)A * ((long)n1 * k1 % B)];
      mid[(size_t)n2 * B + k1] = s * w[(long)n2 * k1 % N];
    }
  for (int k1 = 0; k1 < B; ++k1)
    for (int k2 = 0; k2 < A; ++k2) {
      std::complex<double> s = 0.0;
      for (int n2 = 0; n2 < A; ++n2) s += mid[(size_t)n2 * B + k1] * w[(size_t)B * (n2 * k2 % A)];
      out[k1 + B * k2] = s;
    }
}

static double check(int N, int dir) {
  const Radices f = factorize(N);
  if (!f.n) return -1.0;
  std::vector<float2> tw(N), a(lp_size(N)), b(lp_size(N));
  for (int m = 0; m < N; ++m) tw[m] = float2{(float)std::cos(-2.0 * M_PI * m / N), (float)std::sin(-2.0 * M_PI * m / N)};
  std::vector<std::complex<double>> in(N), ref(N);
  srand(N + dir);
  for (int i = 0; i < N; ++i) {
    in[i] = {rand() / (double)RAND_MAX - 0.3, rand() / (double)RAND_MAX - 0.6};
    a[lp(i)] = float2{(float)in[i].real(), (float)in[i].imag()};
    in[i] = {(double)a[lp(i)].x, (double)a[lp(i)].y};
  }
  float2 *x = a.data(), *y = b.data();
  int p = 1;
  for (int s = 0; s < f.n; ++s) {
    if (dir < 0) run_pass<-1>(f.r[s], x, y, N, p, tw.data());
    else run_pass<1>(f.r[s], x, y, N, p, tw.data());
    p *= f.r[s];
    std::swap(x, y);
  }
  dft64(in, ref, N, dir);
  double norm = 0.0, err = 0.0;
  for (int k = 0; k < N; ++k) norm = std::fmax(norm, std::abs(ref[k]));
  for (int k = 0; k < N; ++k) err = std::fmax(err, std::abs(std::complex<double>(x[lp(k)].x, x[lp(k)].y) - ref[k]));
  return err / norm;
}

int main() {
  int bad = 0;
  for (int N : {4096, 4608, 6144, 8192, 9216}) {
    for (int dir : {-1, 1}) {
      const double e = check(N, dir);
      const Radices f = factorize(N);
      std::printf("N %5d dir %+d passes", N, dir);
      for (int s = 0; s < f.n; ++s) std::printf(" %d", f.r[s]);
      std::printf("  rel err %.2e%s\n", e, e >= 0 && e < 1e-6 ? "" : "  BAD");
      bad += !(e >= 0 && e < 1e-6);
    }
  }
  // rows (lengths 2^a * {1, 3, 9}) and columns (no factor 3) of images beyond 4608 padded points
  const int rows[3][2] = {{4802, 6144}, {8004, 8192}, {8200, 9216}}, cols[2][2] = {{2358, 4096}, {4112, 4608}};
  for (const auto& r : rows) {
    const int got = next_length(r[0]);
    std::printf("next_length rows: %d -> %d%s\n", r[0], got, got == r[1] ? "" : "  BAD");
    bad += got != r[1];
  }
  for (const auto& c : cols) {
    const int got = next_length(c[0], false);
    std::printf("next_length columns: %d -> %d%s\n", c[0], got, got == c[1] ? "" : "  BAD");
    bad += got != c[1];
  }
  return bad ? 1 : 0;
}
