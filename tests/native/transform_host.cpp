// The transform passes of thevc_amd/csrc/hmx_transform.h on the CPU (g++, no HIP): every pass in every form -- multiply-add chains,
// DST butterflies, the loops they replace -- against the plain matrix product written out HERE: y = wrap16((M x + rnd) >> shift)
// forward, clip16((M^T c + rnd) >> shift) inverse, in 64-bit arithmetic.  The matrix does not come from the header: the angle of
// entry (k, n) is folded with cos() / acos() in floating point onto the 33 integers of the standard, and the 4-point matrices and a
// row of the 8-point one are checked against literals.
//
// Sizes 4 (DST and DCT), 8, 16, 32; the shifts the chains use at 8, 10 and 12 bit (forward LG - 1 + (B - 8) and LG + 6, inverse 7
// and 12 - (B - 8)).  Inverse inputs: all -32768, all 32767, alternating extremes in both phases, every single impulse of either
// extreme, random int16.  Forward inputs: the same patterns over the residual range +-(2^B - 1), and the first pass's own outputs
// of those (what the second pass sees), plus random int16 for the second-pass shift.  Prints the number of vectors; exit status 1
// and the first mismatch on stderr otherwise.  tests/test_transform_host.py also builds it with -fsanitize=undefined,address.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "hmx_transform.h"

static int mat[33][33]; // the matrix under test's reference, filled per size
static void fill_dct(int N) {
  static const int tab[33] = {64, 90, 90, 90, 89, 88, 87, 85, 83, 82, 80, 78, 75, 73, 70, 67, 64,
                              61, 57, 54, 50, 46, 43, 38, 36, 31, 25, 22, 18, 13, 9,  4,  0};
  const double pi = std::acos(-1.0);
  for (int k = 0; k < N; k++)
    for (int n = 0; n < N; n++) {
      const double v = std::cos((2 * n + 1) * k * pi / (2 * N));
      const int idx = (int)std::lround(std::acos(std::fabs(v)) * 64 / pi);
      mat[k][n] = (k == 0 ? 64 : (v < 0 ? -tab[idx] : tab[idx]));
    }
}
static void fill_dst() {
  static const int t[4][4] = {{29, 55, 74, 84}, {74, 74, 0, -74}, {84, -29, -74, 55}, {55, -84, 74, -29}};
  for (int k = 0; k < 4; k++)
    for (int n = 0; n < 4; n++) mat[k][n] = t[k][n];
}

static long n_vectors = 0;
static int fail(const char *what, int N, int F, int shift, int i, int got, int want) {
  std::fprintf(stderr, "%s N=%d forms=%d shift=%d output %d: got %d, want %d\n", what, N, F, shift, i, got, want);
  return 1;
}

template <int N, int F>
static int check_fwd(const int *x, int shift, bool dst, int *y) {
  hmx::fwd_pass<N, F>(x, y, shift, dst);
  for (int k = 0; k < N; k++) {
    int64_t s = 0;
    for (int n = 0; n < N; n++) s += (int64_t)mat[k][n] * x[n];
    const int want = (int)(int16_t)((s + ((int64_t)1 << (shift - 1))) >> shift);
    if (y[k] != want) return fail(dst ? "forward DST" : "forward", N, F, shift, k, y[k], want);
  }
  n_vectors++;
  return 0;
}
template <int N, int F>
static int check_inv(const int *c, int shift, bool dst) {
  int y[N];
  hmx::inv_pass<N, F>(c, y, shift, dst);
  for (int n = 0; n < N; n++) {
    int64_t s = 0;
    for (int k = 0; k < N; k++) s += (int64_t)mat[k][n] * c[k];
    int64_t want = (s + ((int64_t)1 << (shift - 1))) >> shift;
    want = want < -32768 ? -32768 : want > 32767 ? 32767 : want;
    if (y[n] != (int)want) return fail(dst ? "inverse DST" : "inverse", N, F, shift, n, y[n], (int)want);
  }
  n_vectors++;
  return 0;
}

// the patterns over [lo, hi]: constants, alternating in both phases, impulses of either end on zero and on the other end
template <int N>
static void patterns(int lo, int hi, std::vector<std::vector<int>> &out) {
  std::vector<int> v(N);
  for (int e : {lo, hi, 0}) out.push_back(std::vector<int>(N, e));
  for (int ph = 0; ph < 2; ph++) {
    for (int i = 0; i < N; i++) v[i] = ((i + ph) & 1) ? hi : lo;
    out.push_back(v);
    for (int i = 0; i < N; i++) v[i] = (((i >> 1) + ph) & 1) ? hi : lo;
    out.push_back(v);
    for (int i = 0; i < N; i++) v[i] = ((i < N / 2) != (ph == 1)) ? hi : lo;
    out.push_back(v);
  }
  for (int i = 0; i < N; i++)
    for (int e : {lo, hi})
      for (int bg : {0, e == lo ? hi : lo}) {
        v.assign(N, bg);
        v[i] = e;
        out.push_back(v);
      }
}

template <int N, int F>
static int run_size(bool dst, std::mt19937 &rng) {
  const int LG = N == 4 ? 2 : N == 8 ? 3 : N == 16 ? 4 : 5;
  if (dst) fill_dst();
  else fill_dct(N);
  std::uniform_int_distribution<int> i16(-32768, 32767);
  for (int B : {8, 10, 12}) {
    const int s1 = LG - 1 + (B - 8), s2 = LG + 6, i1 = 7, i2 = 12 - (B - 8), r = (1 << B) - 1;
    std::vector<std::vector<int>> fw, iv;
    patterns<N>(-r, r, fw);
    std::uniform_int_distribution<int> res(-r, r);
    for (int t = 0; t < 3000; t++) {
      std::vector<int> v(N);
      for (int &e : v) e = res(rng);
      fw.push_back(v);
    }
    for (const auto &x : fw) {
      int y1[N], y2[N];
      if (check_fwd<N, F>(x.data(), s1, dst, y1)) return 1;
      if (check_fwd<N, F>(y1, s2, dst, y2)) return 1; // the first pass's outputs through the second pass's shift
    }
    patterns<N>(-32768, 32767, iv);
    for (int t = 0; t < 3000; t++) {
      std::vector<int> v(N);
      for (int &e : v) e = i16(rng);
      iv.push_back(v);
    }
    for (const auto &c : iv) {
      int y[N];
      if (check_inv<N, F>(c.data(), i1, dst) || check_inv<N, F>(c.data(), i2, dst)) return 1;
      if (check_fwd<N, F>(c.data(), s2, dst, y)) return 1; // any int16 vector as the second forward pass's input
    }
  }
  return 0;
}

template <int F>
static int run_forms(std::mt19937 &rng) {
  return run_size<4, F>(true, rng) || run_size<4, F>(false, rng) || run_size<8, F>(false, rng) || run_size<16, F>(false, rng) ||
         run_size<32, F>(false, rng);
}

int main() {
  // the reference matrix against literals of the standard
  fill_dct(4);
  static const int m4[4][4] = {{64, 64, 64, 64}, {83, 36, -36, -83}, {64, -64, -64, 64}, {36, -83, 83, -36}};
  for (int k = 0; k < 4; k++)
    for (int n = 0; n < 4; n++)
      if (mat[k][n] != m4[k][n]) return fail("matrix", 4, 0, 0, 4 * k + n, mat[k][n], m4[k][n]);
  fill_dct(8);
  static const int r8[2][8] = {{89, 75, 50, 18, -18, -50, -75, -89}, {75, -18, -89, -50, 50, 89, 18, -75}};
  for (int n = 0; n < 8; n++)
    if (mat[1][n] != r8[0][n] || mat[3][n] != r8[1][n]) return fail("matrix", 8, 0, 0, n, mat[1][n], r8[0][n]);
  fill_dct(16);
  static const int r16[16] = {90, 87, 80, 70, 57, 43, 25, 9, -9, -25, -43, -57, -70, -80, -87, -90};
  for (int n = 0; n < 16; n++)
    if (mat[1][n] != r16[n]) return fail("matrix", 16, 0, 0, n, mat[1][n], r16[n]);
  fill_dct(32);
  static const int r32[16] = {90, 90, 88, 85, 82, 78, 73, 67, 61, 54, 46, 38, 31, 22, 13, 4};
  for (int n = 0; n < 16; n++)
    if (mat[1][n] != r32[n] || mat[1][31 - n] != -r32[n]) return fail("matrix", 32, 0, 0, n, mat[1][n], r32[n]);
  for (int N : {4, 8, 16, 32}) { // and the header's own table against it
    fill_dct(N);
    for (int k = 0; k < N; k++)
      for (int n = 0; n < N; n++)
        if (hmx::dct_coef(N, k, n) != mat[k][n]) return fail("dct_coef", N, 0, 0, k * N + n, hmx::dct_coef(N, k, n), mat[k][n]);
  }
  std::mt19937 rng(20240607u);
  // what the kernels use, each part alone, the loops, and the packed kernels' mask (the 16-point forward pass in loops)
  if (run_forms<hmx::kTrDefault>(rng) || run_forms<hmx::kTrMadChains>(rng) || run_forms<hmx::kTrFastDst>(rng) || run_forms<0>(rng) ||
      run_forms<(hmx::kTrMadChains | hmx::kTrFastDst) & ~hmx::kTrMadFwd16>(rng))
    return 1;
  std::printf("%ld\n", n_vectors);
  return 0;
}
