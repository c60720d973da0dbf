// Stand-alone check of posfeat_amd/csrc/fundamental_solve.h and of the sampler
// and slot key ransac_plan.h gained for posfeat_ransac_fundamental, built with
// -fsanitize=address,undefined and run directly by tests/test_fundamental_host.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <set>

#include "../../posfeat_amd/csrc/fundamental_solve.h"
#include "../../posfeat_amd/csrc/ransac_plan.h"

using namespace pfransac_plan;

#define CHECK(c)                                                                            \
  do {                                                                                      \
    if (!(c)) {                                                                             \
      std::fprintf(stderr, "%s:%d: %s failed (case %s)\n", __FILE__, __LINE__, #c, g_case); \
      std::exit(1);                                                                         \
    }                                                                                       \
  } while (0)

static const char* g_case = "";

// the definition the long way round: a sorted list of the earlier draws
template <int K>
static void sample_slow(uint64_t seed, int pair, int it, int n, int32_t (&out)[K]) {
  const uint64_t base = mix(mix(seed ^ mix((uint64_t)pair)) ^ (uint64_t)it);
  std::set<int32_t> prev;
  for (int k = 0; k < K; ++k) {
    const uint64_t r = mix(base ^ (uint64_t)k);
    int32_t j = (int32_t)(((r >> 32) * (uint64_t)(n - k)) >> 32);
    for (int32_t q : prev)
      if (j >= q) ++j;
    out[k] = j;
    prev.insert(j);
  }
}

template <int K>
static void check_sampler_k() {
  const int sizes[] = {K, K + 1, 63, 64, 65, 8192, 60000, INT32_MAX};
  const uint64_t seeds[] = {0ull, 1ull, 0x123456789abcdef0ull, ~0ull};
  for (int n : sizes)
    for (uint64_t seed : seeds)
      for (int pair : {0, 99, INT32_MAX})
        for (int it = 0; it < 128; ++it) {
          int32_t a[K], b[K], c[4];
          sample_k<K>(seed, pair, it, n, a);
          sample_slow<K>(seed, pair, it, n, b);
          sample4(seed, pair, it, n, c);
          for (int k = 0; k < K; ++k) {
            CHECK(a[k] == b[k] && a[k] >= 0 && a[k] < n);
            for (int l = 0; l < k; ++l) CHECK(a[k] != a[l]);
          }
          for (int k = 0; k < 4; ++k) CHECK(a[k] == c[k]);
        }
}

static void check_keys() {
  g_case = "slot key";
  CHECK(slot_key_root(0, 0, 0) > 0ull);
  CHECK(slot_key_root(5, 9, 2) > slot_key_root(4, 0, 0));         // more inliers first
  CHECK(slot_key_root(5, 3, 2) > slot_key_root(5, 4, 0));         // then the lower iteration
  CHECK(slot_key_root(5, 3, 1) > slot_key_root(5, 3, 2));         // then the lower root
  for (int it : {0, 1, 255, 256, RMAXITERS - 1})
    for (int r = 0; r < 3; ++r) {
      const unsigned long long k = slot_key_root(INT32_MAX - 1, it, r);
      CHECK(slot_key_iter(k) == it && slot_key_rootidx(k) == r && (k >> 32) == (unsigned)INT32_MAX);
    }
}

static double urand(uint64_t& s) {
  s = mix(s);
  return (double)(s >> 11) / 9007199254740992.0;
}

// matches of a random scene under a random motion, roughly normalised
static void scene(uint64_t& s, int kind, int n, double (*m)[4]) {
  const double th = kind == 0 ? 0.2 * (urand(s) - 0.5) : 0.0;
  const double t[3] = {kind == 1 ? 0.0 : 0.5 + urand(s), kind == 1 ? 0.0 : urand(s) - 0.5,
                       kind == 2 ? 0.0 : 0.5 + urand(s)};
  for (int i = 0; i < n; ++i) {
    const double X = 4.0 * (urand(s) - 0.5), Y = 3.0 * (urand(s) - 0.5), Z = 4.0 + 5.0 * urand(s);
    const double X2 = std::cos(th) * X + std::sin(th) * Z + t[0], Y2 = Y + t[1],
                 Z2 = -std::sin(th) * X + std::cos(th) * Z + t[2];
    m[i][0] = 2.0 * X / Z, m[i][1] = 2.0 * Y / Z, m[i][2] = 2.0 * X2 / Z2, m[i][3] = 2.0 * Y2 / Z2;
  }
}

static double det3(const double* f) {
  return f[0] * (f[4] * f[8] - f[5] * f[7]) - f[1] * (f[3] * f[8] - f[5] * f[6]) +
         f[2] * (f[3] * f[7] - f[4] * f[6]);
}

static void check_solver() {
  g_case = "solve7";
  uint64_t s = 12345;
  long total = 0, rejected = 0;
  for (int trial = 0; trial < 3000; ++trial) {
    double m[7][4], F[3][9];
    scene(s, trial % 3, 7, m);
    if (trial % 50 == 49)
      for (int k = 0; k < 4; ++k) m[5][k] = m[2][k];  // a repeated match
    const int nc = pffund::solve7(m, F);
    CHECK(nc >= 0 && nc <= 3);
    if (trial % 50 == 49) CHECK(nc == 0);
    rejected += nc == 0;
    for (int r = 0; r < 3; ++r) {
      if (r >= nc) {
        CHECK(F[r][0] != F[r][0]);
        continue;
      }
      ++total;
      CHECK(pffund::unit_sign(F[r]));
      CHECK(std::fabs(det3(F[r])) <= 1e-9);
      for (int i = 0; i < 7; ++i) {
        double row[9], e = 0.0;
        pffund::epi_row(m[i][0], m[i][1], m[i][2], m[i][3], row);
        for (int k = 0; k < 9; ++k) e += row[k] * F[r][k];
        CHECK(std::fabs(e) <= 1e-8);
        CHECK(pffund::sampson_inlier(F[r], m[i][0], m[i][1], m[i][2], m[i][3], 1e-12));
      }
    }
  }
  CHECK(total >= 3000 && rejected >= 60);
  std::printf("solve7: %ld candidates, %ld samples rejected\n", total, rejected);
  // degenerate input: all zero, NaN
  double z[7][4] = {}, F[3][9];
  CHECK(pffund::solve7(z, F) == 0);
  z[3][1] = NAN;
  CHECK(pffund::solve7(z, F) == 0);
}

static void check_roots() {
  g_case = "roots";
  double lam[3];
  const double three[4] = {-6.0, 11.0, -6.0, 1.0};  // (l - 1)(l - 2)(l - 3)
  CHECK(pffund::cubic_roots(three, lam) == 3);
  CHECK(std::fabs(lam[0] - 1) < 1e-14 && std::fabs(lam[1] - 2) < 1e-14 && std::fabs(lam[2] - 3) < 1e-14);
  const double one[4] = {-2.0, 1.0, -2.0, 1.0};  // (l - 2)(l^2 + 1)
  CHECK(pffund::cubic_roots(one, lam) == 1 && std::fabs(lam[0] - 2) < 1e-14 && lam[1] > 1e300);
  const double quad[4] = {2.0, -3.0, 1.0, 1e-14};  // the cubic term dropped: (l - 1)(l - 2)
  CHECK(pffund::cubic_roots(quad, lam) == 2 && lam[0] == 1.0 && lam[1] == 2.0);
  const double noroot[4] = {1.0, 0.0, 1.0, 0.0};
  CHECK(pffund::cubic_roots(noroot, lam) == 0);
  const double lin[4] = {3.0, -2.0, 0.0, 0.0};
  CHECK(pffund::cubic_roots(lin, lam) == 1 && lam[0] == 1.5);
  const double zero[4] = {0.0, 0.0, 0.0, 0.0};
  CHECK(pffund::cubic_roots(zero, lam) == 0);
  const double bad[4] = {1.0, NAN, 0.0, 1.0};
  CHECK(pffund::cubic_roots(bad, lam) == 0);
}

static void check_refit() {
  g_case = "refit";
  uint64_t s = 777;
  for (int trial = 0; trial < 60; ++trial) {
    double m[40][4], nmat[9][9] = {}, Fn[9];
    scene(s, trial % 3, 40, m);
    for (int i = 0; i < 40; ++i) {
      double row[9];
      pffund::epi_row(m[i][0], m[i][1], m[i][2], m[i][3], row);
      for (int r = 0; r < 9; ++r)
        for (int c = r; c < 9; ++c) nmat[r][c] += row[r] * row[c];
    }
    pffund::refit_from_normal(nmat, Fn);
    CHECK(pffund::unit_sign(Fn));
    CHECK(std::fabs(det3(Fn)) <= 1e-12);
    for (int i = 0; i < 40; ++i)
      CHECK(pffund::sampson_inlier(Fn, m[i][0], m[i][1], m[i][2], m[i][3], 1e-16));
  }
  double zero[9] = {};
  CHECK(!pffund::unit_sign(zero));
}

int main() {
  g_case = "sampler";
  check_sampler_k<4>();
  check_sampler_k<5>();
  check_sampler_k<7>();
  check_sampler_k<8>();
  check_keys();
  check_roots();
  check_solver();
  check_refit();
  std::printf("fundamental_solve ok\n");
  return 0;
}
