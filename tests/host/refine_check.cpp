// Stand-alone check of posfeat_amd/csrc/refine_solve.h (one observation's normal
// equations against finite differences, the damped solve, the
// Levenberg-Marquardt round, the two summation orders, the parameter check and
// the workspace layout), built with -fsanitize=address,undefined and run
// directly by tests/test_refine_host.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../posfeat_amd/csrc/refine_solve.h"

using namespace pfrefine;

#define CHECK(c)                                                                            \
  do {                                                                                      \
    if (!(c)) {                                                                             \
      std::fprintf(stderr, "%s:%d: %s failed (case %s)\n", __FILE__, __LINE__, #c, g_case); \
      std::exit(1);                                                                         \
    }                                                                                       \
  } while (0)

static const char* g_case = "";

static uint64_t g_state = 4242;
static double uni(double lo, double hi) {
  g_state = pfransac_plan::mix(g_state);
  return lo + (hi - lo) * (double)(g_state >> 11) / 9007199254740992.0;
}

// a camera at distance d from the origin on a ring, looking at the origin
static void ring_camera(int i, double d, double f, double* cam, double* P) {
  const double a = 0.35 * i + 0.1, b = 0.2 * std::sin(1.7 * i);
  const double C[3] = {d * std::sin(a) * std::cos(b), d * std::sin(b), -d * std::cos(a) * std::cos(b)};
  double z[3] = {-C[0] / d, -C[1] / d, -C[2] / d};
  double x[3] = {z[2], 0.0, -z[0]};  // up x z, up = (0, 1, 0)
  const double nx = std::sqrt(x[0] * x[0] + x[2] * x[2]);
  x[0] /= nx, x[2] /= nx;
  const double y[3] = {z[1] * x[2] - z[2] * x[1], z[2] * x[0] - z[0] * x[2], z[0] * x[1] - z[1] * x[0]};
  const double* R[3] = {x, y, z};
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) P[4 * r + k] = R[r][k];
    P[4 * r + 3] = -(R[r][0] * C[0] + R[r][1] * C[1] + R[r][2] * C[2]);
  }
  cam[0] = cam[1] = f, cam[2] = 0.8 * f, cam[3] = 0.6 * f;
  cam[4] = i % 2 ? -0.05 : 0.0, cam[5] = cam[6] = cam[7] = 0.0;
}

static void pixel_of(const double* cam, const double* P, const double (&X)[3], double& x,
                     double& y) {
  double z;
  // reproj2 against the pixel (0, 0) would square; project by hand
  const double xc = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3];
  const double yc = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7];
  z = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
  const double xn = xc / z, yn = yc / z, f = 1.0 + cam[4] * (xn * xn + yn * yn);
  x = cam[0] * f * xn + cam[2], y = cam[1] * f * yn + cam[3];
}

// n observations of X as [n][22] rows, with `noise` px of uniform noise
static std::vector<double> system_of(int n, const double (&X)[3], double noise) {
  std::vector<double> obs(22 * (size_t)n);
  for (int i = 0; i < n; ++i) {
    double* o = obs.data() + 22 * (size_t)i;
    ring_camera(i, std::exp(uni(std::log(2.0), std::log(40.0))),
                std::exp(uni(std::log(400.0), std::log(1600.0))), o + 2, o + 10);
    pixel_of(o + 2, o + 10, X, o[0], o[1]);
    o[0] += uni(-noise, noise), o[1] += uni(-noise, noise);
  }
  return obs;
}

static void check_row() {
  g_case = "normal equations of one row against finite differences";
  for (int it = 0; it < 200; ++it) {
    const double X[3] = {uni(-0.3, 0.3), uni(-0.3, 0.3), uni(-0.3, 0.3)};
    std::vector<double> obs = system_of(1, X, 0.0);
    double* o = obs.data();
    o[0] += 3.0, o[1] -= 2.0;  // a residual of (-3, 2)
    double acc[ACC];
    acc_zero(acc);
    CHECK(acc_row(o + 2, o + 10, o[0], o[1], X, acc));
    CHECK(std::fabs(acc[9] - 13.0) < 1e-8);
    // g = J^T r = half the gradient of the cost
    for (int c = 0; c < 3; ++c) {
      const double h = 1e-6;
      double Xp[3] = {X[0], X[1], X[2]}, Xm[3] = {X[0], X[1], X[2]}, zp, zm;
      Xp[c] += h, Xm[c] -= h;
      const double cp = pftri::reproj2(o + 2, o + 10, Xp, o[0], o[1], zp);
      const double cm = pftri::reproj2(o + 2, o + 10, Xm, o[0], o[1], zm);
      const double num = (cp - cm) / (4.0 * h);
      CHECK(std::fabs(num - acc[6 + c]) <= 1e-5 * (std::fabs(acc[6 + c]) + std::sqrt(acc[0] + acc[3] + acc[5])));
    }
    CHECK(acc[0] >= 0.0 && acc[3] >= 0.0 && acc[5] >= 0.0);
    CHECK(acc[1] * acc[1] <= acc[0] * acc[3] * (1.0 + 1e-12));  // N is a Gram matrix
  }
  g_case = "rows that are not usable";
  {
    const double X[3] = {0.0, 0.0, 0.0};
    std::vector<double> obs = system_of(1, X, 0.0);
    double* o = obs.data();
    double acc[ACC];
    acc_zero(acc);
    const double behind[3] = {-100.0 * o[18], -100.0 * o[19], -100.0 * o[20]};  // far along -z of the camera
    CHECK(!acc_row(o + 2, o + 10, o[0], o[1], behind, acc));
    const double bad[3] = {NAN, 0.0, 0.0};
    acc_zero(acc);
    CHECK(!acc_row(o + 2, o + 10, o[0], o[1], bad, acc));
    o[2] = INFINITY;
    acc_zero(acc);
    CHECK(!acc_row(o + 2, o + 10, o[0], o[1], X, acc));
  }
}

static void check_solve() {
  g_case = "damped solve";
  double acc[ACC] = {4.0, 1.0, 0.5, 3.0, 0.25, 2.0, -1.0, 2.0, 0.5, 0.0}, d[3];
  CHECK(lm_solve(acc, 0.0, d));
  const double N[3][3] = {{4.0, 1.0, 0.5}, {1.0, 3.0, 0.25}, {0.5, 0.25, 2.0}};
  for (int r = 0; r < 3; ++r)
    CHECK(std::fabs(N[r][0] * d[0] + N[r][1] * d[1] + N[r][2] * d[2] + acc[6 + r]) < 1e-14);
  double d1[3];
  CHECK(lm_solve(acc, 1e8, d1));  // a steepest-descent step scaled by the diagonal
  CHECK(std::fabs(d1[0]) < std::fabs(d[0]) && std::fabs(d1[1]) < 1e-7);
  double zero[ACC] = {0, 0, 0, 0, 0, 0, 1, 1, 1, 0};
  CHECK(!lm_solve(zero, 1e-4, d));
  double rank1[ACC] = {1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 1.0, 0.0};
  CHECK(!lm_solve(rank1, 0.0, d));
  CHECK(lm_solve(rank1, 1.0, d));  // the damping makes it regular
  double nan[ACC] = {NAN, 0, 0, 1, 0, 1, 1, 1, 1, 0};
  CHECK(!lm_solve(nan, 1e-4, d));
}

static void check_round() {
  g_case = "round on exact and noisy systems, both summation orders";
  for (int it = 0; it < 120; ++it) {
    const int n = it % 3 == 2 ? 17 + it % 50 : 2 + it % 7;  // a lane's and a wave's order
    const double noise = it % 2 ? 1.0 : 0.0;
    const double X[3] = {uni(-0.3, 0.3), uni(-0.3, 0.3), uni(-0.3, 0.3)};
    std::vector<double> obs = system_of(n, X, noise);
    double Y[3] = {X[0] + uni(-0.05, 0.05), X[1] + uni(-0.05, 0.05), X[2] + uni(-0.05, 0.05)};
    double acc0[ACC], cost = 0.0;
    CHECK(accumulate_rows(obs.data(), n, Y, acc0));
    const int steps = 1 + it % MAX_STEPS;
    const int taken = lm_round(
        Y, steps, [&](const double (&Z)[3], double (&a)[ACC]) { return accumulate_rows(obs.data(), n, Z, a); },
        cost);
    CHECK(taken >= 0 && taken <= steps && cost <= acc0[9] && cost >= 0.0);
    if (noise == 0.0 && steps >= 8)
      for (int c = 0; c < 3; ++c) CHECK(std::fabs(Y[c] - X[c]) < 1e-8);
    // the two orders agree up to rounding
    if (n > LANE_TRACK) {
      double a[ACC], b[ACC];
      accumulate_rows(obs.data(), n, Y, a);
      acc_zero(b);
      for (int k = 0; k < n; ++k) {
        const double* o = obs.data() + 22 * (size_t)k;
        acc_row(o + 2, o + 10, o[0], o[1], Y, b);
      }
      for (int i = 0; i < 6; ++i) CHECK(std::fabs(a[i] - b[i]) <= 1e-12 * std::fabs(b[i]));
    }
  }
  g_case = "round from an unusable start";
  {
    const double X[3] = {0.0, 0.0, 0.0};
    std::vector<double> obs = system_of(3, X, 0.0);
    double Y[3] = {NAN, 0.0, 0.0}, cost = 0.0;
    const int taken = lm_round(
        Y, 10, [&](const double (&Z)[3], double (&a)[ACC]) { return accumulate_rows(obs.data(), 3, Z, a); },
        cost);
    CHECK(taken == 0 && std::isnan(cost) && std::isnan(Y[0]) && Y[1] == 0.0);
  }
  g_case = "round on two copies of one row: every solve singular or refused";
  {
    const double X[3] = {0.1, 0.0, 0.0};
    std::vector<double> one = system_of(1, X, 0.0), obs(44);
    for (int i = 0; i < 44; ++i) obs[i] = one[i % 22];
    double Y[3] = {0.1, 0.01, 0.0}, cost = 0.0;
    const int taken = lm_round(
        Y, 32, [&](const double (&Z)[3], double (&a)[ACC]) { return accumulate_rows(obs.data(), 2, Z, a); },
        cost);
    CHECK(taken >= 0 && taken <= 32 && std::isfinite(cost));  // must return
  }
}

static void check_plan() {
  g_case = "parameters and layout";
  CHECK(params_ok(4.0, 1.5, 3, 10) && params_ok(1e-3, 0.0, 1, 1) && params_ok(100.0, 89.9, 8, 32));
  CHECK(!params_ok(0.0, 1.5, 3, 10) && !params_ok(-1.0, 1.5, 3, 10) && !params_ok(NAN, 1.5, 3, 10) &&
        !params_ok(INFINITY, 1.5, 3, 10));
  CHECK(!params_ok(4.0, -0.1, 3, 10) && !params_ok(4.0, 90.0, 3, 10) && !params_ok(4.0, NAN, 3, 10));
  CHECK(!params_ok(4.0, 1.5, 0, 10) && !params_ok(4.0, 1.5, 9, 10) && !params_ok(4.0, 1.5, 3, 0) &&
        !params_ok(4.0, 1.5, 3, 33));
  const int32_t good[] = {0, 300, 300, 2349, 2400};
  const int32_t dec[] = {0, 300, 299, 2349, 2400};
  const int32_t empty[] = {0};
  Layout L;
  CHECK(layout(good, 4, 1000, 2000, L) == 0 && L.n == 2400);
  CHECK(L.set_off % 256 == 0 && L.setid % 256 == 0 && L.setid >= L.set_off + 5 * 4 &&
        L.total >= L.setid + 2400 * 4);
  CHECK(layout(dec, 4, 1000, 2000, L) != 0 && layout(nullptr, 4, 1000, 2000, L) != 0 &&
        layout(good, -1, 1000, 2000, L) != 0);
  CHECK(layout(good, 4, -1, 2000, L) != 0 && layout(good, 4, 1000, -1, L) != 0);
  CHECK(layout(good, 4, (long long)INT32_MAX, 2000, L) != 0 &&
        layout(good, 4, 1000, (long long)INT32_MAX + 1, L) != 0);
  CHECK(layout(empty, 0, 0, 0, L) == 0 && L.n == 0 && L.total >= 256);
}

int main() {
  check_row();
  check_solve();
  check_round();
  check_plan();
  std::printf("refine_solve ok\n");
  return 0;
}
