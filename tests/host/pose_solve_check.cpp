// Stand-alone check of posfeat_amd/csrc/pose_solve.h (the quartic's roots, the
// P3P candidates and rejections, the reprojection test, the Gauss-Newton refit
// on a planted pose, the query-table validation and workspace layout), built
// with -fsanitize=address,undefined and run directly by tests/test_pose_host.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../posfeat_amd/csrc/pose_solve.h"

using namespace pfpose;

#define CHECK(c)                                                                            \
  do {                                                                                      \
    if (!(c)) {                                                                             \
      std::fprintf(stderr, "%s:%d: %s failed (case %s)\n", __FILE__, __LINE__, #c, g_case); \
      std::exit(1);                                                                         \
    }                                                                                       \
  } while (0)

static const char* g_case = "";

static uint64_t g_state = 4321;
static double uni(double lo, double hi) {
  g_state = pfransac_plan::mix(g_state);
  return lo + (hi - lo) * (double)(g_state >> 11) / 9007199254740992.0;
}

// a rotation from a random unit quaternion and a centre in [-1, 1]^3
static void random_pose(double (&P)[12]) {
  double q[4], n = 0.0;
  for (double& v : q) v = uni(-1.0, 1.0), n += v * v;
  n = std::sqrt(n);
  const double w = q[0] / n, x = q[1] / n, y = q[2] / n, z = q[3] / n;
  const double R[9] = {1 - 2 * (y * y + z * z), 2 * (x * y - w * z),     2 * (x * z + w * y),
                       2 * (x * y + w * z),     1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                       2 * (x * z - w * y),     2 * (y * z + w * x),     1 - 2 * (x * x + y * y)};
  const double C[3] = {uni(-1, 1), uni(-1, 1), uni(-1, 1)};
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) P[4 * r + k] = R[3 * r + k];
    P[4 * r + 3] = -(R[3 * r] * C[0] + R[3 * r + 1] * C[1] + R[3 * r + 2] * C[2]);
  }
}

// a point at (xn, yn) x depth in the camera of P, in world coordinates
static void world_of(const double (&P)[12], double xn, double yn, double d, double (&X)[3]) {
  const double c[3] = {xn * d - P[3], yn * d - P[7], d - P[11]};
  for (int k = 0; k < 3; ++k) X[k] = P[k] * c[0] + P[4 + k] * c[1] + P[8 + k] * c[2];
}

static double pose_diff(const double* a, const double* b) {
  double d = 0.0;
  for (int i = 0; i < 12; ++i) d = std::fmax(d, std::fabs(a[i] - b[i]));
  return d;
}

static void check_quartic() {
  g_case = "quartic roots";
  // (v - 1)(v - 2)(v - 3)(v - 4), both ways round, and scaled
  const double A[5] = {24.0, -50.0, 35.0, -10.0, 1.0};
  double v[4];
  CHECK(quartic_roots(A, v) == 4);
  for (int i = 0; i < 4; ++i) CHECK(std::fabs(v[i] - (i + 1)) < 1e-12);
  const double B[5] = {1e-3, -10e-3, 35e-3, -50e-3, 24e-3};  // roots 1/4 .. 1
  CHECK(quartic_roots(B, v) == 4 && std::fabs(v[0] - 0.25) < 1e-13 && std::fabs(v[3] - 1.0) < 1e-13);
  // (v^2 + 1)(v - 2)(v + 3): two real roots
  const double C[5] = {-6.0, 1.0, -5.0, 1.0, 1.0};
  CHECK(quartic_roots(C, v) == 2 && std::fabs(v[0] + 3.0) < 1e-13 && std::fabs(v[1] - 2.0) < 1e-13);
  CHECK(v[2] == (double)INFINITY && v[3] == (double)INFINITY);
  // biquadratic (q = 0): v^4 - 5 v^2 + 4
  const double D[5] = {4.0, 0.0, -5.0, 0.0, 1.0};
  CHECK(quartic_roots(D, v) == 4 && std::fabs(v[0] + 2.0) < 1e-13 && std::fabs(v[3] - 2.0) < 1e-13);
  // no real root, a double root counted once, the cubic fallback, bad input
  const double E[5] = {4.0, 0.0, 5.0, 0.0, 1.0};
  CHECK(quartic_roots(E, v) == 0);
  const double F[5] = {4.0, -12.0, 13.0, -6.0, 1.0};  // (v - 1)^2 (v - 2)^2
  const int nf = quartic_roots(F, v);
  CHECK(nf >= 0 && nf <= 4);
  const double G[5] = {-6.0, 11.0, -6.0, 1.0, 1e-14};  // (v - 1)(v - 2)(v - 3)
  CHECK(quartic_roots(G, v) == 3 && std::fabs(v[0] - 1.0) < 1e-9 && std::fabs(v[2] - 3.0) < 1e-9);
  const double Z[5] = {0, 0, 0, 0, 0}, Nn[5] = {1.0, (double)NAN, 0, 0, 1.0};
  CHECK(quartic_roots(Z, v) == 0 && quartic_roots(Nn, v) == 0);
  // random quartics with planted real roots
  for (int it = 0; it < 2000; ++it) {
    double r[4];
    for (double& x : r) x = uni(-3.0, 3.0);
    const double s = uni(0.5, 2.0);
    const double e1 = r[0] + r[1] + r[2] + r[3];
    const double e2 = r[0] * r[1] + r[0] * r[2] + r[0] * r[3] + r[1] * r[2] + r[1] * r[3] + r[2] * r[3];
    const double e3 = r[0] * r[1] * r[2] + r[0] * r[1] * r[3] + r[0] * r[2] * r[3] + r[1] * r[2] * r[3];
    const double e4 = r[0] * r[1] * r[2] * r[3];
    const double Q[5] = {s * e4, -s * e3, s * e2, -s * e1, s};
    double gap = 10.0;
    for (int i = 0; i < 4; ++i)
      for (int j = 0; j < i; ++j) gap = std::fmin(gap, std::fabs(r[i] - r[j]));
    if (gap < 1e-3) continue;
    CHECK(quartic_roots(Q, v) == 4);
    for (int i = 0; i < 4; ++i) {
      double best = 10.0;
      for (int j = 0; j < 4; ++j) best = std::fmin(best, std::fabs(v[i] - r[j]));
      CHECK(best < 1e-7);
      if (i) CHECK(v[i] > v[i - 1]);
    }
  }
}

static void check_p3p() {
  g_case = "p3p on planted poses";
  int found = 0, total = 0;
  for (int it = 0; it < 4000; ++it) {
    double P[12], m[3][5], pose[4][12];
    random_pose(P);
    for (int i = 0; i < 3; ++i) {
      double X[3];
      m[i][0] = uni(-0.6, 0.6), m[i][1] = uni(-0.45, 0.45);
      world_of(P, m[i][0], m[i][1], uni(3.0, 9.0), X);
      m[i][2] = X[0], m[i][3] = X[1], m[i][4] = X[2];
    }
    const int nc = p3p(m, pose);
    CHECK(nc >= 1 && nc <= 4);
    double best = 1e9;
    for (int c = 0; c < 4; ++c) {
      if (c >= nc) {
        for (int i = 0; i < 12; ++i) CHECK(pose[c][i] != pose[c][i]);  // NaN past the count
        continue;
      }
      for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
          double d = 0.0;
          for (int k = 0; k < 3; ++k) d += pose[c][4 * k + i] * pose[c][4 * k + j];
          CHECK(std::fabs(d - (i == j ? 1.0 : 0.0)) <= 1e-12);
        }
      best = std::fmin(best, pose_diff(pose[c], P));
    }
    ++total;
    found += best <= 1e-6 ? 1 : 0;
  }
  CHECK(found >= total * 0.995);

  g_case = "p3p rejections";
  double P[12], pose[4][12];
  random_pose(P);
  double m[3][5];
  for (int i = 0; i < 3; ++i) {
    double X[3];
    m[i][0] = -0.3 + 0.3 * i, m[i][1] = 0.1 * i * i;
    world_of(P, m[i][0], m[i][1], 4.0 + i, X);
    m[i][2] = X[0], m[i][3] = X[1], m[i][4] = X[2];
  }
  CHECK(p3p(m, pose) >= 1);
  double bad[3][5];
  auto reset = [&] {
    for (int i = 0; i < 3; ++i)
      for (int k = 0; k < 5; ++k) bad[i][k] = m[i][k];
  };
  reset();  // collinear world points
  for (int k = 2; k < 5; ++k) bad[2][k] = bad[0][k] + 2.5 * (bad[1][k] - bad[0][k]);
  CHECK(p3p(bad, pose) == 0);
  for (int i = 0; i < 12; ++i) CHECK(pose[0][i] != pose[0][i]);
  reset();  // coincident bearings
  bad[1][0] = bad[0][0], bad[1][1] = bad[0][1];
  CHECK(p3p(bad, pose) == 0);
  reset();  // one world point twice
  for (int k = 2; k < 5; ++k) bad[1][k] = bad[0][k];
  CHECK(p3p(bad, pose) == 0);
  reset();
  bad[2][3] = (double)NAN;
  CHECK(p3p(bad, pose) == 0);
  reset();
  bad[0][0] = (double)INFINITY;
  CHECK(p3p(bad, pose) == 0);
}

static void check_score_and_refit() {
  g_case = "reprojection test and Gauss-Newton refit";
  for (double k1 : {0.0, -0.06}) {
    const double cam[8] = {500.0, 510.0, 320.0, 240.0, k1, 0, 0, 0};
    double P[12];
    random_pose(P);
    const int n = 60;
    std::vector<double> px(2 * n), X(3 * n);
    for (int i = 0; i < n; ++i) {
      double W[3], z;
      const double xn = uni(-0.6, 0.6), yn = uni(-0.45, 0.45);
      world_of(P, xn, yn, uni(3.0, 9.0), W);
      const double f = 1.0 + k1 * (xn * xn + yn * yn);
      px[2 * i] = cam[0] * f * xn + cam[2], px[2 * i + 1] = cam[1] * f * yn + cam[3];
      for (int k = 0; k < 3; ++k) X[3 * i + k] = W[k];
      // the division-free test agrees with pftri::reproj2 away from the threshold
      for (double off : {0.0, 2.9, 3.1, 40.0}) {
        const double e2 = pftri::reproj2(cam, P, W, px[2 * i] + off, px[2 * i + 1], z);
        const bool want = pftri::inlier_of(e2, z, 9.0);
        const bool got = reproj_inlier(cam[0], cam[1], cam[4], P, (px[2 * i] + off - cam[2]) / cam[0],
                                       (px[2 * i + 1] - cam[3]) / cam[1], W[0], W[1], W[2], 9.0);
        CHECK(got == want && want == (off < 3.0));
      }
      CHECK(!reproj_inlier(cam[0], cam[1], cam[4], P, (double)NAN, 0.0, W[0], W[1], W[2], 9.0));
      CHECK(!reproj_inlier(cam[0], cam[1], cam[4], P, 0.0, 0.0, (double)NAN, W[1], W[2], 9.0));
    }
    auto accumulate = [&](const double (&Q)[12], double (&acc)[GN_ACC]) {
      gn_zero(acc);
      for (int i = 0; i < n; ++i)
        gn_row(cam, Q, px[2 * i], px[2 * i + 1], X[3 * i], X[3 * i + 1], X[3 * i + 2], acc);
    };
    // from a pose 0.02 rad and 0.05 units off: back onto the planted pose
    const double d0[6] = {0.02, -0.015, 0.01, 0.05, -0.03, 0.04};
    double Q[12], acc[GN_ACC];
    gn_update(P, d0, Q);
    for (int i = 0; i < 3; ++i)
      for (int j = 0; j < 3; ++j) {
        double d = 0.0;
        for (int k = 0; k < 3; ++k) d += Q[4 * k + i] * Q[4 * k + j];
        CHECK(std::fabs(d - (i == j ? 1.0 : 0.0)) <= 1e-14);  // Rodrigues keeps R a rotation
      }
    CHECK(pose_diff(Q, P) > 1e-2);
    const int steps = gn_refit(Q, accumulate, acc);
    CHECK(steps >= 2 && steps <= GN_STEPS);
    CHECK(pose_diff(Q, P) < 1e-9 && acc[27] < 1e-12 && acc[28] == 0.0);
    // at the minimum nothing moves: the first step is refused or tiny
    double Q2[12];
    for (int i = 0; i < 12; ++i) Q2[i] = Q[i];
    gn_refit(Q2, accumulate);
    CHECK(pose_diff(Q2, Q) < 1e-9);
    // a singular system (every row the same point) stops the refit where it is
    auto degenerate = [&](const double (&R)[12], double (&a)[GN_ACC]) {
      gn_zero(a);
      for (int i = 0; i < 5; ++i) gn_row(cam, R, px[0] + 1.0, px[1], X[0], X[1], X[2], a);
    };
    double Q3[12];
    for (int i = 0; i < 12; ++i) Q3[i] = P[i];
    CHECK(gn_refit(Q3, degenerate) == 0 && pose_diff(Q3, P) == 0.0);
    double delta[6];
    gn_zero(acc);
    CHECK(!gn_solve(acc, delta));
  }
}

static void check_tables() {
  g_case = "query table and layout";
  const int32_t good[] = {0, 300, 300, 1000, 1004};
  const int32_t dec[] = {0, 300, 299, 1000, 1004};
  const int32_t off[] = {1, 300, 300, 1000, 1004};
  const int32_t neg[] = {-1, 300, 300, 1000, 1004};
  const int32_t empty[] = {0};
  CHECK(check_queries(good, 4) == 0 && check_queries(empty, 0) == 0);
  CHECK(check_queries(nullptr, 4) != 0 && check_queries(good, -1) != 0 &&
        check_queries(dec, 4) != 0 && check_queries(off, 4) != 0 && check_queries(neg, 4) != 0);
  Layout L;
  CHECK(layout(good, 4, 0, L) != 0 && layout(good, 4, 65537, L) != 0 && layout(dec, 4, 8, L) != 0);
  CHECK(layout(good, 4, 512, L) == 0 && L.c == 1004 && L.nblk == 2);
  const size_t at[] = {L.table, L.rows, L.slots, L.total};
  const size_t need[] = {5 * 4, 1004 * 64, 4 * 2 * 8};
  for (int k = 0; k < 3; ++k) CHECK(at[k] % 256 == 0 && at[k + 1] >= at[k] + need[k]);
  CHECK(layout(good, 4, 1, L) == 0 && L.nblk == 1);
  CHECK(layout(good, 4, 65536, L) == 0 && L.nblk == 256);
  CHECK(layout(empty, 0, 8, L) == 0 && L.c == 0 && L.total >= 256);
  const int32_t big[] = {0, INT32_MAX};
  CHECK(layout(big, 1, 65536, L) == 0 && L.total > (size_t)INT32_MAX * 64);
}

int main() {
  check_quartic();
  check_p3p();
  check_score_and_refit();
  check_tables();
  std::printf("pose_solve ok\n");
  return 0;
}
