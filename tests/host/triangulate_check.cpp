// Stand-alone check of posfeat_amd/csrc/triangulate_solve.h (camera model, DLT,
// angle test, hypothesis enumeration, set-table validation and workspace
// layout), built with -fsanitize=address,undefined and run directly by
// tests/test_triangulate_host.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../posfeat_amd/csrc/triangulate_solve.h"

using namespace pftri;

#define CHECK(c)                                                                            \
  do {                                                                                      \
    if (!(c)) {                                                                             \
      std::fprintf(stderr, "%s:%d: %s failed (case %s)\n", __FILE__, __LINE__, #c, g_case); \
      std::exit(1);                                                                         \
    }                                                                                       \
  } while (0)

static const char* g_case = "";

static uint64_t g_state = 12345;
static double uni(double lo, double hi) {
  g_state = pfransac_plan::mix(g_state);
  return lo + (hi - lo) * (double)(g_state >> 11) / 9007199254740992.0;
}

// camera i of a line: K = 500 / 320 / 240, centre (0.45 i, 0, 0), a small yaw
static void line_camera(int i, double* cam, double* P) {
  const double yaw = (i % 2 ? 2.0 : -2.0) * 3.14159265358979323846 / 180.0;
  const double c = std::cos(yaw), s = std::sin(yaw);
  const double R[9] = {c, 0, s, 0, 1, 0, -s, 0, c};
  const double C[3] = {0.45 * i, 0.0, 0.0};
  for (int r = 0; r < 3; ++r) {
    for (int k = 0; k < 3; ++k) P[4 * r + k] = R[3 * r + k];
    P[4 * r + 3] = -(R[3 * r] * C[0] + R[3 * r + 1] * C[1] + R[3 * r + 2] * C[2]);
  }
  cam[0] = cam[1] = 500.0, cam[2] = 320.0, cam[3] = 240.0;
  cam[4] = i % 2 ? -0.06 : 0.0, cam[5] = cam[6] = cam[7] = 0.0;
}

// the pixel of X (the forward model of the header)
static void pixel_of(const double* cam, const double* P, const double (&X)[3], double& x,
                     double& y) {
  const double xc = P[0] * X[0] + P[1] * X[1] + P[2] * X[2] + P[3];
  const double yc = P[4] * X[0] + P[5] * X[1] + P[6] * X[2] + P[7];
  const double z = P[8] * X[0] + P[9] * X[1] + P[10] * X[2] + P[11];
  const double xn = xc / z, yn = yc / z, f = 1.0 + cam[4] * (xn * xn + yn * yn);
  x = cam[0] * f * xn + cam[2], y = cam[1] * f * yn + cam[3];
}

static void check_camera() {
  g_case = "undistort / project round trip";
  for (double k1 : {0.0, -0.06, 0.05}) {
    double cam[8], P[12];
    line_camera(1, cam, P);
    cam[4] = k1;
    for (int it = 0; it < 2000; ++it) {
      const double x = uni(0, 640), y = uni(0, 480);
      double xu, yu;
      undistort(cam, x, y, xu, yu);
      // a point on the ray of (xu, yu) at depth d reprojects onto (x, y)
      const double d = uni(3, 9);
      const double xc[3] = {xu * d - P[3], yu * d - P[7], d - P[11]};
      double X[3];
      for (int c = 0; c < 3; ++c) X[c] = P[c] * xc[0] + P[4 + c] * xc[1] + P[8 + c] * xc[2];
      double z;
      const double e2 = reproj2(cam, P, X, x, y, z);
      CHECK(std::fabs(z - d) < 1e-12 * d);
      CHECK(std::sqrt(e2) < 1e-9);  // pixels (1e-12 in normalised coordinates x f = 500)
      CHECK(inlier_of(e2, z, 16.0));
    }
  }
  g_case = "camera with non-finite entries";
  double cam[8], P[12], X[3] = {0.1, 0.2, 5.0}, z, xu, yu;
  line_camera(0, cam, P);
  cam[0] = NAN;
  undistort(cam, 10.0, 20.0, xu, yu);
  CHECK(!inlier_of(reproj2(cam, P, X, 10.0, 20.0, z), z, 16.0));
  line_camera(1, cam, P);
  cam[4] = INFINITY;
  undistort(cam, 10.0, 20.0, xu, yu);  // every Newton step skipped or non-finite: must return
  CHECK(!inlier_of(reproj2(cam, P, X, 10.0, 20.0, z), z, 16.0));
  P[11] = NAN;
  cam[4] = 0.0;
  CHECK(!inlier_of(reproj2(cam, P, X, 10.0, 20.0, z), z, 16.0));
}

static void check_dlt() {
  g_case = "dlt on exact observations";
  for (int it = 0; it < 500; ++it) {
    const int nv = 2 + it % 7;
    const double X[3] = {uni(0.5, 3.0), uni(-0.5, 0.5), uni(3, 9)};
    double nm[4][4];
    dlt_zero(nm);
    for (int v = 0; v < nv; ++v) {
      double cam[8], P[12], x, y, xu, yu;
      line_camera(v, cam, P);
      pixel_of(cam, P, X, x, y);
      undistort(cam, x, y, xu, yu);
      dlt_add(nm, xu, yu, P);
    }
    double Y[3] = {0, 0, 0};
    CHECK(dlt_solve(nm, Y));
    for (int c = 0; c < 3; ++c) CHECK(std::fabs(Y[c] - X[c]) < 1e-8 * 9.0);
  }
  g_case = "dlt rejects";
  {
    // two parallel rays from two centres: the point at infinity
    double cam[8], P0[12], P1[12], nm[4][4], Y[3] = {7, 7, 7};
    line_camera(0, cam, P0);
    line_camera(2, cam, P1);  // the same yaw
    dlt_zero(nm);
    dlt_add(nm, 0.1, -0.05, P0);
    dlt_add(nm, 0.1, -0.05, P1);
    CHECK(!dlt_solve(nm, Y) && Y[0] == 7 && Y[1] == 7 && Y[2] == 7);
    dlt_zero(nm);  // no observation at all
    CHECK(!dlt_solve(nm, Y));
    dlt_zero(nm);
    dlt_add(nm, NAN, 0.0, P0);
    dlt_add(nm, 0.1, 0.0, P1);
    CHECK(!dlt_solve(nm, Y));
  }
  g_case = "angle";
  {
    const double X[3] = {0, 0, 5}, A[3] = {0, 0, 0}, B[3] = {0.45, 0, 0}, Cn[3] = {0.002, 0, 0};
    const double cosmin = std::cos(1.5 * 3.14159265358979323846 / 180.0);
    CHECK(angle_ok(X, A, B, cosmin));
    CHECK(!angle_ok(X, A, Cn, cosmin));
    CHECK(!angle_ok(X, A, A, cosmin));  // one image: the same ray
    CHECK(!angle_ok(X, X, B, cosmin));  // a zero-length ray
    CHECK(!angle_ok(X, A, A, 1.0));     // min_angle = 0 still rejects the same ray
    const double N[3] = {NAN, 0, 0};
    CHECK(!angle_ok(X, A, N, cosmin));
    double cam[8], P[12], C[3];
    line_camera(3, cam, P);
    centre(P, C);
    CHECK(std::fabs(C[0] - 1.35) < 1e-15 && std::fabs(C[1]) < 1e-15 && std::fabs(C[2]) < 1e-15);
  }
}

static void check_pairs() {
  g_case = "hypothesis enumeration";
  for (int m = 2; m <= 46; ++m) {
    int h = 0;
    for (int i = 0; i < m; ++i)
      for (int j = i + 1; j < m; ++j, ++h) {
        int a, b;
        pair_of(h, m, a, b);
        CHECK(a == i && b == j);
      }
    CHECK(h == m * (m - 1) / 2);
  }
  for (int m : {2, 4, 5, 6, 11, 12, 64, 1024})
    for (int iters : {8, 64, 1024}) {
      const long long H = (long long)m * (m - 1) / 2;
      CHECK(num_hyp(m, iters) == (H <= iters ? (int)H : iters));
      for (int h = 0; h < num_hyp(m, iters); ++h) {
        int i, j;
        hyp_pair(99, 1234, h, m, iters, i, j);
        CHECK(i >= 0 && j >= 0 && i < m && j < m && i != j);
        if (H <= iters) CHECK(i < j);
        if (H > iters) {
          int32_t d[4];
          pfransac_plan::sample4(99, 1234, h, m, d);
          CHECK(i == d[0] && j == d[1]);
        }
      }
    }
}

static void check_tables() {
  g_case = "set table and layout";
  const int32_t good[] = {0, 300, 300, 2349, 2400};
  const int32_t dec[] = {0, 300, 299, 2349, 2400};
  const int32_t off[] = {1, 300, 300, 2349, 2400};
  const int32_t neg[] = {-1, 300, 300, 2349, 2400};
  const int32_t empty[] = {0};
  CHECK(check_sets(good, 4) == 0 && check_sets(empty, 0) == 0);
  CHECK(check_sets(nullptr, 4) != 0 && check_sets(good, -1) != 0 && check_sets(dec, 4) != 0 &&
        check_sets(off, 4) != 0 && check_sets(neg, 4) != 0);
  Layout L;
  CHECK(layout(good, 4, -1, L) != 0 && layout(dec, 4, 10, L) != 0);
  CHECK(layout(good, 4, 1000, L) == 0);
  CHECK(L.n == 2400 && L.nblk == 2 && L.tmax == 1000 && L.mmax == 2000);
  const size_t at[] = {L.set_off, L.setid, L.parent, L.size, L.tid, L.cursor, L.und, L.bsum, L.total};
  const size_t need[] = {5 * 4, 2400 * 4, 2400 * 4, 2400 * 4, 2400 * 4, 2400 * 4, 2400 * 16, 2 * 8};
  for (int k = 0; k < 8; ++k) CHECK(at[k] % 256 == 0 && at[k + 1] >= at[k] + need[k]);
  CHECK(layout(good, 4, 1 << 20, L) == 0 && L.tmax == 1200 && L.mmax == 2400);
  CHECK(layout(empty, 0, 0, L) == 0 && L.n == 0 && L.nblk == 1 && L.tmax == 0 && L.total >= 256);
  const int32_t big[] = {0, INT32_MAX};
  CHECK(layout(big, 1, 1ll << 40, L) == 0 && L.tmax == INT32_MAX / 2 && L.mmax == INT32_MAX);
  CHECK(L.total > (size_t)INT32_MAX * 36);
}

int main() {
  check_camera();
  check_dlt();
  check_pairs();
  check_tables();
  std::printf("triangulate_solve ok\n");
  return 0;
}
