// triangulate_solve.h -- the arithmetic of posfeat_triangulate (triangulate.hip)
// that the host and the kernels share: the camera model (undistortion,
// projection, the inlier test), the DLT on the 4x4 normal matrix with the
// cyclic Jacobi of fundamental_solve.h, the triangulation-angle test, the
// hypothesis enumeration and the validation of the set table.  Plain C++
// behind PFR_HD with no HIP call: posfeat_triangulate_dlt and
// tests/host/triangulate_check.cpp compile the same text as the kernels.  The
// definitions are stated in include/posfeat_hip.h.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fundamental_solve.h"
#include "ransac_plan.h"

#pragma clang fp contract(off)

namespace pftri {

constexpr int NEWTON_STEPS = 8;     // of the undistortion
constexpr double W_REL = 1e-12;     // |v4| / max |vi| at or below this: a point at infinity
constexpr int MIN_ITERS = 8, MAX_ITERS = 1024;
constexpr int MIN_TRACK = 2, MAX_TRACK = 1024;

// (x, y) in pixels -> the undistorted normalised point, cam = (fx, fy, cx, cy,
// k1, ...)
PFR_HD inline void undistort(const double* cam, double x, double y, double& xu, double& yu) {
  const double xd = (x - cam[2]) / cam[0], yd = (y - cam[3]) / cam[1], k1 = cam[4];
  const double rd = hypot(xd, yd);
  xu = xd, yu = yd;
  if (k1 == 0.0 || rd == 0.0) return;
  double ru = rd;
  for (int s = 0; s < NEWTON_STEPS; ++s) {
    const double g = ru * (1.0 + k1 * (ru * ru)) - rd;
    const double d = 1.0 + 3.0 * k1 * (ru * ru);
    if (d > 0.0 && pffund::finite_d(d)) ru = ru - g / d;
  }
  const double sc = ru / rd;
  xu = sc * xd, yu = sc * yd;
}

// depth of X in the view P = [R | t] (row-major 3x4)
PFR_HD inline double depth(const double* P, const double (&X)[3]) {
  return ((P[8] * X[0] + P[9] * X[1]) + P[10] * X[2]) + P[11];
}

// the squared reprojection error of X against the pixel (x, y); z = the depth
PFR_HD inline double reproj2(const double* cam, const double* P, const double (&X)[3], double x,
                             double y, double& z) {
  const double xc = ((P[0] * X[0] + P[1] * X[1]) + P[2] * X[2]) + P[3];
  const double yc = ((P[4] * X[0] + P[5] * X[1]) + P[6] * X[2]) + P[7];
  z = depth(P, X);
  const double xn = xc / z, yn = yc / z;
  const double f = 1.0 + cam[4] * (xn * xn + yn * yn);
  const double dx = (cam[0] * f * xn + cam[2]) - x, dy = (cam[1] * f * yn + cam[3]) - y;
  return dx * dx + dy * dy;
}

PFR_HD inline bool inlier_of(double e2, double z, double thr2) {
  return z > 0.0 && e2 <= thr2 && pffund::finite_d(e2);
}

// C = -R^T t
PFR_HD inline void centre(const double* P, double (&C)[3]) {
#pragma unroll
  for (int c = 0; c < 3; ++c) C[c] = -((P[c] * P[3] + P[4 + c] * P[7]) + P[8 + c] * P[11]);
}

// the angle at X between X - Ci and X - Cj is at least the minimum: cos <
// cosmin, a zero-length ray (or a NaN) failing
PFR_HD inline bool angle_ok(const double (&X)[3], const double (&Ci)[3], const double (&Cj)[3],
                            double cosmin) {
  double a[3], b[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) a[c] = X[c] - Ci[c], b[c] = X[c] - Cj[c];
  const double d = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
  const double na = sqrt((a[0] * a[0] + a[1] * a[1]) + a[2] * a[2]);
  const double nb = sqrt((b[0] * b[0] + b[1] * b[1]) + b[2] * b[2]);
  return na > 0.0 && nb > 0.0 && d / (na * nb) < cosmin;
}

PFR_HD inline void dlt_zero(double (&n)[4][4]) {
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) n[r][c] = 0.0;
}

// N += a a^T + b b^T (upper triangle), a = xu P3 - P1, b = yu P3 - P2
PFR_HD inline void dlt_add(double (&n)[4][4], double xu, double yu, const double* P) {
  double a[4], b[4];
#pragma unroll
  for (int c = 0; c < 4; ++c) a[c] = xu * P[8 + c] - P[c], b[c] = yu * P[8 + c] - P[4 + c];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = r; c < 4; ++c) n[r][c] = (n[r][c] + a[r] * a[c]) + b[r] * b[c];
}

// X from the normal matrix (destroyed): the eigenvector of its lowest diagonal
// entry after the Jacobi; false for a rejected system (X untouched)
PFR_HD inline bool dlt_solve(double (&n)[4][4], double (&X)[3]) {
  double v[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) v[r][c] = r == c ? 1.0 : 0.0;
  pffund::jacobi_sym<4, 4>(n, v);
  const int jm = pffund::min_diag<4>(n);
  double e[4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
    e[r] = jm == 0 ? v[r][0] : (jm == 1 ? v[r][1] : (jm == 2 ? v[r][2] : v[r][3]));
  const double big = fmax(fmax(fabs(e[0]), fabs(e[1])), fmax(fabs(e[2]), fabs(e[3])));
  const double x = e[0] / e[3], y = e[1] / e[3], z = e[2] / e[3];
  const bool ok = fabs(e[3]) > W_REL * big && pffund::finite_d(big) &&
                  pffund::finite_d(e[0] + e[1] + e[2] + e[3]) && pffund::finite_d(x) &&
                  pffund::finite_d(y) && pffund::finite_d(z);
  if (ok) X[0] = x, X[1] = y, X[2] = z;
  return ok;
}

// the h-th pair (i < j) of 0..m-1 in lexicographic order, h < m (m - 1) / 2
PFR_HD inline void pair_of(int h, int m, int& i, int& j) {
  int a = 0, rem = h;
  while (rem >= m - 1 - a) rem -= m - 1 - a, ++a;
  i = a, j = a + 1 + rem;
}

// the member pair of hypothesis h of a track of m members with root row `root`
PFR_HD inline void hyp_pair(uint64_t seed, int root, int h, int m, int iters, int& i, int& j) {
  const long long H = (long long)m * (m - 1) / 2;
  if (H <= iters) {
    pair_of(h, m, i, j);
  } else {
    int32_t d[4];
    pfransac_plan::sample4(seed, root, h, m, d);
    i = d[0], j = d[1];
  }
}

PFR_HD inline int num_hyp(int m, int iters) {
  const long long H = (long long)m * (m - 1) / 2;
  return H <= iters ? (int)H : iters;
}

// 0, or -1 for a bad table: null, nsets < 0, set_off[0] != 0 or a decreasing set_off
inline int check_sets(const int32_t* set_off, int nsets) {
  if (!set_off || nsets < 0 || set_off[0] != 0) return -1;
  for (int s = 0; s < nsets; ++s)
    if (set_off[s + 1] < set_off[s]) return -1;
  return 0;
}

// Workspace (byte offsets, each 256-B aligned), N = set_off[nsets] rows:
//   set table   (nsets + 1) int32 (uploaded per call)
//   setid       N int32: the set of a row
//   parent      N int32: the union-find forest, after the flatten launch the root
//   size        N int32: at a root, the rows of its component
//   tid         N int32: at a root of a track, its id, else -1
//   cursor      N int32: at a root, the members filled so far
//   und         N x 2 fp64: the undistorted normalised point of a row
//   bsum        max(1, ceil(N / SCAN_ROWS)) uint64: the scan's block sums
constexpr int SCAN_ROWS = 2048;  // rows per workgroup of the scan launches
struct Layout {
  long long n = 0, nblk = 0, tmax = 0, mmax = 0;
  size_t set_off = 0, setid = 0, parent = 0, size = 0, tid = 0, cursor = 0, und = 0, bsum = 0,
         total = 0;
};
inline size_t al256(size_t x) { return (x + 255) / 256 * 256; }
inline long long max_tracks(long long n, long long nedges) {
  return nedges < n / 2 ? nedges : n / 2;
}
inline long long max_members(long long n, long long nedges) {
  return 2 * nedges < n ? 2 * nedges : n;
}
inline int layout(const int32_t* set_off, int nsets, long long nedges, Layout& L) {
  L = Layout();
  if (check_sets(set_off, nsets) != 0 || nedges < 0) return -1;
  const long long n = set_off[nsets];
  L.n = n, L.nblk = n > 0 ? (n + SCAN_ROWS - 1) / SCAN_ROWS : 1;
  L.tmax = max_tracks(n, nedges), L.mmax = max_members(n, nedges);
  size_t at = 0;
  L.set_off = at, at += al256((size_t)(nsets + 1) * 4);
  L.setid = at, at += al256((size_t)n * 4);
  L.parent = at, at += al256((size_t)n * 4);
  L.size = at, at += al256((size_t)n * 4);
  L.tid = at, at += al256((size_t)n * 4);
  L.cursor = at, at += al256((size_t)n * 4);
  L.und = at, at += al256((size_t)n * 16);
  L.bsum = at, at += al256((size_t)L.nblk * 8);
  L.total = at + 256;
  return 0;
}

}  // namespace pftri
