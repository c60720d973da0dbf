// pose_solve.h -- the arithmetic of posfeat_ransac_pose (pose.hip) that the host
// and the kernels share: the P3P minimal solve (Grunert's quartic, its real
// roots in closed form by Ferrari through the cubic of fundamental_solve.h, the
// poses from the depths), the division-free reprojection inlier test, the
// pieces of the Gauss-Newton refit (a row's normal equations, the 6x6 solve,
// the update by Rodrigues' formula, the step control) and the plan (table
// check, workspace layout).  The camera model is triangulate_solve.h's.  Plain
// C++ behind PFR_HD with no HIP call: posfeat_pose_solve3 and
// tests/host/pose_solve_check.cpp compile the same text as the kernels.  The
// definitions are stated in include/posfeat_hip.h; every array is indexed by
// compile-time constants once the loops are unrolled.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "fundamental_solve.h"
#include "ransac_plan.h"
#include "triangulate_solve.h"

#pragma clang fp contract(off)

namespace pfpose {

using pffund::finite_d;

constexpr int MIN_CORR = 4;              // correspondences a query needs (the sampler draws from n >= 4)
constexpr double COLLINEAR_REL = 1e-6;   // |d12 x d13| <= this |d12| |d13|: rejected
constexpr double BEARING_COS = 1.0 - 1e-12;  // two bearings with a cosine >= this: rejected
constexpr double LEAD_REL = 1e-12;       // |A4| <= this max |Ak|: the cubic
constexpr int QUARTIC_NEWTON = 2;        // steps on each closed-form root
constexpr double ROOT_GAP = 1e-9;        // roots closer than this max(1, |v|) count once
constexpr int GN_STEPS = 10;             // of the refit, at the most
constexpr int GN_MIN_INLIERS = 4;        // the refit is attempted from this many
constexpr double GN_PIVOT_REL = 1e-12;   // pivot / largest entry of its column below this: stop
constexpr double GN_STOP = 1e-12;        // max |delta| at or below this: converged
constexpr int GN_ACC = 29;               // 21 of N (upper triangle, row-major), 6 of g, cost, bad rows

// ---- the quartic ----------------------------------------------------------

PFR_HD inline void sort4(double (&v)[4]) {
  double t;
#define PFPOSE_CS(i, j) \
  if (v[j] < v[i]) t = v[i], v[i] = v[j], v[j] = t
  PFPOSE_CS(0, 1);
  PFPOSE_CS(2, 3);
  PFPOSE_CS(0, 2);
  PFPOSE_CS(1, 3);
  PFPOSE_CS(1, 2);
#undef PFPOSE_CS
}

// The real roots of A[0] + A[1] v + ... + A[4] v^4, ascending in v[0..count);
// the unused entries are +inf.  With cm the largest |A[k]|:
// |A[4]| > LEAD_REL cm: for |A[0]| > |A[4]| the coefficients are reversed first
// (the quartic in 1 / v, whose roots are inverted at the end; a root 0 of it is
// no root).  Monic v^4 + a v^3 + b v^2 + c v + d, depressed by v = y
// - a / 4 to y^4 + p y^2 + q y + r (p = b - 3 a^2 / 8, q = c - a b / 2 + a^3 /
// 8, r = d - a c / 4 + a^2 b / 16 - 3 a^4 / 256).  m = the largest real root of
// the resolvent 8 m^3 + 8 p m^2 + (2 p^2 - 8 r) m - q^2 (pffund::cubic_roots).
// For m > 0, with s = sqrt(2 m), h = p / 2 + m, w = q / (2 s), the quartic
// factors into y^2 + s y + (h - w) and y^2 - s y + (h + w); each with a
// discriminant >= 0 gives the two roots t and C / t, t = -(B + sign(B)
// sqrt(disc)) / 2 (B = +-s, C its constant).  Otherwise (q = 0 up to rounding)
// the biquadratic: z = y^2 solves z^2 + p z + r the same way, and every z >= 0
// gives y = +-sqrt(z).  Else the cubic A[0..3] by pffund::cubic_roots (which
// drops to the quadratic and the linear case itself).  Every root then takes
// QUARTIC_NEWTON Newton steps on the quartic as given (a step with a zero
// derivative or a non-finite result is skipped); the roots are sorted, and a
// root within ROOT_GAP max(1, |v|) of the last root kept is dropped.  No root
// when a coefficient is not finite or all are 0.
PFR_HD inline int quartic_roots(const double (&A)[5], double (&v)[4]) {
  const double inf = (double)INFINITY;
  v[0] = v[1] = v[2] = v[3] = inf;
  const double cm =
      fmax(fmax(fmax(fabs(A[0]), fabs(A[1])), fmax(fabs(A[2]), fabs(A[3]))), fabs(A[4]));
  if (!(cm > 0.0) || !finite_d(A[0] + A[1] + A[2] + A[3] + A[4]) || !finite_d(cm)) return 0;
  if (fabs(A[4]) > LEAD_REL * cm) {
    // the end of larger magnitude leads: for |A[0]| > |A[4]| the reversed
    // quartic in 1 / v is solved, so a root far out does not swamp the others
    const bool rev = fabs(A[0]) > fabs(A[4]);
    const double l = rev ? A[0] : A[4];
    const double a = (rev ? A[1] : A[3]) / l, b = A[2] / l, c = (rev ? A[3] : A[1]) / l,
                 d = (rev ? A[4] : A[0]) / l;
    const double a2 = a * a, a4 = 0.25 * a;
    const double p = b - 0.375 * a2;
    const double q = (c - 0.5 * (a * b)) + 0.125 * (a2 * a);
    const double r = ((d - 0.25 * (a * c)) + 0.0625 * (a2 * b)) - (3.0 / 256.0) * (a2 * a2);
    const double co[4] = {-(q * q), 2.0 * (p * p) - 8.0 * r, 8.0 * p, 8.0};
    double lam[3];
    const int nc = pffund::cubic_roots(co, lam);
    const double m = nc == 3 ? lam[2] : (nc == 2 ? lam[1] : lam[0]);
    if (m > 0.0 && finite_d(m)) {
      const double s = sqrt(2.0 * m), h = 0.5 * p + m, w = q / (2.0 * s);
      const double c1 = h - w, c2 = h + w;
      const double d1 = s * s - 4.0 * c1, d2 = s * s - 4.0 * c2;
      if (d1 >= 0.0) {
        const double t = -0.5 * (s + sqrt(d1));  // s > 0: never 0
        v[0] = t - a4, v[1] = c1 / t - a4;
      }
      if (d2 >= 0.0) {
        const double t = 0.5 * (s + sqrt(d2));
        v[2] = t - a4, v[3] = c2 / t - a4;
      }
    } else {
      const double disc = p * p - 4.0 * r;
      if (disc >= 0.0) {
        const double sd = sqrt(disc);
        const double t = -0.5 * (p + (p >= 0.0 ? sd : -sd));
        const double z1 = t, z2 = t != 0.0 ? r / t : 0.0;
        if (z1 >= 0.0) v[0] = sqrt(z1) - a4, v[1] = -sqrt(z1) - a4;
        if (z2 >= 0.0) v[2] = sqrt(z2) - a4, v[3] = -sqrt(z2) - a4;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const double w = 1.0 / v[i];  // 1 / 0 and 1 / inf: no root
      v[i] = rev ? ((v[i] < inf && finite_d(w)) ? w : inf) : v[i];
    }
  } else {
    const double co[4] = {A[0], A[1], A[2], A[3]};
    double lam[3];
    pffund::cubic_roots(co, lam);
    v[0] = lam[0], v[1] = lam[1], v[2] = lam[2];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    double x = v[i];
    const bool have = x < inf && x > -inf;
#pragma unroll
    for (int k = 0; k < QUARTIC_NEWTON; ++k) {
      const double f = (((A[4] * x + A[3]) * x + A[2]) * x + A[1]) * x + A[0];
      const double df = ((4.0 * A[4] * x + 3.0 * A[3]) * x + 2.0 * A[2]) * x + A[1];
      const double xn = x - f / df;
      x = (df != 0.0 && finite_d(xn)) ? xn : x;
    }
    v[i] = have ? x : inf;
  }
  sort4(v);
  double last = v[0];
#pragma unroll
  for (int i = 1; i < 4; ++i) {
    const bool dup = v[i] < inf && v[i] - last <= ROOT_GAP * fmax(1.0, fabs(v[i]));
    last = dup ? last : v[i];
    v[i] = dup ? inf : v[i];
  }
  sort4(v);
  int nr = 0;
#pragma unroll
  for (int i = 0; i < 4; ++i) nr += v[i] < inf ? 1 : 0;
  return nr;
}

// ---- P3P --------------------------------------------------------------------

PFR_HD inline double dot3(const double (&a)[3], const double (&b)[3]) {
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}
PFR_HD inline void cross3(const double (&a)[3], const double (&b)[3], double (&c)[3]) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// the orthonormal triad of the points A, B, C: e1 = (B - A) normalised, e3 = e1
// x (C - A) normalised, e2 = e3 x e1
PFR_HD inline void triad(const double (&A)[3], const double (&B)[3], const double (&C)[3],
                         double (&e)[3][3]) {
  double d1[3], d2[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) d1[c] = B[c] - A[c], d2[c] = C[c] - A[c];
  const double n1 = sqrt(dot3(d1, d1));
#pragma unroll
  for (int c = 0; c < 3; ++c) e[0][c] = d1[c] / n1;
  double x[3];
  cross3(e[0], d2, x);
  const double n3 = sqrt(dot3(x, x));
#pragma unroll
  for (int c = 0; c < 3; ++c) e[2][c] = x[c] / n3;
  cross3(e[2], e[0], e[1]);
}

// The candidate poses of three correspondences m[i] = (xu, yu, X, Y, Z): the
// undistorted normalised image point and the world point.  Returns their
// number (0 for a rejected sample), in ascending root order; the rows of pose
// past it are NaN.
PFR_HD inline int p3p(const double (&m)[3][5], double (&pose)[4][12]) {
#pragma unroll
  for (int k = 0; k < 4; ++k)
#pragma unroll
    for (int j = 0; j < 12; ++j) pose[k][j] = (double)NAN;
  double f[3][3], P[3][3], sum = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double n = sqrt((m[i][0] * m[i][0] + m[i][1] * m[i][1]) + 1.0);
    f[i][0] = m[i][0] / n, f[i][1] = m[i][1] / n, f[i][2] = 1.0 / n;
    P[i][0] = m[i][2], P[i][1] = m[i][3], P[i][2] = m[i][4];
#pragma unroll
    for (int c = 0; c < 5; ++c) sum = sum + m[i][c];
  }
  bool ok = finite_d(sum);
  double d12[3], d13[3], d23[3], cr[3];
#pragma unroll
  for (int c = 0; c < 3; ++c)
    d12[c] = P[1][c] - P[0][c], d13[c] = P[2][c] - P[0][c], d23[c] = P[2][c] - P[1][c];
  const double c2 = dot3(d12, d12), b2 = dot3(d13, d13), a2 = dot3(d23, d23);
  cross3(d12, d13, cr);
  ok = ok && sqrt(dot3(cr, cr)) > COLLINEAR_REL * (sqrt(c2) * sqrt(b2));
  const double ca = dot3(f[1], f[2]), cb = dot3(f[0], f[2]), cg = dot3(f[0], f[1]);
  ok = ok && ca < BEARING_COS && cb < BEARING_COS && cg < BEARING_COS;
  const double k = (a2 - c2) / b2, mm = (a2 + c2) / b2;
  const double ab = a2 / b2, cbr = c2 / b2;
  double A[5], v[4];
  A[4] = (k - 1.0) * (k - 1.0) - 4.0 * cbr * (ca * ca);
  A[3] = 4.0 * ((k * (1.0 - k) * cb - (1.0 - mm) * (ca * cg)) + 2.0 * cbr * ((ca * ca) * cb));
  A[2] = 2.0 * (((((k * k - 1.0) + 2.0 * (k * k) * (cb * cb)) + 2.0 * ((b2 - c2) / b2) * (ca * ca)) -
                 4.0 * mm * ((ca * cb) * cg)) +
                2.0 * ((b2 - a2) / b2) * (cg * cg));
  A[1] = 4.0 * ((-(k * (1.0 + k)) * cb + 2.0 * ab * ((cg * cg) * cb)) - (1.0 - mm) * (ca * cg));
  A[0] = (1.0 + k) * (1.0 + k) - 4.0 * ab * (cg * cg);
  quartic_roots(A, v);
  double ew[3][3];
  triad(P[0], P[1], P[2], ew);
  int cnt = 0;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const double vv = v[r];
    const double u = (((k - 1.0) * (vv * vv) - 2.0 * k * cb * vv) + 1.0 + k) / (2.0 * (cg - vv * ca));
    const double s1 = sqrt(b2 / ((1.0 + vv * vv) - 2.0 * vv * cb));
    const double s2 = u * s1, s3 = vv * s1;
    double Q[3][3], ec[3][3], cand[12];
#pragma unroll
    for (int c = 0; c < 3; ++c) Q[0][c] = s1 * f[0][c], Q[1][c] = s2 * f[1][c], Q[2][c] = s3 * f[2][c];
    triad(Q[0], Q[1], Q[2], ec);
    double tot = 0.0;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j)
        cand[4 * i + j] = (ec[0][i] * ew[0][j] + ec[1][i] * ew[1][j]) + ec[2][i] * ew[2][j];
      cand[4 * i + 3] = Q[0][i] - ((cand[4 * i] * P[0][0] + cand[4 * i + 1] * P[0][1]) +
                                   cand[4 * i + 2] * P[0][2]);
#pragma unroll
      for (int j = 0; j < 4; ++j) tot = tot + cand[4 * i + j];
    }
    const bool good = ok && vv < (double)INFINITY && vv > 0.0 && u > 0.0 && finite_d(u) &&
                      s1 > 0.0 && finite_d(s1) && finite_d(tot);
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) {
      const bool here = good && cnt == kk;
#pragma unroll
      for (int j = 0; j < 12; ++j) pose[kk][j] = here ? cand[j] : pose[kk][j];
    }
    cnt += good ? 1 : 0;
  }
  return cnt;
}

// ---- score --------------------------------------------------------------------

// z > 0 and the squared pixel reprojection error finite and <= thr2, without
// the division: with (xc, yc, z) = R X + t, g = z^2 + k1 (xc^2 + yc^2) and (xd,
// yd) = ((x - cx) / fx, (y - cy) / fy), the error times z^3 is (fx (xc g - xd
// z^3), fy (yc g - yd z^3)).  A NaN anywhere fails every test.
PFR_HD inline bool reproj_inlier(double fx, double fy, double k1, const double (&P)[12], double xd,
                                 double yd, double X, double Y, double Z, double thr2) {
  const double xc = __builtin_fma(P[0], X, __builtin_fma(P[1], Y, __builtin_fma(P[2], Z, P[3])));
  const double yc = __builtin_fma(P[4], X, __builtin_fma(P[5], Y, __builtin_fma(P[6], Z, P[7])));
  const double z = __builtin_fma(P[8], X, __builtin_fma(P[9], Y, __builtin_fma(P[10], Z, P[11])));
  const double z2 = z * z, z3 = z2 * z;
  const double g = __builtin_fma(k1, __builtin_fma(xc, xc, yc * yc), z2);
  const double ex = fx * __builtin_fma(xc, g, -(xd * z3));
  const double ey = fy * __builtin_fma(yc, g, -(yd * z3));
  const double lim = thr2 * (z3 * z3);
  return z > 0.0 && __builtin_fma(ex, ex, ey * ey) <= lim && lim < (double)INFINITY;
}

// ---- the Gauss-Newton refit -------------------------------------------------

PFR_HD inline void gn_zero(double (&acc)[GN_ACC]) {
#pragma unroll
  for (int i = 0; i < GN_ACC; ++i) acc[i] = 0.0;
}

// The pixel reprojection residual (pftri's forward model) of the camera point
// (xc, yc, z) against the pixel (x, y), and its derivative by the camera point:
// r = pixel(Xc) - (x, y), jx = d r_x / d Xc, jy = d r_y / d Xc (d pixel / d (xn,
// yn), then d (xn, yn) / d Xc).  The pose refit below and the point refinement
// (refine_solve.h) compile this one text.
PFR_HD inline void pixel_jac(const double* cam, double xc, double yc, double z, double x, double y,
                             double& rx, double& ry, double (&jx)[3], double (&jy)[3]) {
  const double xn = xc / z, yn = yc / z, k1 = cam[4];
  const double f = 1.0 + k1 * (xn * xn + yn * yn);
  rx = (cam[0] * f * xn + cam[2]) - x, ry = (cam[1] * f * yn + cam[3]) - y;
  const double axx = cam[0] * (f + 2.0 * k1 * (xn * xn)), axy = cam[0] * (2.0 * k1 * (xn * yn));
  const double ayx = cam[1] * (2.0 * k1 * (xn * yn)), ayy = cam[1] * (f + 2.0 * k1 * (yn * yn));
  const double iz = 1.0 / z;
  jx[0] = axx * iz, jx[1] = axy * iz, jx[2] = -(axx * xn + axy * yn) * iz;
  jy[0] = ayx * iz, jy[1] = ayy * iz, jy[2] = -(ayx * xn + ayy * yn) * iz;
}

// One inlier's share of the normal equations of the pixel reprojection error
// (pftri's forward model) at the pose P: the residual r = pixel(P X) - (x, y),
// its Jacobian J (2 x 6) against delta = (omega, tau) perturbing the camera
// point as Xc + omega x Xc + tau; acc += (J^T J upper triangle row-major, J^T
// r, r . r, 1 if the depth is not positive or the residual not finite).
PFR_HD inline void gn_row(const double* cam, const double (&P)[12], double x, double y, double X,
                          double Y, double Z, double (&acc)[GN_ACC]) {
  const double xc = ((P[0] * X + P[1] * Y) + P[2] * Z) + P[3];
  const double yc = ((P[4] * X + P[5] * Y) + P[6] * Z) + P[7];
  const double z = ((P[8] * X + P[9] * Y) + P[10] * Z) + P[11];
  double rx, ry, jx[3], jy[3];
  pixel_jac(cam, xc, yc, z, x, y, rx, ry, jx, jy);
  // d Xc / d omega = -[Xc]x, d Xc / d tau = I
  double a[6], b[6];
  a[0] = jx[2] * yc - jx[1] * z, a[1] = jx[0] * z - jx[2] * xc, a[2] = jx[1] * xc - jx[0] * yc;
  b[0] = jy[2] * yc - jy[1] * z, b[1] = jy[0] * z - jy[2] * xc, b[2] = jy[1] * xc - jy[0] * yc;
#pragma unroll
  for (int c = 0; c < 3; ++c) a[3 + c] = jx[c], b[3 + c] = jy[c];
  int k = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c, ++k) acc[k] = (acc[k] + a[r] * a[c]) + b[r] * b[c];
#pragma unroll
  for (int r = 0; r < 6; ++r) acc[21 + r] = (acc[21 + r] + a[r] * rx) + b[r] * ry;
  const double e2 = rx * rx + ry * ry;
  acc[27] = acc[27] + e2;
  acc[28] = acc[28] + ((z > 0.0 && finite_d(e2)) ? 0.0 : 1.0);
}

// a[.][0..D) delta = a[.][D] (destroyed) by Gaussian elimination with partial
// pivoting (the first largest entry of the column); false when a pivot is below
// GN_PIVOT_REL times the largest entry of its column of the matrix as given, or
// is not a positive number, or delta is not finite.  The pose refit (D = 6) and
// the point refinement (D = 3, refine_solve.h) compile this one text.
template <int D>
PFR_HD inline bool pivot_solve(double (&a)[D][D + 1], double (&delta)[D]) {
  double cmax[D];
#pragma unroll
  for (int c = 0; c < D; ++c) {
    cmax[c] = fabs(a[0][c]);
#pragma unroll
    for (int r = 1; r < D; ++r) cmax[c] = fmax(cmax[c], fabs(a[r][c]));
  }
  bool ok = true;
#pragma unroll
  for (int c = 0; c < D; ++c) {
    int piv = c;
    double best = fabs(a[c][c]);
#pragma unroll
    for (int r = c + 1; r < D; ++r) {
      const double v = fabs(a[r][c]);
      if (v > best) best = v, piv = r;
    }
#pragma unroll
    for (int r = c + 1; r < D; ++r) {
      const bool sw = piv == r;
#pragma unroll
      for (int j = c; j < D + 1; ++j) {
        const double t = a[c][j], u = a[r][j];
        a[c][j] = sw ? u : t;
        a[r][j] = sw ? t : u;
      }
    }
    ok = ok && best >= GN_PIVOT_REL * cmax[c] && best > 0.0;
#pragma unroll
    for (int r = c + 1; r < D; ++r) {
      const double f = a[r][c] / a[c][c];
#pragma unroll
      for (int j = c + 1; j < D + 1; ++j) a[r][j] = a[r][j] - f * a[c][j];
    }
  }
#pragma unroll
  for (int c = D - 1; c >= 0; --c) {
    double s = a[c][D];
#pragma unroll
    for (int j = c + 1; j < D; ++j) s = s - a[c][j] * delta[j];
    delta[c] = s / a[c][c];
  }
  double tot = 0.0;
#pragma unroll
  for (int c = 0; c < D; ++c) tot = tot + delta[c];
  return ok && finite_d(tot);
}

// N delta = -g by pivot_solve; false when a pivot is below GN_PIVOT_REL times
// the largest entry of its column of N as given, or is not a positive number
PFR_HD inline bool gn_solve(const double (&acc)[GN_ACC], double (&delta)[6]) {
  double a[6][7];
  int k = 0;
#pragma unroll
  for (int r = 0; r < 6; ++r)
#pragma unroll
    for (int c = r; c < 6; ++c, ++k) a[r][c] = acc[k], a[c][r] = acc[k];
#pragma unroll
  for (int r = 0; r < 6; ++r) a[r][6] = -acc[21 + r];
  return pivot_solve<6>(a, delta);
}

// Q = [exp(omega) R | exp(omega) t + tau] with exp by Rodrigues' formula: theta =
// |omega|, exp = I + A K + B K^2, K = [omega]x, A = sin(theta) / theta, B = 2
// sin^2(theta / 2) / theta^2 (A = 1, B = 1 / 2 for theta = 0)
PFR_HD inline void gn_update(const double (&P)[12], const double (&d)[6], double (&Q)[12]) {
  const double th2 = (d[0] * d[0] + d[1] * d[1]) + d[2] * d[2], th = sqrt(th2);
  const double sh = sin(0.5 * th);
  const double A = th > 0.0 ? sin(th) / th : 1.0, B = th > 0.0 ? 2.0 * (sh * sh) / th2 : 0.5;
  const double K[3][3] = {{0.0, -d[2], d[1]}, {d[2], 0.0, -d[0]}, {-d[1], d[0], 0.0}};
  double E[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double kk = (K[i][0] * K[0][j] + K[i][1] * K[1][j]) + K[i][2] * K[2][j];
      E[i][j] = ((i == j ? 1.0 : 0.0) + A * K[i][j]) + B * kk;
    }
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      Q[4 * i + j] = (E[i][0] * P[j] + E[i][1] * P[4 + j]) + E[i][2] * P[8 + j];
    Q[4 * i + 3] = Q[4 * i + 3] + d[3 + i];
  }
}

// The refit's step control.  accumulate(P, acc) fills acc with the sums of
// gn_row over the fixed inlier set at the pose P (every caller of one refit
// must get the same bits).  From the winner's pose: solve, update, accept the
// step iff no row of the set has a non-positive depth or a non-finite residual
// at the new pose and the cost decreased; at most GN_STEPS steps, stopping at a
// refused step, a refused solve or max |delta| <= GN_STOP.  P ends as the last
// accepted pose; returns the number of accepted steps.
template <class Acc>
PFR_HD inline int gn_refit(double (&P)[12], Acc&& accumulate, double* last_acc = nullptr) {
  double acc[GN_ACC];
  accumulate(P, acc);
  int taken = 0;
  for (int step = 0; step < GN_STEPS; ++step) {
    double delta[6], Q[12], acc1[GN_ACC];
    if (!gn_solve(acc, delta)) break;
    gn_update(P, delta, Q);
    accumulate(Q, acc1);
    if (!(acc1[28] == 0.0 && acc1[27] < acc[27])) break;
#pragma unroll
    for (int i = 0; i < 12; ++i) P[i] = Q[i];
#pragma unroll
    for (int i = 0; i < GN_ACC; ++i) acc[i] = acc1[i];
    ++taken;
    double big = 0.0;
#pragma unroll
    for (int i = 0; i < 6; ++i) big = fmax(big, fabs(delta[i]));
    if (big <= GN_STOP) break;
  }
  if (last_acc)
    for (int i = 0; i < GN_ACC; ++i) last_acc[i] = acc[i];
  return taken;
}

// ---- the plan -------------------------------------------------------------------

// 0, or -1 for a bad table: null, nq < 0, q_off[0] != 0, a decreasing q_off
// (its last entry, the number of correspondences, is an int32 by type)
inline int check_queries(const int32_t* q_off, int nq) {
  if (!q_off || nq < 0 || q_off[0] != 0) return -1;
  for (int q = 0; q < nq; ++q)
    if (q_off[q + 1] < q_off[q]) return -1;
  return 0;
}

// Workspace (byte offsets, each 256-B aligned), C = q_off[nq] correspondences:
//   table   (nq + 1) int32 (uploaded per call)
//   rows    C x 8 fp64: x y (the pixel), xu yu (undistorted), X Y Z, 0; a
//           correspondence out of range or not finite is eight NaNs
//   slots   nq x nblk uint64: per (query, hypothesis block) the packed
//           (count, iteration, root) key of the block's best
constexpr int ROW_DOUBLES = 8;
struct Layout {
  long long c = 0;
  int nblk = 0;
  size_t table = 0, rows = 0, slots = 0, total = 0;
};
inline int layout(const int32_t* q_off, int nq, int iters, Layout& L) {
  L = Layout();
  if (check_queries(q_off, nq) != 0) return -1;
  if (iters < 1 || iters > pfransac_plan::RMAXITERS) return -1;
  L.c = q_off[nq];
  L.nblk = (iters + pfransac_plan::RBLOCK - 1) / pfransac_plan::RBLOCK;
  if ((long long)nq * L.nblk > INT32_MAX) return -1;
  size_t at = 0;
  L.table = at, at += pftri::al256((size_t)(nq + 1) * 4);
  L.rows = at, at += pftri::al256((size_t)L.c * ROW_DOUBLES * 8);
  L.slots = at, at += pftri::al256((size_t)nq * L.nblk * 8);
  L.total = at + 256;
  return 0;
}

}  // namespace pfpose
