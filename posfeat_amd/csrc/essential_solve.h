// essential_solve.h -- the arithmetic of posfeat_ransac_essential
// (essential.hip) that the host and the kernels share: the five-point solve
// (the 5x9 elimination with full pivoting, the ten cubic constraints, the
// Gauss-Jordan step, the degree-10 polynomial, its Aberth-Ehrlich roots), the
// normalised threshold, the projection onto the essential manifold, the four
// decompositions and the closed-form depths of the cheirality test.  Plain C++
// behind PFR_HD with no HIP call: posfeat_essential_solve5,
// posfeat_essential_decompose and tests/host/essential_solve_check.cpp compile
// the same text as the kernels.  The definitions are stated in
// include/posfeat_hip.h.  Unlike fundamental_solve.h the solver indexes its
// arrays at run time (pivot rows, monomial tables): on the device it is meant
// for the solve kernel, which keeps the 10x20 system in private memory and
// hands the candidates over as records; nothing here runs in the scoring loop
// but pffund::sampson_inlier.
#pragma once
#include <math.h>
#include <stdint.h>

#include "fundamental_solve.h"
#include "triangulate_solve.h"

#pragma clang fp contract(off)

namespace pfess {

constexpr int MINSET = 5;               // the sample size; below it a pair has no model
constexpr int MAXCAND = 10;             // real roots of the degree-10 polynomial
constexpr double GJ_PIVOT_REL = 1e-12;  // Gauss-Jordan pivot / largest entry of the 10x20 matrix
constexpr double LEAD_REL = 1e-12;      // |c10| <= this max |ck|: rejected
constexpr int ABERTH_SWEEPS = 40;       // Gauss-Seidel sweeps of the root finder, always all
constexpr double ROOT_IM_TOL = 1e-8;    // a root is real iff |Im| <= this max(1, |z|)
constexpr int NEWTON_STEPS = 2;         // on each real root, on the real polynomial
constexpr int POLISH_STEPS = 3;         // Gauss-Newton steps on the ten cubics per candidate
constexpr int REFIT_MIN = 8;            // inliers the linear refit needs

using pffund::finite_d;

// (thr / f1 + thr / f2) / 2 squared, fi = (fx_i + fy_i) / 2: COLMAP's rule
PFR_HD inline double thr_norm2(const double* cam1, const double* cam2, double thr) {
  const double f1 = (cam1[0] + cam1[1]) / 2.0, f2 = (cam2[0] + cam2[1]) / 2.0;
  const double t = (thr / f1 + thr / f2) / 2.0;
  return t * t;
}

// The null space of the 5x9 system `a` (destroyed): pffund::null2's
// elimination with five pivots and four free columns.  e_j (j = 0..3) is the
// null vector with 1 at free position 5 + j and 0 at the other three, by back
// substitution; eb = MIX e with the fixed orthogonal matrix MIX = I - w w^T /
// 27, w = (-2, -4, -5, 3), whose last row is (2, 4, 5, 6) / 9, so the gauge
// vector eb[3] takes part of every free column.  False for a rejected system.
PFR_HD inline bool null4(double (&a)[5][9], double (&eb)[4][9]) {
  double amax = 0.0;
  for (int r = 0; r < 5; ++r)
    for (int c = 0; c < 9; ++c) {
      const double v = fabs(a[r][c]);
      amax = (v > amax || v != v) ? v : amax;  // a NaN sticks
    }
  int perm[9];
  for (int c = 0; c < 9; ++c) perm[c] = c;
  bool ok = true;
  for (int s = 0; s < 5; ++s) {
    int pr = s, pc = s;
    double best = fabs(a[s][s]);
    for (int r = s; r < 5; ++r)
      for (int c = s; c < 9; ++c) {
        const double v = fabs(a[r][c]);
        if (v > best) best = v, pr = r, pc = c;
      }
    for (int k = 0; k < 9; ++k) {
      const double t = a[s][k];
      a[s][k] = a[pr][k], a[pr][k] = t;
    }
    for (int r = 0; r < 5; ++r) {
      const double t = a[r][s];
      a[r][s] = a[r][pc], a[r][pc] = t;
    }
    const int t = perm[s];
    perm[s] = perm[pc], perm[pc] = t;
    ok = ok && best >= pffund::PIVOT_REL * amax && best > 0.0;
    for (int r = s + 1; r < 5; ++r) {
      const double f = a[r][s] / a[s][s];
      for (int k = s + 1; k < 9; ++k) a[r][k] = a[r][k] - f * a[s][k];
    }
  }
  double e[4][9];
  for (int j = 0; j < 4; ++j) {
    double z[9];
    for (int k = 5; k < 9; ++k) z[k] = k == 5 + j ? 1.0 : 0.0;
    for (int c = 4; c >= 0; --c) {
      double t = -a[c][5 + j];
      for (int k = c + 1; k < 5; ++k) t = t - a[c][k] * z[k];
      z[c] = t / a[c][c];
    }
    for (int k = 0; k < 9; ++k) e[j][perm[k]] = z[k];
  }
  const double mix[4][4] = {{23.0, -8.0, -10.0, 6.0},
                            {-8.0, 11.0, -20.0, 12.0},
                            {-10.0, -20.0, 2.0, 15.0},
                            {6.0, 12.0, 15.0, 18.0}};
  for (int i = 0; i < 4; ++i)
    for (int k = 0; k < 9; ++k)
      eb[i][k] = (((mix[i][0] / 27.0) * e[0][k] + (mix[i][1] / 27.0) * e[1][k]) +
                  (mix[i][2] / 27.0) * e[2][k]) +
                 (mix[i][3] / 27.0) * e[3][k];
  return ok;
}

// Polynomials in (x, y, z): a linear one is 4 coefficients over (x, y, z, 1), a
// quadratic one 10 over (x^2, xy, xz, x, y^2, yz, y, z^2, z, 1), a cubic one 20
// over (x^3, y^3, x^2 y, x y^2, x^2 z, x^2, y^2 z, y^2, xyz, xy, x z^2, xz, x,
// y z^2, yz, y, z^3, z^2, z, 1).  o = a b, summed over i then j of a[i] b[j].
PFR_HD inline void qmul(const double* a, const double* b, double (&o)[10]) {
  const int qi[4][4] = {{0, 1, 2, 3}, {1, 4, 5, 6}, {2, 5, 7, 8}, {3, 6, 8, 9}};
  for (int k = 0; k < 10; ++k) o[k] = 0.0;
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j) o[qi[i][j]] = o[qi[i][j]] + a[i] * b[j];
}
// out += s q l, summed over k then j of s (q[k] l[j])
PFR_HD inline void cacc(double* out, const double (&q)[10], const double* l, double s) {
  const int ci[10][4] = {{0, 2, 4, 5},     {2, 3, 8, 9},     {4, 8, 10, 11},   {5, 9, 11, 12},
                         {3, 1, 6, 7},     {8, 6, 13, 14},   {9, 7, 14, 15},   {10, 13, 16, 17},
                         {11, 14, 17, 18}, {12, 15, 18, 19}};
  for (int k = 0; k < 10; ++k)
    for (int j = 0; j < 4; ++j) out[ci[k][j]] = out[ci[k][j]] + s * (q[k] * l[j]);
}

// The ten cubic constraints on E = x eb[0] + y eb[1] + z eb[2] + eb[3]: row 0
// is det E (expanded along the first row), row 1 + 3 i + j the entry (i, j) of
// 2 E E^T E - tr(E E^T) E.
PFR_HD inline void constraints(const double (&eb)[4][9], double (&A)[10][20]) {
  double L[9][4];
  for (int e = 0; e < 9; ++e)
    for (int k = 0; k < 4; ++k) L[e][k] = eb[k][e];
  for (int r = 0; r < 10; ++r)
    for (int c = 0; c < 20; ++c) A[r][c] = 0.0;
  double p[10], q[10], m[10];
  const int minors[3][4] = {{4, 8, 5, 7}, {3, 8, 5, 6}, {3, 7, 4, 6}};
  for (int k = 0; k < 3; ++k) {
    qmul(L[minors[k][0]], L[minors[k][1]], p);
    qmul(L[minors[k][2]], L[minors[k][3]], q);
    for (int i = 0; i < 10; ++i) m[i] = p[i] - q[i];
    cacc(A[0], m, L[k], k == 1 ? -1.0 : 1.0);
  }
  double G[3][3][10], tr[10];
  for (int i = 0; i < 3; ++i)
    for (int j = i; j < 3; ++j) {
      double r[10];
      qmul(L[3 * i], L[3 * j], p);
      qmul(L[3 * i + 1], L[3 * j + 1], q);
      qmul(L[3 * i + 2], L[3 * j + 2], r);
      for (int k = 0; k < 10; ++k) G[i][j][k] = G[j][i][k] = (p[k] + q[k]) + r[k];
    }
  for (int k = 0; k < 10; ++k) tr[k] = (G[0][0][k] + G[1][1][k]) + G[2][2][k];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      for (int k = 0; k < 3; ++k) cacc(A[1 + 3 * i + j], G[i][k], L[3 * k + j], 2.0);
      cacc(A[1 + 3 * i + j], tr, L[3 * i + j], -1.0);
    }
}

// Gauss-Jordan on the first ten columns with partial pivoting (the first
// largest |A[r][s]|, r >= s); row s is divided by the pivot and column s
// cleared in every other row.  False when a pivot is below GJ_PIVOT_REL times
// the largest entry of A as given, or is not a positive number.
PFR_HD inline bool gauss_jordan(double (&A)[10][20]) {
  double amax = 0.0;
  for (int r = 0; r < 10; ++r)
    for (int c = 0; c < 20; ++c) {
      const double v = fabs(A[r][c]);
      amax = (v > amax || v != v) ? v : amax;
    }
  bool ok = finite_d(amax);
  for (int s = 0; s < 10; ++s) {
    int pr = s;
    double best = fabs(A[s][s]);
    for (int r = s + 1; r < 10; ++r) {
      const double v = fabs(A[r][s]);
      if (v > best) best = v, pr = r;
    }
    for (int k = 0; k < 20; ++k) {
      const double t = A[s][k];
      A[s][k] = A[pr][k], A[pr][k] = t;
    }
    ok = ok && best >= GJ_PIVOT_REL * amax && best > 0.0;
    const double piv = A[s][s];
    for (int k = s; k < 20; ++k) A[s][k] = A[s][k] / piv;
    for (int r = 0; r < 10; ++r) {
      if (r == s) continue;
      const double f = A[r][s];
      for (int k = s + 1; k < 20; ++k) A[r][k] = A[r][k] - f * A[s][k];
      A[r][s] = 0.0;
    }
  }
  return ok;
}

template <int NA, int NB>
PFR_HD inline void pmul(const double (&a)[NA], const double (&b)[NB], double (&o)[NA + NB - 1]) {
  for (int k = 0; k < NA + NB - 1; ++k) o[k] = 0.0;
  for (int i = 0; i < NA; ++i)
    for (int j = 0; j < NB; ++j) o[i + j] = o[i + j] + a[i] * b[j];
}

// The rows of the 3x3 polynomial matrix B(z) (coefficients ascending in z):
// with e..j rows 4..9 of the reduced matrix, row 0 = e - z f, row 1 = g - z h,
// row 2 = i - z j; bx is the factor of x (degree 3), by of y (3), b1 of 1 (4).
struct BMat {
  double bx[3][4], by[3][4], b1[3][5];
};
PFR_HD inline void bmatrix(const double (&A)[10][20], BMat& B) {
  for (int r = 0; r < 3; ++r) {
    const double *P = A[4 + 2 * r], *Q = A[5 + 2 * r];
    B.bx[r][0] = P[12], B.bx[r][1] = P[11] - Q[12], B.bx[r][2] = P[10] - Q[11], B.bx[r][3] = -Q[10];
    B.by[r][0] = P[15], B.by[r][1] = P[14] - Q[15], B.by[r][2] = P[13] - Q[14], B.by[r][3] = -Q[13];
    B.b1[r][0] = P[19], B.b1[r][1] = P[18] - Q[19], B.b1[r][2] = P[17] - Q[18];
    B.b1[r][3] = P[16] - Q[17], B.b1[r][4] = -Q[16];
  }
}

// det B(z) = bx0 (by1 b12 - b11 by2) - by0 (bx1 b12 - b11 bx2) + b10 (bx1 by2 -
// by1 bx2), ascending coefficients
PFR_HD inline void poly10(const BMat& B, double (&co)[11]) {
  double p[8], q[8], d[8], t0[11], t1[11], t2[11];
  pmul<4, 5>(B.by[1], B.b1[2], p);
  pmul<5, 4>(B.b1[1], B.by[2], q);
  for (int k = 0; k < 8; ++k) d[k] = p[k] - q[k];
  pmul<4, 8>(B.bx[0], d, t0);
  pmul<4, 5>(B.bx[1], B.b1[2], p);
  pmul<5, 4>(B.b1[1], B.bx[2], q);
  for (int k = 0; k < 8; ++k) d[k] = p[k] - q[k];
  pmul<4, 8>(B.by[0], d, t1);
  double p7[7], q7[7], d7[7];
  pmul<4, 4>(B.bx[1], B.by[2], p7);
  pmul<4, 4>(B.by[1], B.bx[2], q7);
  for (int k = 0; k < 7; ++k) d7[k] = p7[k] - q7[k];
  pmul<5, 7>(B.b1[0], d7, t2);
  for (int k = 0; k < 11; ++k) co[k] = (t0[k] - t1[k]) + t2[k];
}

// The real roots of co[0] + ... + co[10] z^10, ascending in zr[0..count).  No
// root when a coefficient is not finite or |co[10]| <= LEAD_REL max |co[k]|.
// Monic a = co / co[10]; r0 = max_k |a[10 - k]|^(1 / k) (1 when that is 0); the
// ten estimates start at r0 (cos t_k, sin t_k), t_k = 2 pi k / 10 + 0.7.  One
// sweep visits i = 0..9 in order, each with the estimates as they stand: p and
// p' at z_i by Horner; p = 0 leaves z_i; w = p / p', s = sum_{j != i} 1 / (z_i -
// z_j), z_i -= w / (1 - w s) when that correction is finite.  Complex products
// and quotients are the textbook formulas ((a c + b d) + (b c - a d) i) / (c^2
// + d^2).  ABERTH_SWEEPS sweeps, always all of them.  z_i is real iff |Im z_i|
// <= ROOT_IM_TOL max(1, |z_i|); its real part then takes NEWTON_STEPS Newton
// steps on the real monic polynomial (a step with a zero derivative or a
// non-finite result is skipped).
PFR_HD inline int roots10(const double (&co)[11], double (&zr)[10]) {
  double cm = 0.0, sum = 0.0;
  for (int k = 0; k < 11; ++k) cm = fmax(cm, fabs(co[k])), sum = sum + co[k];
  for (int k = 0; k < 10; ++k) zr[k] = (double)INFINITY;
  if (!(cm > 0.0) || !finite_d(cm) || !finite_d(sum) || !(fabs(co[10]) > LEAD_REL * cm)) return 0;
  double a[10];
  for (int k = 0; k < 10; ++k) a[k] = co[k] / co[10];
  double r0 = 0.0;
  for (int k = 1; k <= 10; ++k) r0 = fmax(r0, pow(fabs(a[10 - k]), 1.0 / (double)k));
  if (!(r0 > 0.0)) r0 = 1.0;
  const double start[10][2] = {{0.7648421872844885, 0.64421768723769102},
                               {0.24010867170377775, 0.9707460150691567},
                               {-0.37633819547418595, 0.92648235958772218},
                               {-0.84903666324581262, 0.52833393272097962},
                               {-0.99743198335233718, -0.071620099035276802},
                               {-0.76484218728448838, -0.64421768723769113},
                               {-0.24010867170377764, -0.97074601506915681},
                               {0.37633819547418601, -0.92648235958772218},
                               {0.84903666324581251, -0.52833393272097973},
                               {0.99743198335233729, 0.071620099035276691}};
  double zx[10], zy[10];
  for (int i = 0; i < 10; ++i) zx[i] = r0 * start[i][0], zy[i] = r0 * start[i][1];
  for (int sweep = 0; sweep < ABERTH_SWEEPS; ++sweep)
    for (int i = 0; i < 10; ++i) {
      const double x = zx[i], y = zy[i];
      double pr = 1.0, pi = 0.0, dr = 0.0, di = 0.0;
      for (int k = 9; k >= 0; --k) {
        const double ndr = (dr * x - di * y) + pr, ndi = (dr * y + di * x) + pi;
        const double npr = (pr * x - pi * y) + a[k], npi = pr * y + pi * x;
        dr = ndr, di = ndi, pr = npr, pi = npi;
      }
      if (pr == 0.0 && pi == 0.0) continue;
      const double dd = dr * dr + di * di;
      const double wr = (pr * dr + pi * di) / dd, wi = (pi * dr - pr * di) / dd;
      double sr = 0.0, si = 0.0;
      for (int j = 0; j < 10; ++j) {
        if (j == i) continue;
        const double ex = x - zx[j], ey = y - zy[j], ee = ex * ex + ey * ey;
        sr = sr + ex / ee, si = si - ey / ee;
      }
      const double qr = 1.0 - (wr * sr - wi * si), qi = -(wr * si + wi * sr);
      const double qq = qr * qr + qi * qi;
      const double cr = (wr * qr + wi * qi) / qq, cim = (wi * qr - wr * qi) / qq;
      if (finite_d(cr) && finite_d(cim)) zx[i] = x - cr, zy[i] = y - cim;
    }
  int nr = 0;
  for (int i = 0; i < 10; ++i) {
    const double mod = sqrt(zx[i] * zx[i] + zy[i] * zy[i]);
    if (!(fabs(zy[i]) <= ROOT_IM_TOL * fmax(1.0, mod))) continue;
    double x = zx[i];
    for (int s = 0; s < NEWTON_STEPS; ++s) {
      double p = 1.0, dp = 0.0;
      for (int k = 9; k >= 0; --k) dp = dp * x + p, p = p * x + a[k];
      const double xn = x - p / dp;
      x = (dp != 0.0 && finite_d(xn)) ? xn : x;
    }
    int pos = nr;  // insertion, ascending; equal values keep their order
    while (pos > 0 && zr[pos - 1] > x) zr[pos] = zr[pos - 1], --pos;
    zr[pos] = x;
    ++nr;
  }
  return nr;
}

template <int N>
PFR_HD inline double peval(const double (&c)[N], double z) {
  double v = c[N - 1];
  for (int k = N - 2; k >= 0; --k) v = v * z + c[k];
  return v;
}

// POLISH_STEPS Gauss-Newton steps on the ten cubics A mon(x, y, z) = 0, A the
// 10x20 matrix before the elimination: mon_k = (x^a y^b) z^c over the cubic
// monomials, r = A mon, J = A (dmon/dx, dmon/dy, dmon/dz) with dmon/dx = a
// ((x^(a-1) y^b) z^c) and so on, N = J^T J, g = J^T r (sums in row order), delta
// = adj(N) g / det N by cofactors, det expanded along the first row; (x, y, z)
// -= delta.  A step with a zero determinant or a non-finite delta is skipped.
// The hidden-variable route leaves (x, y, z) with the rounding of the
// elimination and of the polynomial's coefficients; these steps return to the
// constraints themselves.
PFR_HD inline void polish(const double (&A)[10][20], double& x, double& y, double& z) {
  const int ex[20][3] = {{3, 0, 0}, {0, 3, 0}, {2, 1, 0}, {1, 2, 0}, {2, 0, 1}, {2, 0, 0}, {0, 2, 1},
                         {0, 2, 0}, {1, 1, 1}, {1, 1, 0}, {1, 0, 2}, {1, 0, 1}, {1, 0, 0}, {0, 1, 2},
                         {0, 1, 1}, {0, 1, 0}, {0, 0, 3}, {0, 0, 2}, {0, 0, 1}, {0, 0, 0}};
  for (int step = 0; step < POLISH_STEPS; ++step) {
    const double px[4] = {1.0, x, x * x, (x * x) * x}, py[4] = {1.0, y, y * y, (y * y) * y};
    const double pz[4] = {1.0, z, z * z, (z * z) * z};
    double mon[20], d[20][3];
    for (int k = 0; k < 20; ++k) {
      const int a = ex[k][0], b = ex[k][1], c = ex[k][2];
      mon[k] = (px[a] * py[b]) * pz[c];
      d[k][0] = a ? (double)a * ((px[a - 1] * py[b]) * pz[c]) : 0.0;
      d[k][1] = b ? (double)b * ((px[a] * py[b - 1]) * pz[c]) : 0.0;
      d[k][2] = c ? (double)c * ((px[a] * py[b]) * pz[c - 1]) : 0.0;
    }
    double N[3][3] = {{0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}, {0.0, 0.0, 0.0}}, g[3] = {0.0, 0.0, 0.0};
    for (int r = 0; r < 10; ++r) {
      double res = 0.0, j[3] = {0.0, 0.0, 0.0};
      for (int k = 0; k < 20; ++k) {
        res = res + A[r][k] * mon[k];
        for (int i = 0; i < 3; ++i) j[i] = j[i] + A[r][k] * d[k][i];
      }
      for (int i = 0; i < 3; ++i) {
        g[i] = g[i] + j[i] * res;
        for (int l = i; l < 3; ++l) N[i][l] = N[i][l] + j[i] * j[l];
      }
    }
    const double c00 = N[1][1] * N[2][2] - N[1][2] * N[1][2];
    const double c01 = N[0][2] * N[1][2] - N[0][1] * N[2][2];
    const double c02 = N[0][1] * N[1][2] - N[0][2] * N[1][1];
    const double c11 = N[0][0] * N[2][2] - N[0][2] * N[0][2];
    const double c12 = N[0][1] * N[0][2] - N[0][0] * N[1][2];
    const double c22 = N[0][0] * N[1][1] - N[0][1] * N[0][1];
    const double det = (N[0][0] * c00 + N[0][1] * c01) + N[0][2] * c02;
    const double dx = ((c00 * g[0] + c01 * g[1]) + c02 * g[2]) / det;
    const double dy = ((c01 * g[0] + c11 * g[1]) + c12 * g[2]) / det;
    const double dz = ((c02 * g[0] + c12 * g[1]) + c22 * g[2]) / det;
    if (det != 0.0 && finite_d(dx) && finite_d(dy) && finite_d(dz)) x = x - dx, y = y - dy, z = z - dz;
  }
}

// The candidates of five matches m[i] = (x, y, u, v) in normalised camera
// coordinates, unit_sign-scaled, for the real roots in ascending order; their
// number, 0 for a rejected sample.  Per root z: B(z) is evaluated by Horner,
// the three cross products of its rows (0, 1), (0, 2), (1, 2) are formed, the
// first with the largest |third component| gives x = c0 / c2, y = c1 / c2;
// (x, y, z) is polished; E = ((x eb0 + y eb1) + z eb2) + eb3.  A root whose E
// is not finite or zero is dropped and the later ones move up.
PFR_HD inline int solve5(const double (&m)[5][4], double (&E)[MAXCAND][9]) {
  double a[5][9], eb[4][9];
  for (int i = 0; i < 5; ++i) pffund::epi_row(m[i][0], m[i][1], m[i][2], m[i][3], a[i]);
  if (!null4(a, eb)) return 0;
  double A[10][20], A0[10][20];
  constraints(eb, A);
  for (int r = 0; r < 10; ++r)
    for (int c = 0; c < 20; ++c) A0[r][c] = A[r][c];
  if (!gauss_jordan(A)) return 0;
  BMat B;
  bmatrix(A, B);
  double co[11], zr[10];
  poly10(B, co);
  const int nr = roots10(co, zr);
  int nc = 0;
  for (int r = 0; r < nr; ++r) {
    double z = zr[r];
    double b[3][3];
    for (int k = 0; k < 3; ++k)
      b[k][0] = peval<4>(B.bx[k], z), b[k][1] = peval<4>(B.by[k], z), b[k][2] = peval<5>(B.b1[k], z);
    const int pa[3] = {0, 0, 1}, pb[3] = {1, 2, 2};
    double c0 = 0.0, c1 = 0.0, c2 = 0.0;
    for (int k = 0; k < 3; ++k) {
      const double *u = b[pa[k]], *v = b[pb[k]];
      const double w2 = u[0] * v[1] - u[1] * v[0];
      if (k == 0 || fabs(w2) > fabs(c2))
        c0 = u[1] * v[2] - u[2] * v[1], c1 = u[2] * v[0] - u[0] * v[2], c2 = w2;
    }
    double x = c0 / c2, y = c1 / c2;
    polish(A0, x, y, z);
    double e[9];
    bool fin = true;
    for (int k = 0; k < 9; ++k) {
      e[k] = ((x * eb[0][k] + y * eb[1][k]) + z * eb[2][k]) + eb[3][k];
      fin = fin && finite_d(e[k]);
    }
    if (!fin || !pffund::unit_sign(e)) continue;
    for (int k = 0; k < 9; ++k) E[nc][k] = e[k];
    ++nc;
  }
  return nc;
}

PFR_HD inline void cross(const double* a, const double* b, double* c) {
  c[0] = a[1] * b[2] - a[2] * b[1];
  c[1] = a[2] * b[0] - a[0] * b[2];
  c[2] = a[0] * b[1] - a[1] * b[0];
}

// The frames of E: Jacobi on E^T E; v1, v2 the eigenvectors of the largest and
// the second largest eigenvalue (the first of equal ones first), v3 = v1 x v2;
// u_i = E v_i / |E v_i| for i = 1, 2, u3 = u1 x u2; when the first
// largest-magnitude entry of u3 is negative, (u1, u2) and (v1, v2) are swapped
// and u3, v3 negated.  U and V hold them as
// columns (row-major 3x3), so det V = +1 and, u1 and u2 being orthogonal, det U
// = +1.
PFR_HD inline void frames(const double (&E)[9], double (&U)[9], double (&V)[9]) {
  double g[3][3], w[3][3];
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      g[i][j] = (E[i] * E[j] + E[3 + i] * E[3 + j]) + E[6 + i] * E[6 + j];
      w[i][j] = i == j ? 1.0 : 0.0;
    }
  pffund::jacobi_sym<3, 3>(g, w);
  const double d0 = g[0][0], d1 = g[1][1], d2 = g[2][2];
  int i0 = 0;
  if (d1 > d0) i0 = 1;
  if (d2 > (i0 == 0 ? d0 : d1)) i0 = 2;
  const int ra = i0 == 0 ? 1 : 0, rb = i0 == 2 ? 1 : 2;  // the other two, ascending index
  const int i1 = g[rb][rb] > g[ra][ra] ? rb : ra;
  double v[3][3], u[3][3];
  for (int r = 0; r < 3; ++r) v[0][r] = w[r][i0], v[1][r] = w[r][i1];
  cross(v[0], v[1], v[2]);
  for (int k = 0; k < 2; ++k) {
    double s = 0.0;
    for (int r = 0; r < 3; ++r) {
      u[k][r] = (E[3 * r] * v[k][0] + E[3 * r + 1] * v[k][1]) + E[3 * r + 2] * v[k][2];
      s = s + u[k][r] * u[k][r];
    }
    s = sqrt(s);
    for (int r = 0; r < 3; ++r) u[k][r] = u[k][r] / s;
  }
  cross(u[0], u[1], u[2]);
  // E has two equal singular values, so which eigenvector comes first is decided
  // by rounding; swapping them turns u3 and v3 round.  The order that makes the
  // first largest-magnitude entry of u3 positive is taken.
  double big = 0.0;
  bool neg = false;
  for (int r = 0; r < 3; ++r)
    if (fabs(u[2][r]) > big) big = fabs(u[2][r]), neg = u[2][r] < 0.0;
  if (neg)
    for (int r = 0; r < 3; ++r) {
      double t = u[0][r];
      u[0][r] = u[1][r], u[1][r] = t, u[2][r] = -u[2][r];
      t = v[0][r];
      v[0][r] = v[1][r], v[1][r] = t, v[2][r] = -v[2][r];
    }
  for (int r = 0; r < 3; ++r)
    for (int k = 0; k < 3; ++k) U[3 * r + k] = u[k][r], V[3 * r + k] = v[k][r];
}

// E <- u1 v1^T + u2 v2^T: the nearest matrix with singular values (1, 1, 0)
PFR_HD inline void project(double (&E)[9]) {
  double U[9], V[9];
  frames(E, U, V);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) E[3 * r + c] = U[3 * r] * V[3 * c] + U[3 * r + 1] * V[3 * c + 1];
}

// The four [R | t] of E, row-major 3x4, in the order (U W V^T, +u3), (U W V^T,
// -u3), (U W^T V^T, +u3), (U W^T V^T, -u3), W = [0 -1 0; 1 0 0; 0 0 1]: U W =
// (u2, -u1, u3) and U W^T = (-u2, u1, u3) as columns.
PFR_HD inline void decompositions(const double (&E)[9], double (&P)[4][12]) {
  double U[9], V[9];
  frames(E, U, V);
  for (int r = 0; r < 3; ++r)
    for (int c = 0; c < 3; ++c) {
      const double a = U[3 * r + 1] * V[3 * c] - U[3 * r] * V[3 * c + 1];
      const double b = U[3 * r + 2] * V[3 * c + 2];
      const double ra = a + b, rb = b - a;
      P[0][4 * r + c] = ra, P[1][4 * r + c] = ra;
      P[2][4 * r + c] = rb, P[3][4 * r + c] = rb;
    }
  for (int r = 0; r < 3; ++r) {
    P[0][4 * r + 3] = U[3 * r + 2], P[1][4 * r + 3] = -U[3 * r + 2];
    P[2][4 * r + 3] = U[3 * r + 2], P[3][4 * r + 3] = -U[3 * r + 2];
  }
}

// The match (x, y) <-> (u, v) triangulated between [I | 0] and P = [R | t]:
// with a = R (x, y, 1), the two rows d1 (a0 - u a2) = u t2 - t0 and d1 (a1 - v
// a2) = v t2 - t1 give the least-squares depth d1 = (p . q) / (p . p) in the
// first view, and d2 = pftri::depth(P, d1 (x, y, 1)) in the second.  In front:
// both finite and positive.
PFR_HD inline bool in_front(const double (&P)[12], double x, double y, double u, double v) {
  const double a0 = (P[0] * x + P[1] * y) + P[2], a1 = (P[4] * x + P[5] * y) + P[6];
  const double a2 = (P[8] * x + P[9] * y) + P[10];
  const double p0 = a0 - u * a2, p1 = a1 - v * a2;
  const double q0 = u * P[11] - P[3], q1 = v * P[11] - P[7];
  const double d1 = (p0 * q0 + p1 * q1) / (p0 * p0 + p1 * p1);
  const double X[3] = {d1 * x, d1 * y, d1};
  const double d2 = pftri::depth(P, X);
  return d1 > 0.0 && d2 > 0.0 && finite_d(d1) && finite_d(d2);
}

// Host form of the refit: the linear fit from the 9x9 normal matrix
// (pffund::refit_from_normal), projected and unit_sign-scaled.  False when the
// result is not finite or zero.
PFR_HD inline bool refit_from_normal(double (&nmat)[9][9], double (&E)[9]) {
  pffund::refit_from_normal(nmat, E);
  project(E);
  bool fin = true;
  for (int k = 0; k < 9; ++k) fin = fin && finite_d(E[k]);
  return fin && pffund::unit_sign(E);
}

}  // namespace pfess
