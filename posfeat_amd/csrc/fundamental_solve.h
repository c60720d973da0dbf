// fundamental_solve.h -- the arithmetic of posfeat_ransac_fundamental
// (fundamental.hip) that the host and the kernels share: the 7-point solve
// (elimination with full pivoting, the cubic, its roots), the Sampson inlier
// test, the cyclic Jacobi eigen-solve (9x9 for the 8-point refit, 3x3 for the
// rank-2 projection) and the output scaling.  Plain C++ behind PFR_HD with no
// HIP call: posfeat_fundamental_solve7 and tests/host/fundamental_solve_check.cpp
// compile the same text as the kernels.  The definitions are stated in
// include/posfeat_hip.h; every array is indexed by compile-time constants once
// the loops are unrolled, so on the device they live in registers.
#pragma once
#include <math.h>
#include <stdint.h>

#include "ransac_plan.h"

#pragma clang fp contract(off)

namespace pffund {

constexpr double PIVOT_REL = 1e-12;   // pivot / largest entry of the system below this: rejected
constexpr double LEAD_REL = 1e-12;    // leading coefficient / largest coefficient: degree drops
constexpr int NEWTON_STEPS = 2;       // on each closed-form root of the cubic
constexpr int JACOBI_SWEEPS = 16;     // at most
constexpr double JACOBI_OFF = 1e-32;  // stop: sum offdiag^2 <= this * sum diag^2

PFR_HD inline bool finite_d(double x) { return fabs(x) < (double)INFINITY; }

// the row of x2^T F x1 = 0 for x1 = (x, y, 1), x2 = (u, v, 1), F row-major
PFR_HD inline void epi_row(double x, double y, double u, double v, double (&r)[9]) {
  r[0] = u * x, r[1] = u * y, r[2] = u;
  r[3] = v * x, r[4] = v * y, r[5] = v;
  r[6] = x, r[7] = y, r[8] = 1.0;
}

// The null space of the 7x9 system `a` (destroyed): Gaussian elimination with
// full pivoting.  Step s = 0..6 takes the first largest |a[r][c]| over r >= s,
// c >= s in row-major order, swaps it to (s, s) (rows, then columns, the
// column permutation remembered), rejects when it is below PIVOT_REL times the
// largest entry of the system as given (or is not a positive number), and
// clears column s below.  The columns left at positions 7 and 8 are free: f1
// is the null vector with (1, 0) there, f2 the one with (0, -1), by back
// substitution.  The pencil l f1 + (1 - l) f2 has (l, l - 1) there, so its
// point at infinity is the matrix whose two free entries are equal; with (0,
// 1) it would be the one whose free entries are opposite, which is every
// skew-symmetric F (a pure translation) whenever the free columns are a
// transposed pair.  False for a rejected system (f1, f2 not meaningful).
PFR_HD inline bool null2(double (&a)[7][9], double (&f1)[9], double (&f2)[9]) {
  double amax = 0.0;
#pragma unroll
  for (int r = 0; r < 7; ++r)
#pragma unroll
    for (int c = 0; c < 9; ++c) {
      const double v = fabs(a[r][c]);
      amax = (v > amax || v != v) ? v : amax;  // a NaN sticks
    }
  int perm[9];
#pragma unroll
  for (int c = 0; c < 9; ++c) perm[c] = c;
  bool ok = true;
#pragma unroll
  for (int s = 0; s < 7; ++s) {
    int pr = s, pc = s;
    double best = fabs(a[s][s]);
#pragma unroll
    for (int r = s; r < 7; ++r)
#pragma unroll
      for (int c = s; c < 9; ++c) {
        const double v = fabs(a[r][c]);
        if (v > best) {
          best = v;
          pr = r;
          pc = c;
        }
      }
#pragma unroll
    for (int r = s + 1; r < 7; ++r) {
      const bool sw = pr == r;
#pragma unroll
      for (int k = s; k < 9; ++k) {
        const double t = a[s][k], u = a[r][k];
        a[s][k] = sw ? u : t;
        a[r][k] = sw ? t : u;
      }
    }
#pragma unroll
    for (int c = s + 1; c < 9; ++c) {
      const bool sw = pc == c;
#pragma unroll
      for (int r = 0; r < 7; ++r) {
        const double t = a[r][s], u = a[r][c];
        a[r][s] = sw ? u : t;
        a[r][c] = sw ? t : u;
      }
      const int t = perm[s], u = perm[c];
      perm[s] = sw ? u : t;
      perm[c] = sw ? t : u;
    }
    ok = ok && best >= PIVOT_REL * amax && best > 0.0;
#pragma unroll
    for (int r = s + 1; r < 7; ++r) {
      const double f = a[r][s] / a[s][s];
#pragma unroll
      for (int k = s + 1; k < 9; ++k) a[r][k] = a[r][k] - f * a[s][k];
    }
  }
  double z1[9], z2[9];
  z1[7] = 1.0, z1[8] = 0.0, z2[7] = 0.0, z2[8] = -1.0;
#pragma unroll
  for (int c = 6; c >= 0; --c) {
    double s1 = -a[c][7], s2 = a[c][8];
#pragma unroll
    for (int k = c + 1; k < 7; ++k) {
      s1 = s1 - a[c][k] * z1[k];
      s2 = s2 - a[c][k] * z2[k];
    }
    z1[c] = s1 / a[c][c];
    z2[c] = s2 / a[c][c];
  }
#pragma unroll
  for (int j = 0; j < 9; ++j) {
    double v1 = 0.0, v2 = 0.0;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      v1 = perm[k] == j ? z1[k] : v1;
      v2 = perm[k] == j ? z2[k] : v2;
    }
    f1[j] = v1;
    f2[j] = v2;
  }
  return ok;
}

// a . (b x c) of three rows
PFR_HD inline double triple(const double* a, const double* b, const double* c) {
  return a[0] * (b[1] * c[2] - b[2] * c[1]) - a[1] * (b[0] * c[2] - b[2] * c[0]) +
         a[2] * (b[0] * c[1] - b[1] * c[0]);
}

// det(l f1 + (1 - l) f2) = det(B + l D), B = f2, D = f1 - f2, as
// co[0] + co[1] l + co[2] l^2 + co[3] l^3: the determinant is linear in each
// row, so co[k] sums the determinants with k rows from D
PFR_HD inline void cubic_coeffs(const double (&f1)[9], const double (&f2)[9], double (&co)[4]) {
  double d[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) d[i] = f1[i] - f2[i];
  const double *b0 = f2, *b1 = f2 + 3, *b2 = f2 + 6, *d0 = d, *d1 = d + 3, *d2 = d + 6;
  co[0] = triple(b0, b1, b2);
  co[1] = triple(d0, b1, b2) + triple(b0, d1, b2) + triple(b0, b1, d2);
  co[2] = triple(d0, d1, b2) + triple(d0, b1, d2) + triple(b0, d1, d2);
  co[3] = triple(d0, d1, d2);
}

// The real roots of co[0] + co[1] l + co[2] l^2 + co[3] l^3, ascending in
// lam[0..count); the unused entries are +inf.  With cm the largest |co[k]|:
// |co[3]| > LEAD_REL cm: the monic cubic l^3 + a l^2 + b l + d in closed form
// (Q = (a^2 - 3 b) / 9, R = (2 a^3 - 9 a b + 27 d) / 54; R^2 < Q^3: three roots
// -2 sqrt(Q) cos((t + 2 pi k) / 3) - a / 3, t = acos(R / sqrt(Q^3)), k = 0, 1,
// -1; else the one root A + Q / A - a / 3, A = -sign(R) cbrt(|R| + sqrt(R^2 -
// Q^3)), Q / A read as 0 for A = 0), each polished by NEWTON_STEPS Newton steps
// on the monic cubic (a step with a zero derivative or a non-finite result is
// skipped), then sorted; else |co[2]| > LEAD_REL cm: the quadratic by q =
// -(co[1] + sign(co[1]) sqrt(disc)) / 2, roots q / co[2] and co[0] / q (both 0
// for q = 0), none for disc < 0; else |co[1]| > LEAD_REL cm: -co[0] / co[1];
// else none.  No root either when a coefficient is not finite or all are 0.
PFR_HD inline int cubic_roots(const double (&co)[4], double (&lam)[3]) {
  lam[0] = lam[1] = lam[2] = (double)INFINITY;
  const double cm = fmax(fmax(fabs(co[0]), fabs(co[1])), fmax(fabs(co[2]), fabs(co[3])));
  if (!(cm > 0.0) || !finite_d(co[0] + co[1] + co[2] + co[3]) || !finite_d(cm)) return 0;
  int nr = 0;
  if (fabs(co[3]) > LEAD_REL * cm) {
    const double a = co[2] / co[3], b = co[1] / co[3], d = co[0] / co[3];
    const double Q = (a * a - 3.0 * b) / 9.0;
    const double R = ((2.0 * (a * a) - 9.0 * b) * a + 27.0 * d) / 54.0;
    const double Q3 = Q * Q * Q, a3 = a / 3.0;
    if (R * R < Q3) {
      const double sq = -2.0 * sqrt(Q);
      const double t = acos(fmin(1.0, fmax(-1.0, R / sqrt(Q3))));
      const double tp = 6.283185307179586476925;
      lam[0] = sq * cos(t / 3.0) - a3;
      lam[1] = sq * cos((t + tp) / 3.0) - a3;
      lam[2] = sq * cos((t - tp) / 3.0) - a3;
      nr = 3;
    } else {
      const double m = cbrt(fabs(R) + sqrt(R * R - Q3));
      const double A = R >= 0.0 ? -m : m;
      const double B = A != 0.0 ? Q / A : 0.0;
      lam[0] = A + B - a3;
      nr = 1;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      double x = lam[i];
#pragma unroll
      for (int k = 0; k < NEWTON_STEPS; ++k) {
        const double p = ((x + a) * x + b) * x + d;
        const double dp = (3.0 * x + 2.0 * a) * x + b;
        const double xn = x - p / dp;
        x = (dp != 0.0 && finite_d(xn)) ? xn : x;
      }
      lam[i] = i < nr ? x : lam[i];
    }
  } else if (fabs(co[2]) > LEAD_REL * cm) {
    const double disc = co[1] * co[1] - 4.0 * co[2] * co[0];
    if (disc >= 0.0) {
      const double sd = sqrt(disc);
      const double q = -(co[1] + (co[1] >= 0.0 ? sd : -sd)) / 2.0;
      lam[0] = q != 0.0 ? q / co[2] : 0.0;
      lam[1] = q != 0.0 ? co[0] / q : 0.0;
      nr = 2;
    }
  } else if (fabs(co[1]) > LEAD_REL * cm) {
    lam[0] = -co[0] / co[1];
    nr = 1;
  }
  // ascending (the unused entries, +inf, stay last)
  double t;
  if (lam[1] < lam[0]) t = lam[0], lam[0] = lam[1], lam[1] = t;
  if (lam[2] < lam[1]) t = lam[1], lam[1] = lam[2], lam[2] = t;
  if (lam[1] < lam[0]) t = lam[0], lam[0] = lam[1], lam[1] = t;
  return nr;
}

// The candidates of seven matches m[i] = (x, y, u, v) in normalised
// coordinates: Fn[r] = lam_r f1 + (1 - lam_r) f2 for the roots in ascending
// order.  Returns their number, 0 for a rejected sample; the rows of Fn past
// it are NaN.
PFR_HD inline int solve7(const double (&m)[7][4], double (&Fn)[3][9]) {
  double a[7][9], f1[9], f2[9], co[4], lam[3];
#pragma unroll
  for (int i = 0; i < 7; ++i) epi_row(m[i][0], m[i][1], m[i][2], m[i][3], a[i]);
  const bool ok = null2(a, f1, f2);
  cubic_coeffs(f1, f2, co);
  int nr = cubic_roots(co, lam);
  nr = ok ? nr : 0;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int i = 0; i < 9; ++i)
      Fn[r][i] = r < nr ? lam[r] * f1[i] + (1.0 - lam[r]) * f2[i] : (double)NAN;
  return nr;
}

// F = T2^T Fn T1 with Ti = [s 0 -s cx; 0 s -s cy; 0 0 1]
PFR_HD inline void denormalise(const double (&fn)[9], double cx1, double cy1, double s1, double cx2,
                               double cy2, double s2, double (&F)[9]) {
  double m[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    m[3 * r] = fn[3 * r] * s1;
    m[3 * r + 1] = fn[3 * r + 1] * s1;
    m[3 * r + 2] = fn[3 * r + 2] - s1 * (fn[3 * r] * cx1 + fn[3 * r + 1] * cy1);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    F[c] = s2 * m[c];
    F[3 + c] = s2 * m[3 + c];
    F[6 + c] = m[6 + c] - s2 * (cx2 * m[c] + cy2 * m[3 + c]);
  }
}

// squared Sampson distance <= thr2, without the division: e^2 <= thr2 den with
// den finite and positive.  A NaN anywhere fails every test.
PFR_HD inline bool sampson_inlier(const double (&F)[9], double x, double y, double u, double v,
                                  double thr2) {
  const double a0 = __builtin_fma(F[0], x, __builtin_fma(F[1], y, F[2]));
  const double a1 = __builtin_fma(F[3], x, __builtin_fma(F[4], y, F[5]));
  const double a2 = __builtin_fma(F[6], x, __builtin_fma(F[7], y, F[8]));
  const double b0 = __builtin_fma(F[0], u, __builtin_fma(F[3], v, F[6]));
  const double b1 = __builtin_fma(F[1], u, __builtin_fma(F[4], v, F[7]));
  const double e = __builtin_fma(u, a0, __builtin_fma(v, a1, a2));
  const double den = __builtin_fma(a0, a0, __builtin_fma(a1, a1, __builtin_fma(b0, b0, b1 * b1)));
  const double lim = thr2 * den;
  return e * e <= lim && lim < (double)INFINITY && den > 0.0;
}

// Cyclic Jacobi on the symmetric N x N matrix held in the upper triangle of a
// (r <= c; the rest is neither read nor written).  A sweep visits (p, q), p < q,
// in row-major order; with apq != 0: theta = (aqq - app) / (2 apq), t =
// sign(theta) / (|theta| + sqrt(theta^2 + 1)) (sign(0) = +1), c = 1 / sqrt(t^2
// + 1), s = t c; app -= t apq, aqq += t apq, apq = 0, and for every other k
// (akp, akq) <- (c akp - s akq, s akp + c akq); the rows of v turn the same
// way.  Before each sweep: stop unless sum_{p<q} apq^2 > JACOBI_OFF sum aii^2;
// at most JACOBI_SWEEPS sweeps.  v holds NR rows of the accumulated rotation
// (the caller sets them to rows of the identity): eigenvector j is column j.
template <int N, int NR>
PFR_HD inline void jacobi_sym(double (&a)[N][N], double (&v)[NR][N]) {
  for (int sweep = 0; sweep < JACOBI_SWEEPS; ++sweep) {
    double off = 0.0, dg = 0.0;
#pragma unroll
    for (int p = 0; p < N; ++p) {
      dg = dg + a[p][p] * a[p][p];
#pragma unroll
      for (int q = p + 1; q < N; ++q) off = off + a[p][q] * a[p][q];
    }
    if (!(off > JACOBI_OFF * dg)) break;
#pragma unroll
    for (int p = 0; p < N - 1; ++p)
#pragma unroll
      for (int q = p + 1; q < N; ++q) {
        const double apq = a[p][q];
        const double theta = (a[q][q] - a[p][p]) / (2.0 * apq);
        const double tt = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
        const double t = apq != 0.0 ? tt : 0.0;
        const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
        a[p][p] = a[p][p] - t * apq;
        a[q][q] = a[q][q] + t * apq;
        a[p][q] = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) {
          if (k == p || k == q) continue;
          double& akp = k < p ? a[k][p] : a[p][k];
          double& akq = k < q ? a[k][q] : a[q][k];
          const double x = akp, y = akq;
          akp = c * x - s * y;
          akq = s * x + c * y;
        }
#pragma unroll
        for (int r = 0; r < NR; ++r) {
          const double x = v[r][p], y = v[r][q];
          v[r][p] = c * x - s * y;
          v[r][q] = s * x + c * y;
        }
      }
  }
}

// the first lowest diagonal entry
template <int N>
PFR_HD inline int min_diag(const double (&a)[N][N]) {
  int j = 0;
  double best = a[0][0];
#pragma unroll
  for (int i = 1; i < N; ++i)
    if (a[i][i] < best) best = a[i][i], j = i;
  return j;
}

// Rank 2: with w the eigenvector of the smallest eigenvalue of F^T F (3x3
// Jacobi, first lowest on a tie), F <- F - (F w) w^T, which zeroes the smallest
// singular value.
PFR_HD inline void rank2(double (&F)[9]) {
  double g[3][3], w[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      g[i][j] = F[i] * F[j] + F[3 + i] * F[3 + j] + F[6 + i] * F[6 + j];
      w[i][j] = i == j ? 1.0 : 0.0;
    }
  jacobi_sym<3, 3>(g, w);
  const int jm = min_diag<3>(g);
  double e[3];
#pragma unroll
  for (int r = 0; r < 3; ++r) e[r] = jm == 0 ? w[r][0] : (jm == 1 ? w[r][1] : w[r][2]);
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double fw = F[3 * r] * e[0] + F[3 * r + 1] * e[1] + F[3 * r + 2] * e[2];
#pragma unroll
    for (int c = 0; c < 3; ++c) F[3 * r + c] = F[3 * r + c] - fw * e[c];
  }
}

// Frobenius norm 1, the first largest-magnitude entry positive.  False (F
// untouched) when the norm is 0 or not finite.
PFR_HD inline bool unit_sign(double (&F)[9]) {
  double ss = 0.0, big = 0.0, sgn = 1.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) {
    ss = ss + F[i] * F[i];
    if (fabs(F[i]) > big) big = fabs(F[i]), sgn = F[i] >= 0.0 ? 1.0 : -1.0;
  }
  if (!(ss > 0.0) || !finite_d(ss)) return false;
  const double sc = sgn / sqrt(ss);
#pragma unroll
  for (int i = 0; i < 9; ++i) F[i] = F[i] * sc;
  return true;
}

// The 8-point refit from the 9x9 normal matrix (upper triangle of nmat,
// destroyed): the eigenvector of its smallest eigenvalue, then rank 2.  Host
// form, with the whole rotation; the select kernel keeps one row per lane.
PFR_HD inline void refit_from_normal(double (&nmat)[9][9], double (&Fn)[9]) {
  double v[9][9];
#pragma unroll
  for (int i = 0; i < 9; ++i)
#pragma unroll
    for (int j = 0; j < 9; ++j) v[i][j] = i == j ? 1.0 : 0.0;
  jacobi_sym<9, 9>(nmat, v);
  const int jm = min_diag<9>(nmat);
#pragma unroll
  for (int r = 0; r < 9; ++r) {
    double e = 0.0;
#pragma unroll
    for (int j = 0; j < 9; ++j) e = jm == j ? v[r][j] : e;
    Fn[r] = e;
  }
  rank2(Fn);
}

}  // namespace pffund
