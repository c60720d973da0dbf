// refine_solve.h -- the arithmetic of posfeat_refine_points (refine.hip) that the
// host and the kernels share: one observation's share of the 3x3 normal
// equations of the pixel reprojection error in the point, the damped solve, the
// Levenberg-Marquardt round with its step control, the fixed summation order of
// a long track (64 partial sums and the xor butterfly, restated for the host)
// and the plan (argument check, workspace layout).  The camera model and the
// inlier test are triangulate_solve.h's; d pixel / d Xc and the pivoted
// elimination are pose_solve.h's (pixel_jac, pivot_solve): the pose refit and
// this stage compile one text.  Plain C++ behind PFR_HD with no HIP call:
// posfeat_refine_point and tests/host/refine_check.cpp compile the same text as
// the kernels.  The definitions are stated in include/posfeat_hip.h.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "pose_solve.h"
#include "triangulate_solve.h"

#pragma clang fp contract(off)

namespace pfrefine {

using pffund::finite_d;

constexpr int LANE_TRACK = 16;        // members a lane-mapped track has at the most
constexpr int MAX_TRACK = pftri::MAX_TRACK;  // members a track has at the most (the wave kernel's LDS)
constexpr int MIN_ROUNDS = 1, MAX_ROUNDS = 8;
constexpr int MIN_STEPS = 1, MAX_STEPS = 32;
constexpr double LAMBDA0 = 1e-4;      // the damping a round starts with
constexpr double LAMBDA_MAX = 1e8;    // a damping above this ends the round
constexpr double LAMBDA_STEP = 10.0;  // down after a taken step, up after a refused one
constexpr double STEP_STOP = 1e-10;   // max |delta| <= this max(1, max |X|): converged
constexpr int ACC = 10;               // 6 of N (upper triangle, row-major), 3 of g, cost
constexpr int WAVE = 64;              // partial sums of a long track

PFR_HD inline void acc_zero(double (&acc)[ACC]) {
#pragma unroll
  for (int i = 0; i < ACC; ++i) acc[i] = 0.0;
}

// One observation's share at the point X: the residual r = pixel(R X + t) - (x,
// y), J = (d pixel / d Xc) R (2 x 3); acc += (J^T J upper triangle row-major,
// J^T r, r . r).  False when the depth is not positive or the residual is not
// finite (the sums are then of no use).
PFR_HD inline bool acc_row(const double* cam, const double* P, double x, double y,
                           const double (&X)[3], double (&acc)[ACC]) {
  const double xc = ((P[0] * X[0] + P[1] * X[1]) + P[2] * X[2]) + P[3];
  const double yc = ((P[4] * X[0] + P[5] * X[1]) + P[6] * X[2]) + P[7];
  const double z = ((P[8] * X[0] + P[9] * X[1]) + P[10] * X[2]) + P[11];
  double rx, ry, jx[3], jy[3];
  pfpose::pixel_jac(cam, xc, yc, z, x, y, rx, ry, jx, jy);
  double a[3], b[3];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    a[c] = (jx[0] * P[c] + jx[1] * P[4 + c]) + jx[2] * P[8 + c];
    b[c] = (jy[0] * P[c] + jy[1] * P[4 + c]) + jy[2] * P[8 + c];
  }
  int k = 0;
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int c = r; c < 3; ++c, ++k) acc[k] = (acc[k] + a[r] * a[c]) + b[r] * b[c];
#pragma unroll
  for (int r = 0; r < 3; ++r) acc[6 + r] = (acc[6 + r] + a[r] * rx) + b[r] * ry;
  const double e2 = rx * rx + ry * ry;
  acc[9] = acc[9] + e2;
  return z > 0.0 && finite_d(e2);
}

// (N + lambda diag N) delta = -g by pfpose::pivot_solve
PFR_HD inline bool lm_solve(const double (&acc)[ACC], double lambda, double (&delta)[3]) {
  double a[3][4];
  a[0][0] = acc[0] + lambda * acc[0], a[0][1] = acc[1], a[0][2] = acc[2];
  a[1][0] = acc[1], a[1][1] = acc[3] + lambda * acc[3], a[1][2] = acc[4];
  a[2][0] = acc[2], a[2][1] = acc[4], a[2][2] = acc[5] + lambda * acc[5];
#pragma unroll
  for (int r = 0; r < 3; ++r) a[r][3] = -acc[6 + r];
  return pfpose::pivot_solve<3>(a, delta);
}

// One round on a fixed set.  accumulate(X, acc) fills acc with the sums of
// acc_row over the set at X in the set's fixed order and returns whether every
// row of the set had a positive depth and a finite residual (every caller of
// one round must get the same bits).  X ends as the last accepted point, cost
// as the cost there (NaN when the set is unusable at the start); returns the
// number of taken steps.  At most `steps` evaluations after the first, and at
// most 13 refused solves in a row (lambda from LAMBDA0 past LAMBDA_MAX): no
// other loop bound.
template <class Acc>
PFR_HD inline int lm_round(double (&X)[3], int steps, Acc&& accumulate, double& cost) {
  double acc[ACC];
  cost = (double)NAN;
  if (!accumulate(X, acc)) return 0;
  double lambda = LAMBDA0;
  int taken = 0, evals = 0;
  while (evals < steps && lambda <= LAMBDA_MAX) {
    double delta[3];
    bool take = false;
    if (lm_solve(acc, lambda, delta)) {
      double Xn[3] = {X[0] + delta[0], X[1] + delta[1], X[2] + delta[2]}, accn[ACC];
      const bool ok = accumulate(Xn, accn);
      ++evals;
      take = ok && accn[9] < acc[9];
      if (take) {
#pragma unroll
        for (int i = 0; i < 3; ++i) X[i] = Xn[i];
#pragma unroll
        for (int i = 0; i < ACC; ++i) acc[i] = accn[i];
      }
    }
    if (!take) {
      lambda = lambda * LAMBDA_STEP;
      continue;
    }
    lambda = lambda / LAMBDA_STEP;
    ++taken;
    const double big = fmax(fmax(fabs(delta[0]), fabs(delta[1])), fabs(delta[2]));
    const double size = fmax(1.0, fmax(fmax(fabs(X[0]), fabs(X[1])), fabs(X[2])));
    if (big <= STEP_STOP * size) break;
  }
  cost = acc[9];
  return taken;
}

// The sums of a track of more than LANE_TRACK members, on the host: member k
// adds to partial sum k mod 64 in ascending k (a member outside the set adds
// nothing), then the xor butterfly v[l] <- v[l] + v[l ^ o] for o = 32, 16, 8, 4,
// 2, 1, which leaves every v[l] with the same bits.  The wave kernel does the
// same with a lane per partial sum.
inline void butterfly(double (&part)[WAVE][ACC], double (&acc)[ACC]) {
  for (int o = WAVE / 2; o > 0; o >>= 1) {
    double next[WAVE][ACC];
    for (int l = 0; l < WAVE; ++l)
      for (int i = 0; i < ACC; ++i) next[l][i] = part[l][i] + part[l ^ o][i];
    for (int l = 0; l < WAVE; ++l)
      for (int i = 0; i < ACC; ++i) part[l][i] = next[l][i];
  }
  for (int i = 0; i < ACC; ++i) acc[i] = part[0][i];
}

// obs [n][22] = (x, y, cam 8, pose 12): the sums over all n rows at X in the
// order a track of n members has (n <= LANE_TRACK: member order)
inline bool accumulate_rows(const double* obs, int n, const double (&X)[3], double (&acc)[ACC]) {
  bool ok = true;
  if (n <= LANE_TRACK) {
    acc_zero(acc);
    for (int k = 0; k < n; ++k) {
      const double* o = obs + 22 * (size_t)k;
      ok = acc_row(o + 2, o + 10, o[0], o[1], X, acc) && ok;
    }
    return ok;
  }
  double part[WAVE][ACC];
  for (int l = 0; l < WAVE; ++l) acc_zero(part[l]);
  for (int k = 0; k < n; ++k) {
    const double* o = obs + 22 * (size_t)k;
    ok = acc_row(o + 2, o + 10, o[0], o[1], X, part[k % WAVE]) && ok;
  }
  butterfly(part, acc);
  return ok;
}

// ---- the plan -------------------------------------------------------------------

inline bool params_ok(double thr, double min_angle_deg, int rounds, int steps) {
  return thr > 0.0 && thr < (double)INFINITY && min_angle_deg >= 0.0 && min_angle_deg < 90.0 &&
         rounds >= MIN_ROUNDS && rounds <= MAX_ROUNDS && steps >= MIN_STEPS && steps <= MAX_STEPS;
}

// Workspace (byte offsets, each 256-B aligned), N = set_off[nsets] rows:
//   set table   (nsets + 1) int32 (uploaded per call)
//   setid       N int32: the set of a row
struct Layout {
  long long n = 0;
  size_t set_off = 0, setid = 0, total = 0;
};
inline int layout(const int32_t* set_off, int nsets, long long tmax, long long mmax, Layout& L) {
  L = Layout();
  if (pftri::check_sets(set_off, nsets) != 0 || tmax < 0 || mmax < 0 || tmax > INT32_MAX - 1 ||
      mmax > INT32_MAX)
    return -1;
  L.n = set_off[nsets];
  size_t at = 0;
  L.set_off = at, at += pftri::al256((size_t)(nsets + 1) * 4);
  L.setid = at, at += pftri::al256((size_t)L.n * 4);
  L.total = at + 256;
  return 0;
}

}  // namespace pfrefine
