// guided_solve.h -- the arithmetic of posfeat_match_pairs_guided
// (matchpairs.hip) that the host and the kernels share: the per-keypoint
// record of a pair's 3x3 model and the fp32 admissibility predicate the top-2
// fold evaluates.  Plain C++ behind PFG_HD with no HIP call:
// posfeat_guided_record / posfeat_guided_admissible and
// tests/host/guided_check.cpp compile the same text as the kernels.  The
// definitions are stated in include/posfeat_hip.h.  Contraction is off inside
// each function (not for the including file), so every operation is rounded
// once wherever the text is inlined and numpy restates it bit for bit.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PFG_HD __host__ __device__ __forceinline__
#else
#define PFG_HD inline
#endif

namespace pfguided {

constexpr int HOMOGRAPHY = 0, FUNDAMENTAL = 1;

// The record of point (a, b): side 0 an image-1 point (Q = M), side 1 an
// image-2 point (Q = M^T for a fundamental matrix; the point itself for a
// homography).  q_k = (Q[k][0] a + Q[k][1] b) + Q[k][2] in fp64; each
// component is rounded to fp32 last.
PFG_HD void record(int model, int side, const double* M, float a, float b, float (&r)[4]) {
#pragma clang fp contract(off)
  if (model == HOMOGRAPHY && side != 0) {
    r[0] = a, r[1] = b, r[2] = 0.f, r[3] = 0.f;
    return;
  }
  const double x = (double)a, y = (double)b;
  double q[3];
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    const double q0 = side == 0 ? M[3 * k] : M[k];
    const double q1 = side == 0 ? M[3 * k + 1] : M[3 + k];
    const double q2 = side == 0 ? M[3 * k + 2] : M[6 + k];
    q[k] = (q0 * x + q1 * y) + q2;
  }
  if (model == FUNDAMENTAL) {
    r[0] = (float)q[0], r[1] = (float)q[1], r[2] = (float)q[2];
    r[3] = (float)(q[0] * q[0] + q[1] * q[1]);
  } else {  // the projected point, no sign test on q2
    r[0] = (float)(q[0] / q[2]), r[1] = (float)(q[1] / q[2]), r[2] = 0.f, r[3] = 0.f;
  }
}

// Admissible(streamed row, column) in fp32.  (ra0..ra3) is the streamed row's
// record.  Fundamental: (cx, cy) is the column's keypoint and cw the w of the
// column's record.  Homography: (cx, cy) is the column's record (x, y); the
// definition's du = u - px is ra0 - cx on the side that streams image 2 and
// cx - ra0 on the other, and the two squares are the same fp32 number, so one
// text serves both sides.  Any NaN fails.
template <int MODEL>
PFG_HD bool admissible(float ra0, float ra1, float ra2, float ra3, float cx, float cy, float cw,
                       float t2) {
#pragma clang fp contract(off)
  if (MODEL == FUNDAMENTAL) {
    const float e = ((ra0 * cx) + (ra1 * cy)) + ra2;
    const float den = ra3 + cw;
    const float td = t2 * den;
    return den > 0.f && fabsf(td) < INFINITY && e * e <= td;
  }
  const float du = ra0 - cx, dv = ra1 - cy;
  return (du * du + dv * dv) <= t2;
}

}  // namespace pfguided
