// split_plan.h -- the plan of posfeat_split_tracks (triangulate.hip) that the
// host and the kernels share: the parameter check, the numbering of the output
// tracks under a capacity and the workspace layout.  Plain C++ behind PFR_HD
// with no HIP call: tests/host/split_check.cpp compiles the same text as the
// kernels.  The definitions are stated in include/posfeat_hip.h.
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "triangulate_solve.h"

namespace pfsplit {

constexpr int MIN_ROUNDS = 1, MAX_ROUNDS = 4;  // generations a parent runs at the most
constexpr int SCAN_PARENTS = 2048;             // parents per workgroup of the scan launches

inline bool params_ok(int iters, double thr, double min_angle_deg, int rounds) {
  return iters >= pftri::MIN_ITERS && iters <= pftri::MAX_ITERS && thr > 0.0 &&
         thr < (double)INFINITY && min_angle_deg >= 0.0 && min_angle_deg < 90.0 &&
         rounds >= MIN_ROUNDS && rounds <= MAX_ROUNDS;
}

// The output tracks under the capacity tmax_out >= T.  Parent t of T found c
// children; u = the sum of (1 + c) over the parents before it.  In output order
// (parent 0, its children, parent 1, ...) a child is created iff its number
// plus the parents still to come stays below tmax_out, so every parent keeps a
// place.  That quantity grows by 0 (a parent) or 1 (a child) along the order,
// so the refused children are a suffix of the children and the rule has this
// closed form, which needs nothing but u:
//   id(t)      = min(u, tmax_out - (T - t))
//   created(t) = min(c, tmax_out - (T - 1 - t) - 1 - id(t))
PFR_HD inline long long parent_id(long long u, long long t, long long T, long long tmax_out) {
  const long long last = tmax_out - (T - t);
  return u < last ? u : last;
}
PFR_HD inline int children_created(long long u, int c, long long t, long long T, long long tmax_out) {
  const long long room = tmax_out - (T - 1 - t) - 1 - parent_id(u, t, T, tmax_out);
  return (long long)c < room ? c : (int)(room > 0 ? room : 0);
}

// Workspace (byte offsets, each 256-B aligned), N = set_off[nsets] rows:
//   set table   (nsets + 1) int32 (uploaded per call)
//   setid       N int32: the set of a row
//   und         N x 2 fp64: the undistorted normalised point of a row
//   list        mmax int32: the left-over list of a lane-mapped parent, in its range
//   mark        mmax uint8: the generation that claimed a member, 0 for none
//   nleft       tmax int32: |L1| of a parent that may split, -1 for a carried one
//   nchild      tmax int32: the children a parent found
//   ids         tmax int32: the output id of a parent
//   ncreated    tmax int32: the children of a parent that fit
//   cpoint      tmax x 4 x 3 fp64, cerr tmax x 4 fp64, cinfo tmax x 4 x 4 int32:
//               the children's points, errors and info
//   bsum        max(1, ceil(tmax / SCAN_PARENTS)) uint64: the scan's block sums
struct Layout {
  long long n = 0, nblk = 0;
  size_t set_off = 0, setid = 0, und = 0, list = 0, mark = 0, nleft = 0, nchild = 0, ids = 0,
         ncreated = 0, cpoint = 0, cerr = 0, cinfo = 0, bsum = 0, total = 0;
};
inline int layout(const int32_t* set_off, int nsets, long long tmax, long long mmax,
                  long long tmax_out, Layout& L) {
  L = Layout();
  if (pftri::check_sets(set_off, nsets) != 0 || tmax < 0 || mmax < 0 || tmax > INT32_MAX - 1 ||
      mmax > INT32_MAX || tmax_out < tmax || tmax_out > INT32_MAX - 1)
    return -1;
  using pftri::al256;
  L.n = set_off[nsets];
  L.nblk = tmax > 0 ? (tmax + SCAN_PARENTS - 1) / SCAN_PARENTS : 1;
  const size_t n = (size_t)L.n, t = (size_t)tmax, m = (size_t)mmax;
  size_t at = 0;
  L.set_off = at, at += al256((size_t)(nsets + 1) * 4);
  L.setid = at, at += al256(n * 4);
  L.und = at, at += al256(n * 16);
  L.list = at, at += al256(m * 4);
  L.mark = at, at += al256(m);
  L.nleft = at, at += al256(t * 4);
  L.nchild = at, at += al256(t * 4);
  L.ids = at, at += al256(t * 4);
  L.ncreated = at, at += al256(t * 4);
  L.cpoint = at, at += al256(t * 4 * 3 * 8);
  L.cerr = at, at += al256(t * 4 * 8);
  L.cinfo = at, at += al256(t * 4 * 4 * 4);
  L.bsum = at, at += al256((size_t)L.nblk * 8);
  L.total = at + 256;
  return 0;
}

}  // namespace pfsplit
