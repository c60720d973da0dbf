// pose.hip -- RANSAC absolute poses for every query of a list from 2D-3D
// correspondences, on gfx950: what the reference's Aachen pipeline asks of
// `colmap image_registrator`.  Three launches whatever the number of queries,
// in the mould of fundamental.hip:
//
//   pose_gather_kernel  per correspondence: its query (binary search in the
//                       uploaded table), the pixel, the undistorted point and
//                       the world point as one 64-byte row; a correspondence
//                       out of range or not finite becomes a row of NaNs.
//   pose_hyp_kernel     one workgroup per (query, block of 256 iterations), one
//                       sample per lane.  Phase 1: the lane draws three
//                       correspondences (the first three draws of sample4),
//                       solves Grunert's quartic and keeps up to four candidate
//                       poses (48 doubles).  Phase 2: the query's rows go
//                       through LDS in tiles of 256 as (xd, yd, X, Y, Z) (12 KB
//                       with the padding; every lane reads the same address, a
//                       broadcast) and the lane scores its candidates against
//                       each staged row with the division-free reprojection
//                       test.  A wave then a block reduction of the (count,
//                       iteration, root) key fills the slot.
//   pose_select_kernel  one workgroup per query: reduces the slots, rebuilds the
//                       winner from (iteration, root) with the same operations,
//                       marks its inliers, runs the Gauss-Newton refit over
//                       them (each accumulation: thread-strided ascending rows,
//                       the xor butterfly inside the wave, the waves in order;
//                       every thread then solves the same 6x6 system on the
//                       same bits), recounts, applies the keep rule, writes the
//                       pose, info and the mask.
//
// All of the arithmetic is pose_solve.h, the text the host compiles for
// posfeat_pose_solve3.  Floating-point contraction is off for the whole file.
#include <math.h>

#include "common.h"
#include "pose_solve.h"

#pragma clang fp contract(off)

namespace {

using namespace pfransac_plan;
using namespace pfpose;

static_assert(RBLOCK == 256 && RTILE == 256, "one staged row per thread of a workgroup");
constexpr int TILE_DOUBLES = 6;  // xd yd X Y Z and one of padding: 16-B aligned rows

__global__ __launch_bounds__(256) void pose_gather_kernel(
    const float* __restrict__ kp, long long nkp, const double* __restrict__ cams,
    const double* __restrict__ points, long long npoints, const int32_t* __restrict__ corr,
    const int32_t* __restrict__ q_tab, int nq, long long ncorr, double* __restrict__ rows) {
  const long long c = (long long)blockIdx.x * 256 + threadIdx.x;
  if (c >= ncorr) return;
  // the query q with q_tab[q] <= c < q_tab[q + 1] (empty queries skipped)
  int lo = 0, hi = nq;
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (q_tab[mid] <= c) lo = mid; else hi = mid;
  }
  const int r = corr[2 * c], pt = corr[2 * c + 1];
  double o[ROW_DOUBLES];
#pragma unroll
  for (int i = 0; i < ROW_DOUBLES; ++i) o[i] = (double)NAN;
  if (r >= 0 && r < nkp && pt >= 0 && pt < npoints) {
    const double x = (double)kp[2 * (long long)r], y = (double)kp[2 * (long long)r + 1];
    const double X = points[3 * (long long)pt], Y = points[3 * (long long)pt + 1],
                 Z = points[3 * (long long)pt + 2];
    double xu, yu;
    pftri::undistort(cams + 8 * (long long)lo, x, y, xu, yu);
    if (finite_d(((((x + y) + xu) + yu) + X) + (Y + Z)))
      o[0] = x, o[1] = y, o[2] = xu, o[3] = yu, o[4] = X, o[5] = Y, o[6] = Z, o[7] = 0.0;
  }
  double2* dst = reinterpret_cast<double2*>(rows + ROW_DOUBLES * c);
#pragma unroll
  for (int i = 0; i < ROW_DOUBLES / 2; ++i) dst[i] = make_double2(o[2 * i], o[2 * i + 1]);
}

// the candidates of iteration `it` of query `q`; their number (0 for a rejected
// sample); the rows of pose past it are NaN and score nothing
__device__ __forceinline__ int candidates(uint64_t seed, int q, int it, int n,
                                          const double* __restrict__ rows, double (&pose)[4][12]) {
  int32_t idx[4];
  sample4(seed, q, it, n, idx);
  double m[3][5];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    const double* r = rows + ROW_DOUBLES * (long long)idx[i];
#pragma unroll
    for (int c = 0; c < 5; ++c) m[i][c] = r[2 + c];  // a NaN row rejects the sample
  }
  return p3p(m, pose);
}

__global__ __launch_bounds__(256) void pose_hyp_kernel(const int32_t* __restrict__ q_tab,
                                                       const double* __restrict__ cams,
                                                       const double* __restrict__ rows, int iters,
                                                       int nblk, double thr2, uint64_t seed,
                                                       unsigned long long* __restrict__ slots) {
  __shared__ __attribute__((aligned(16))) double tile[RTILE * TILE_DOUBLES];  // 12 KB
  __shared__ unsigned long long wbest[RBLOCK / 64];
  const int q = blockIdx.x / nblk, blk = blockIdx.x - q * nblk, tid = threadIdx.x;
  const int off = q_tab[q], n = q_tab[q + 1] - off;
  if (n < MIN_CORR) {  // the whole workgroup: nothing to sample from
    if (tid == 0) slots[blockIdx.x] = 0;
    return;
  }
  const double* qr = rows + ROW_DOUBLES * (long long)off;
  const double* cam = cams + 8 * (long long)q;
  const double fx = cam[0], fy = cam[1], cx = cam[2], cy = cam[3], k1 = cam[4];
  const int it = blk * RBLOCK + tid;
  double P[4][12];
  int nc = 0;
  if (it < iters) nc = candidates(seed, q, it, n, qr, P);
  if (nc == 0) {
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
      for (int i = 0; i < 12; ++i) P[r][i] = (double)NAN;  // scores nothing
  }
  int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
  for (int base = 0; base < n; base += RTILE) {
    __syncthreads();
    if (base + tid < n) {
      const double2* s = reinterpret_cast<const double2*>(qr + ROW_DOUBLES * (long long)(base + tid));
      const double2 xy = s[0], Xa = s[2], Xb = s[3];
      double2* t = reinterpret_cast<double2*>(tile + TILE_DOUBLES * tid);
      t[0] = make_double2((xy.x - cx) / fx, (xy.y - cy) / fy);
      t[1] = Xa;
      t[2] = make_double2(Xb.x, 0.0);
    }
    __syncthreads();
    const int lim = min(RTILE, n - base);
    for (int j = 0; j < lim; ++j) {
      const double2 a = *reinterpret_cast<const double2*>(tile + TILE_DOUBLES * j);
      const double2 b = *reinterpret_cast<const double2*>(tile + TILE_DOUBLES * j + 2);
      const double Z = tile[TILE_DOUBLES * j + 4];
      c0 += reproj_inlier(fx, fy, k1, P[0], a.x, a.y, b.x, b.y, Z, thr2) ? 1 : 0;
      c1 += reproj_inlier(fx, fy, k1, P[1], a.x, a.y, b.x, b.y, Z, thr2) ? 1 : 0;
      c2 += reproj_inlier(fx, fy, k1, P[2], a.x, a.y, b.x, b.y, Z, thr2) ? 1 : 0;
      c3 += reproj_inlier(fx, fy, k1, P[3], a.x, a.y, b.x, b.y, Z, thr2) ? 1 : 0;
    }
  }
  unsigned long long key = 0ull;
  if (nc > 0) key = slot_key_root(c0, it, 0);
  if (nc > 1) {
    const unsigned long long k = slot_key_root(c1, it, 1);
    key = k > key ? k : key;
  }
  if (nc > 2) {
    const unsigned long long k = slot_key_root(c2, it, 2);
    key = k > key ? k : key;
  }
  if (nc > 3) {
    const unsigned long long k = slot_key_root(c3, it, 3);
    key = k > key ? k : key;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = pf_shfl_xor(key, o, 64);
    key = other > key ? other : key;
  }
  if ((tid & 63) == 0) wbest[tid >> 6] = key;
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < RBLOCK / 64; ++w) key = wbest[w] > key ? wbest[w] : key;
    slots[blockIdx.x] = key;
  }
}

// the inlier test on a workspace row
__device__ __forceinline__ bool row_inlier(const double* cam, const double (&P)[12],
                                           const double* __restrict__ r, double thr2) {
  return reproj_inlier(cam[0], cam[1], cam[4], P, (r[0] - cam[2]) / cam[0], (r[1] - cam[3]) / cam[1],
                       r[4], r[5], r[6], thr2);
}

__global__ __launch_bounds__(256) void pose_select_kernel(
    const int32_t* __restrict__ q_tab, const double* __restrict__ cams,
    const double* __restrict__ rows, const unsigned long long* __restrict__ slots, int nblk,
    double thr2, uint64_t seed, double* __restrict__ poses, int* __restrict__ info,
    uint8_t* __restrict__ inlier) {
  __shared__ unsigned long long kred[RBLOCK];
  __shared__ int ired[RBLOCK];
  __shared__ double wsum[RBLOCK / 64][GN_ACC];
  const int q = blockIdx.x, tid = threadIdx.x;
  const int off = q_tab[q], n = q_tab[q + 1] - off;
  uint8_t* ip = inlier + off;
  unsigned long long mine = tid < nblk ? slots[(long long)q * nblk + tid] : 0ull;
  {  // the fixed-order tree of ransac_gather.h's block_reduce
    kred[tid] = mine;
    __syncthreads();
#pragma unroll
    for (int s = RBLOCK / 2; s > 0; s >>= 1) {
      if (tid < s) kred[tid] = kred[tid] > kred[tid + s] ? kred[tid] : kred[tid + s];
      __syncthreads();
    }
  }
  const unsigned long long key = kred[0];
  if ((key >> 32) == 0) {  // fewer than 4 correspondences, or every sample rejected
    for (int i = tid; i < n; i += RBLOCK) ip[i] = 0;
    if (tid < 12) poses[12 * (long long)q + tid] = 0.0;
    if (tid < 4) info[4 * (long long)q + tid] = tid == 0 ? 1 : (tid == 2 ? -1 : 0);
    return;
  }
  const int it = slot_key_iter(key), root = slot_key_rootidx(key);
  const double* qr = rows + ROW_DOUBLES * (long long)off;
  const double* cam = cams + 8 * (long long)q;
  double P0[12];
  {
    double Pc[4][12];
    candidates(seed, q, it, n, qr, Pc);  // every thread: the same operations, the same bits
#pragma unroll
    for (int i = 0; i < 12; ++i)
      P0[i] = root == 0 ? Pc[0][i] : (root == 1 ? Pc[1][i] : (root == 2 ? Pc[2][i] : Pc[3][i]));
  }
  auto count = [&](const double (&P)[12], bool write) {
    int c = 0;
    for (int i = tid; i < n; i += RBLOCK) {
      const bool in = row_inlier(cam, P, qr + ROW_DOUBLES * (long long)i, thr2);
      if (write) ip[i] = in ? 1 : 0;
      c += in ? 1 : 0;
    }
    __syncthreads();  // ired may still be read from the call before
    ired[tid] = c;
    __syncthreads();
#pragma unroll
    for (int s = RBLOCK / 2; s > 0; s >>= 1) {
      if (tid < s) ired[tid] = ired[tid] + ired[tid + s];
      __syncthreads();
    }
    return ired[0];
  };
  const int c0 = count(P0, true);  // each thread reads back only the flags it wrote
  // the sums of gn_row over the winner's inliers at the pose P: each thread over
  // its rows in ascending order, the xor butterfly inside the wave (every lane
  // ends with the same bits), then the four waves in order
  auto accumulate = [&](const double (&P)[12], double (&acc)[GN_ACC]) {
    gn_zero(acc);
    for (int i = tid; i < n; i += RBLOCK) {
      if (!ip[i]) continue;
      const double* r = qr + ROW_DOUBLES * (long long)i;
      gn_row(cam, P, r[0], r[1], r[4], r[5], r[6], acc);
    }
    __syncthreads();  // wsum may still be read from the call before
#pragma unroll
    for (int k = 0; k < GN_ACC; ++k) {
      double v = acc[k];
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) v = v + pf_shfl_xor(v, o, 64);
      if ((tid & 63) == 0) wsum[tid >> 6][k] = v;
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < GN_ACC; ++k) {
      double v = wsum[0][k];
#pragma unroll
      for (int w = 1; w < RBLOCK / 64; ++w) v = v + wsum[w][k];
      acc[k] = v;
    }
  };
  double P1[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) P1[i] = P0[i];
  bool keep = false;
  int c1 = 0;
  if (c0 >= GN_MIN_INLIERS) {  // the whole workgroup: c0 is the same everywhere
    gn_refit(P1, accumulate);
    double tot = 0.0;
#pragma unroll
    for (int i = 0; i < 12; ++i) tot = tot + P1[i];
    c1 = count(P1, false);
    keep = finite_d(tot) && c1 >= c0;
  }
  if (keep) count(P1, true);
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < 12; ++i) poses[12 * (long long)q + i] = keep ? P1[i] : P0[i];
    int* o = info + 4 * (long long)q;
    o[0] = 0, o[1] = keep ? c1 : c0, o[2] = it, o[3] = (keep ? 1 : 0) | (root << 8);
  }
}

}  // namespace

extern "C" int posfeat_pose_solve3(const double* m, double* poses) {
  if (!m || !poses) return POSFEAT_E_INVALID;
  double mm[3][5], P[4][12];
  for (int i = 0; i < 3; ++i)
    for (int k = 0; k < 5; ++k) mm[i][k] = m[5 * i + k];
  const int nc = pfpose::p3p(mm, P);
  for (int r = 0; r < nc; ++r)
    for (int i = 0; i < 12; ++i) poses[12 * r + i] = P[r][i];
  return nc;
}

extern "C" size_t posfeat_ransac_pose_workspace(const int32_t* q_off, int nq, int iters) {
  pfpose::Layout L;
  if (pfpose::layout(q_off, nq, iters, L) != 0) return 0;
  return L.total;
}

extern "C" int posfeat_ransac_pose(const float* kp, long long nkp, const double* cams,
                                   const double* points, long long npoints, const int32_t* corr,
                                   const int32_t* q_off, int nq, int iters, double thr,
                                   uint64_t seed, double* poses, int32_t* info, uint8_t* inlier,
                                   void* ws, size_t ws_bytes, void* stream) {
  pfpose::Layout L;
  if (pfpose::layout(q_off, nq, iters, L) != 0) return POSFEAT_E_INVALID;
  if (!kp || !cams || !points || !corr || !poses || !info || !inlier || !ws || nkp < 0 ||
      npoints < 0)
    return POSFEAT_E_INVALID;
  if (!(thr > 0.0) || !(thr < (double)INFINITY)) return POSFEAT_E_INVALID;
  if ((reinterpret_cast<uintptr_t>(ws) & 255) || (reinterpret_cast<uintptr_t>(poses) & 7) ||
      (reinterpret_cast<uintptr_t>(points) & 7) || (reinterpret_cast<uintptr_t>(cams) & 7) ||
      (reinterpret_cast<uintptr_t>(info) & 3) || (reinterpret_cast<uintptr_t>(corr) & 3))
    return POSFEAT_E_INVALID;
  if (ws_bytes < L.total) return POSFEAT_E_WORKSPACE;
  if (nq == 0) return POSFEAT_OK;
  hipStream_t st = pf_stream(stream);
  char* w = static_cast<char*>(ws);
  // the runtime has read a pageable source when the copy call returns (as
  // posfeat_ransac_homography relies on)
  if (hipMemcpyAsync(w + L.table, q_off, (size_t)(nq + 1) * 4, hipMemcpyHostToDevice, st) !=
      hipSuccess)
    return POSFEAT_E_HIP;
  const int32_t* q_tab = reinterpret_cast<const int32_t*>(w + L.table);
  double* rows = reinterpret_cast<double*>(w + L.rows);
  unsigned long long* slots = reinterpret_cast<unsigned long long*>(w + L.slots);
  const unsigned ggrid = (unsigned)((L.c + 255) / 256 > 0 ? (L.c + 255) / 256 : 1);
  hipLaunchKernelGGL(pose_gather_kernel, dim3(ggrid), dim3(256), 0, st, kp, nkp, cams, points,
                     npoints, corr, q_tab, nq, L.c, rows);
  PF_CHECK_LAUNCH();
  hipLaunchKernelGGL(pose_hyp_kernel, dim3((unsigned)(nq * L.nblk)), dim3(RBLOCK), 0, st, q_tab,
                     cams, rows, iters, L.nblk, thr * thr, seed, slots);
  PF_CHECK_LAUNCH();
  hipLaunchKernelGGL(pose_select_kernel, dim3(nq), dim3(RBLOCK), 0, st, q_tab, cams, rows, slots,
                     L.nblk, thr * thr, seed, poses, info, inlier);
  PF_CHECK_LAUNCH();
  return POSFEAT_OK;
}
