// ransac.hip -- RANSAC homographies for every pair of a pair list, on gfx950.
//
// The stage after posfeat_match_pairs (matchpairs.hip): the matches of the
// whole list, as that call left them on the device, go through three launches
// whatever the number of pairs:
//
//   ransac_gather_kernel  (ransac_gather.h, shared with fundamental.hip) one
//                         workgroup per pair: the matched keypoints
//                         gathered into a compact (x1 y1 x2 y2) fp32 row per
//                         match, and the two normalisations (centroid, mean
//                         distance sqrt 2) reduced in fp64 in a fixed order.
//   ransac_hyp_kernel     one workgroup per (pair, block of 256 iterations),
//                         one hypothesis per lane: the lane draws its sample
//                         (ransac_plan.h sample4), runs the degeneracy test and
//                         solves its 8x8 system in registers, all fp64; the
//                         workgroup then stages the pair's matches through LDS
//                         in tiles of 256 (as doubles, 8 KB) and every lane
//                         scores its own H against each staged match -- all
//                         lanes read one LDS address, a broadcast.  A wave then
//                         a block reduction of (count, lowest iteration) fills
//                         the (pair, block) slot.
//   ransac_select_kernel  one workgroup per pair: reduces the slots, rebuilds
//                         the winner from its iteration index, marks its
//                         inliers, accumulates the 8x8 normal equations over
//                         them in a fixed order, solves, recounts, keeps the
//                         refit iff it has at least as many inliers, and
//                         writes H, info and the inlier mask.
//
// The solver's arrays are indexed by compile-time constants only (every loop
// fully unrolled, the pivot row swapped in by selects), so they live in
// registers.  Floating-point contraction is off for the whole file: the
// hypothesis a lane builds in ransac_hyp_kernel and the one
// ransac_select_kernel rebuilds are the same operations; the residual uses
// explicit fma.
#include <math.h>

#include <vector>

#include "common.h"
#include "ransac_plan.h"

#pragma clang fp contract(off)

namespace {

using namespace pfransac_plan;

static_assert(sizeof(Pair) == 32, "device table layout");
static_assert(RBLOCK == 256 && RTILE == 256, "one staged match per thread of a workgroup");

#include "ransac_gather.h"  // Norm, block_reduce, pair_count, ransac_gather_kernel, load_norm

// Gaussian elimination with partial pivoting on the augmented 8x9 system, in
// place; x = the solution.  False when a pivot is below 1e-12 times the largest
// entry of its column of the system as given (or is not a positive number).
__device__ __forceinline__ bool solve8(double (&a)[8][9], double (&x)[8]) {
  double cmax[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    cmax[c] = fabs(a[0][c]);
#pragma unroll
    for (int r = 1; r < 8; ++r) cmax[c] = fmax(cmax[c], fabs(a[r][c]));
  }
  bool ok = true;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    int piv = c;  // the first row holding the largest |a[r][c]|, r >= c
    double best = fabs(a[c][c]);
#pragma unroll
    for (int r = c + 1; r < 8; ++r) {
      const double v = fabs(a[r][c]);
      if (v > best) {
        best = v;
        piv = r;
      }
    }
#pragma unroll
    for (int r = c + 1; r < 8; ++r) {
      const bool sw = piv == r;
#pragma unroll
      for (int k = c; k < 9; ++k) {
        const double t = a[c][k], u = a[r][k];
        a[c][k] = sw ? u : t;
        a[r][k] = sw ? t : u;
      }
    }
    ok = ok && best >= 1e-12 * cmax[c] && best > 0.0;
#pragma unroll
    for (int r = c + 1; r < 8; ++r) {
      const double f = a[r][c] / a[c][c];
#pragma unroll
      for (int k = c + 1; k < 9; ++k) a[r][k] = a[r][k] - f * a[c][k];
    }
  }
#pragma unroll
  for (int c = 7; c >= 0; --c) {
    double s = a[c][8];
#pragma unroll
    for (int k = c + 1; k < 8; ++k) s = s - a[c][k] * x[k];
    x[c] = s / a[c][c];
  }
  return ok;
}

// H = T2^-1 Hn T1 with Hn = (x[0..7], 1)
__device__ __forceinline__ void denormalise(const double (&x)[8], const Norm& nm, double (&H)[9]) {
  const double hn[9] = {x[0], x[1], x[2], x[3], x[4], x[5], x[6], x[7], 1.0};
  double m[9];
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    m[3 * r] = hn[3 * r] * nm.s1;
    m[3 * r + 1] = hn[3 * r + 1] * nm.s1;
    m[3 * r + 2] = hn[3 * r + 2] - nm.s1 * (hn[3 * r] * nm.cx1 + hn[3 * r + 1] * nm.cy1);
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    H[c] = m[c] / nm.s2 + nm.cx2 * m[6 + c];
    H[3 + c] = m[3 + c] / nm.s2 + nm.cy2 * m[6 + c];
    H[6 + c] = m[6 + c];
  }
}

// the triple (i, j, k) is in general position in both images, the same way round
__device__ __forceinline__ bool triple_ok(const float4& pi, const float4& pj, const float4& pk) {
  const double ax = (double)pj.x - (double)pi.x, ay = (double)pj.y - (double)pi.y;
  const double bx = (double)pk.x - (double)pi.x, by = (double)pk.y - (double)pi.y;
  const double c1 = ax * by - ay * bx;
  const double l1 = 1e-6 * sqrt(ax * ax + ay * ay) * sqrt(bx * bx + by * by);
  const double ux = (double)pj.z - (double)pi.z, uy = (double)pj.w - (double)pi.w;
  const double vx = (double)pk.z - (double)pi.z, vy = (double)pk.w - (double)pi.w;
  const double c2 = ux * vy - uy * vx;
  const double l2 = 1e-6 * sqrt(ux * ux + uy * uy) * sqrt(vx * vx + vy * vy);
  return fabs(c1) > l1 && fabs(c2) > l2 && ((c1 > 0.0) == (c2 > 0.0));
}

// the two rows of the h33 = 1 system of one correspondence, normalised
__device__ __forceinline__ void dlt_rows(const float4& m, const Norm& nm, double (&r1)[9],
                                         double (&r2)[9]) {
  const double x = ((double)m.x - nm.cx1) * nm.s1, y = ((double)m.y - nm.cy1) * nm.s1;
  const double u = ((double)m.z - nm.cx2) * nm.s2, v = ((double)m.w - nm.cy2) * nm.s2;
  r1[0] = x, r1[1] = y, r1[2] = 1.0, r1[3] = 0.0, r1[4] = 0.0, r1[5] = 0.0;
  r1[6] = -(u * x), r1[7] = -(u * y), r1[8] = u;
  r2[0] = 0.0, r2[1] = 0.0, r2[2] = 0.0, r2[3] = x, r2[4] = y, r2[5] = 1.0;
  r2[6] = -(v * x), r2[7] = -(v * y), r2[8] = v;
}

// the hypothesis of iteration `it` of pair `pair`; false for a rejected sample
__device__ __forceinline__ bool hypothesis(uint64_t seed, int pair, int it, int n,
                                           const float4* __restrict__ mp, const Norm& nm,
                                           double (&H)[9]) {
  int32_t idx[4];
  sample4(seed, pair, it, n, idx);
  const float4 m0 = mp[idx[0]], m1 = mp[idx[1]], m2 = mp[idx[2]], m3 = mp[idx[3]];
  bool ok = triple_ok(m0, m1, m2) && triple_ok(m0, m1, m3) && triple_ok(m0, m2, m3) &&
            triple_ok(m1, m2, m3);
  double a[8][9], x[8];
  dlt_rows(m0, nm, a[0], a[1]);
  dlt_rows(m1, nm, a[2], a[3]);
  dlt_rows(m2, nm, a[4], a[5]);
  dlt_rows(m3, nm, a[6], a[7]);
  ok = solve8(a, x) && ok;
  denormalise(x, nm, H);
  return ok;
}

// the residual test of posfeat_reproj_hist without its division:
// |(u, v) - (px, py) / pz| <= thr  <=>  |(u, v) pz - (px, py)|^2 <= thr^2 pz^2
__device__ __forceinline__ bool is_inlier(const double (&H)[9], double x, double y, double u,
                                          double v, double thr2) {
  const double px = __builtin_fma(H[0], x, __builtin_fma(H[1], y, H[2]));
  const double py = __builtin_fma(H[3], x, __builtin_fma(H[4], y, H[5]));
  const double pz = __builtin_fma(H[6], x, __builtin_fma(H[7], y, H[8]));
  const double ex = __builtin_fma(u, pz, -px), ey = __builtin_fma(v, pz, -py);
  const double d2 = __builtin_fma(ex, ex, ey * ey), lim = thr2 * (pz * pz);
  return d2 <= lim && lim < (double)INFINITY && pz != 0.0;  // NaN fails every test
}
__device__ __forceinline__ bool is_inlier(const double (&H)[9], const float4& m, double thr2) {
  return is_inlier(H, (double)m.x, (double)m.y, (double)m.z, (double)m.w, thr2);
}

// key of a scored hypothesis: more inliers first, then the lower iteration; 0
// for a rejected sample
__device__ __forceinline__ unsigned long long hyp_key(int cnt, int it) {
  return ((unsigned long long)(unsigned)(cnt + 1) << 32) | (0xffffffffu - (unsigned)it);
}

__global__ __launch_bounds__(256) void ransac_hyp_kernel(const Pair* __restrict__ tab,
                                                         const float4* __restrict__ pts,
                                                         const double* __restrict__ norm,
                                                         const int* __restrict__ counts, int iters,
                                                         int nblk, double thr2, uint64_t seed,
                                                         unsigned long long* __restrict__ slots) {
  __shared__ __attribute__((aligned(16))) double tile[RTILE * 4];  // 8 KB
  __shared__ unsigned long long wbest[RBLOCK / 64];
  const int p = blockIdx.x / nblk, blk = blockIdx.x - p * nblk, tid = threadIdx.x;
  const Pair q = tab[p];
  const int n = pair_count(counts, p, q);
  if (n < 4) {  // the whole workgroup: nothing to sample from
    if (tid == 0) slots[blockIdx.x] = 0;
    return;
  }
  const float4* mp = pts + q.moff;
  const Norm nm = load_norm(norm, p);
  const int it = blk * RBLOCK + tid;
  double H[9];
  bool valid = false;
  if (it < iters) valid = hypothesis(seed, p, it, n, mp, nm, H);
  if (!valid) {
#pragma unroll
    for (int i = 0; i < 9; ++i) H[i] = (double)NAN;  // scores nothing
  }
  int cnt = 0;
  for (int base = 0; base < n; base += RTILE) {
    __syncthreads();
    if (base + tid < n) {
      const float4 m = mp[base + tid];
      double2* t = reinterpret_cast<double2*>(tile + 4 * tid);
      t[0] = make_double2((double)m.x, (double)m.y);
      t[1] = make_double2((double)m.z, (double)m.w);
    }
    __syncthreads();
    const int lim = min(RTILE, n - base);
    for (int j = 0; j < lim; ++j) {
      const double2 a = *reinterpret_cast<const double2*>(tile + 4 * j);
      const double2 b = *reinterpret_cast<const double2*>(tile + 4 * j + 2);
      cnt += is_inlier(H, a.x, a.y, b.x, b.y, thr2) ? 1 : 0;
    }
  }
  unsigned long long key = valid ? hyp_key(cnt, it) : 0ull;
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

__global__ __launch_bounds__(256) void ransac_select_kernel(
    const Pair* __restrict__ tab, const float4* __restrict__ pts, const double* __restrict__ norm,
    const int* __restrict__ counts, const unsigned long long* __restrict__ slots, int nblk,
    double thr2, uint64_t seed, double* __restrict__ Hout, int* __restrict__ info,
    uint8_t* __restrict__ inlier) {
  __shared__ unsigned long long kred[RBLOCK];
  __shared__ int ired[RBLOCK];
  __shared__ double wsum[RBLOCK / 64][44];
  const int p = blockIdx.x, tid = threadIdx.x;
  const Pair q = tab[p];
  const int n = pair_count(counts, p, q);
  uint8_t* ip = inlier + q.moff;
  const unsigned long long mine = tid < nblk ? slots[(long long)p * nblk + tid] : 0ull;
  const unsigned long long key = block_reduce(mine, kred, OpMax());
  if ((key >> 32) == 0) {  // fewer than 4 matches, or every sample rejected
    for (int i = tid; i < q.n1; i += RBLOCK) ip[i] = 0;
    if (tid < 9) Hout[9 * (long long)p + tid] = 0.0;
    if (tid < 4) info[4 * (long long)p + tid] = tid == 0 ? 1 : (tid == 2 ? -1 : 0);
    return;
  }
  const int it = (int)(0xffffffffu - (unsigned)key);
  const float4* mp = pts + q.moff;
  const Norm nm = load_norm(norm, p);
  double H0[9];
  hypothesis(seed, p, it, n, mp, nm, H0);  // every thread: the same operations, the same bits
  // inliers of the winner and the normal equations over them (upper triangle
  // and right-hand side), each thread over its rows in ascending order
  double a[8][9];
#pragma unroll
  for (int r = 0; r < 8; ++r)
#pragma unroll
    for (int c = 0; c < 9; ++c) a[r][c] = 0.0;
  int c0 = 0;
  for (int i = tid; i < n; i += RBLOCK) {
    const float4 m = mp[i];
    const bool in = is_inlier(H0, m, thr2);
    ip[i] = in ? 1 : 0;
    if (!in) continue;
    ++c0;
    double r1[9], r2[9];
    dlt_rows(m, nm, r1, r2);
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int c = r; c < 9; ++c) a[r][c] = a[r][c] + (r1[r] * r1[c] + r2[r] * r2[c]);
  }
  c0 = block_reduce(c0, ired, OpAdd());
  // xor butterfly inside the wave (every lane ends with the same bits), then
  // the four waves in order
  {
    int k = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int c = r; c < 9; ++c, ++k) {
        double v = a[r][c];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v = v + pf_shfl_xor(v, o, 64);
        if ((tid & 63) == 0) wsum[tid >> 6][k] = v;
      }
    __syncthreads();
    k = 0;
#pragma unroll
    for (int r = 0; r < 8; ++r)
#pragma unroll
      for (int c = r; c < 9; ++c, ++k) {
        double v = wsum[0][k];
#pragma unroll
        for (int w = 1; w < RBLOCK / 64; ++w) v = v + wsum[w][k];
        a[r][c] = v;
      }
#pragma unroll
    for (int r = 1; r < 8; ++r)
#pragma unroll
      for (int c = 0; c < r; ++c) a[r][c] = a[c][r];
  }
  double x[8], H1[9];
  const bool ok1 = solve8(a, x);
  denormalise(x, nm, H1);
  int c1 = 0;
  for (int i = tid; i < n; i += RBLOCK) c1 += is_inlier(H1, mp[i], thr2) ? 1 : 0;
  c1 = block_reduce(c1, ired, OpAdd());
  const bool keep = ok1 && c1 >= c0;
  if (keep)
    for (int i = tid; i < n; i += RBLOCK) ip[i] = is_inlier(H1, mp[i], thr2) ? 1 : 0;
  for (int i = n + tid; i < q.n1; i += RBLOCK) ip[i] = 0;
  if (tid == 0) {
    double ss = 0.0;
#pragma unroll
    for (int i = 0; i < 9; ++i) {
      H0[i] = keep ? H1[i] : H0[i];
      ss = ss + H0[i] * H0[i];
    }
    const double sc = (H0[8] >= 0.0 ? 1.0 : -1.0) / sqrt(ss);
#pragma unroll
    for (int i = 0; i < 9; ++i) Hout[9 * (long long)p + i] = H0[i] * sc;
    int* o = info + 4 * (long long)p;
    o[0] = 0, o[1] = keep ? c1 : c0, o[2] = it, o[3] = keep ? 1 : 0;
  }
}

}  // namespace

extern "C" int posfeat_ransac_sample(uint64_t seed, int pair, int iter, int n, int32_t out4[4]) {
  if (!out4 || n < 4 || pair < 0 || iter < 0) return POSFEAT_E_INVALID;
  pfransac_plan::sample4(seed, pair, iter, n, out4);
  return POSFEAT_OK;
}

extern "C" size_t posfeat_ransac_homography_workspace(const int32_t* set_off, int nsets,
                                                      const int32_t* pairs, int npairs,
                                                      int iters) {
  Plan pl;
  if (nsets <= 0 || npairs <= 0 || build_plan(set_off, nsets, pairs, npairs, iters, pl) != 0)
    return 0;
  return pl.total_bytes;
}

extern "C" int posfeat_ransac_homography(const float* kp, const int32_t* set_off, int nsets,
                                         const int32_t* pairs, int npairs, const int32_t* matches,
                                         const int32_t* counts, int iters, double thr,
                                         uint64_t seed, double* H, int32_t* info, uint8_t* inlier,
                                         void* ws, size_t ws_bytes, void* stream) {
  if (!kp || !set_off || !pairs || !matches || !counts || !H || !info || !inlier || !ws ||
      nsets <= 0 || npairs <= 0)
    return POSFEAT_E_INVALID;
  if (!(thr > 0.0) || !(thr < (double)INFINITY)) return POSFEAT_E_INVALID;
  if ((reinterpret_cast<uintptr_t>(ws) & 255) || (reinterpret_cast<uintptr_t>(H) & 7) ||
      (reinterpret_cast<uintptr_t>(info) & 3))
    return POSFEAT_E_INVALID;
  Plan pl;
  if (build_plan(set_off, nsets, pairs, npairs, iters, pl) != 0) return POSFEAT_E_INVALID;
  if ((int64_t)npairs * pl.nblk > INT32_MAX) return POSFEAT_E_INVALID;
  if (ws_bytes < pl.total_bytes) return POSFEAT_E_WORKSPACE;
  hipStream_t st = pf_stream(stream);
  char* w = static_cast<char*>(ws);
  // the runtime has read a pageable source when the copy call returns (as
  // posfeat_match_pairs relies on), so the plan may die with us
  if (hipMemcpyAsync(w, pl.tab.data(), pl.tab.size() * sizeof(Pair), hipMemcpyHostToDevice, st) !=
      hipSuccess)
    return POSFEAT_E_HIP;
  const Pair* tab = reinterpret_cast<const Pair*>(w);
  float4* pts = reinterpret_cast<float4*>(w + pl.pts_off);
  double* norm = reinterpret_cast<double*>(w + pl.norm_off);
  unsigned long long* slots = reinterpret_cast<unsigned long long*>(w + pl.slot_off);
  hipLaunchKernelGGL(ransac_gather_kernel, dim3(npairs), dim3(RBLOCK), 0, st, kp, tab, matches,
                     counts, pts, norm);
  PF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ransac_hyp_kernel, dim3((unsigned)(npairs * pl.nblk)), dim3(RBLOCK), 0, st,
                     tab, pts, norm, counts, iters, pl.nblk, thr * thr, seed, slots);
  PF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ransac_select_kernel, dim3(npairs), dim3(RBLOCK), 0, st, tab, pts, norm,
                     counts, slots, pl.nblk, thr * thr, seed, H, info, inlier);
  PF_CHECK_LAUNCH();
  return POSFEAT_OK;
}
