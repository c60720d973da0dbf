// fundamental.hip -- RANSAC fundamental matrices for every pair of a pair list,
// on gfx950: the epipolar counterpart of ransac.hip, on the same tables, the
// same workspace and the same three launches whatever the number of pairs:
//
//   ransac_gather_kernel  (ransac_gather.h, the homography stage's) the matched
//                         keypoints as compact fp32 rows and the two
//                         normalisations.
//   fund_hyp_kernel       one workgroup per (pair, block of 256 iterations),
//                         one sample per lane.  Phase 1: the lane draws seven
//                         matches (ransac_plan.h sample_k<7>), eliminates its
//                         7x9 system with full pivoting, solves the cubic and
//                         keeps up to three candidate matrices (27 doubles);
//                         the 63-double system is dead from there on.  Phase
//                         2: the pair's matches go through LDS in tiles of 256
//                         (as doubles, 8 KB; every lane reads the same address,
//                         a broadcast) and the lane scores its candidates
//                         against each staged match with the division-free
//                         Sampson test.  A wave then a block reduction of the
//                         (count, iteration, root) key fills the slot.
//   fund_select_kernel    one workgroup per pair: reduces the slots, rebuilds
//                         the winner from (iteration, root) with the same
//                         operations, marks its inliers, accumulates the upper
//                         triangle of the 9x9 normal matrix over them in a
//                         fixed order, runs the Jacobi eigen-solve (every lane
//                         the same rotations on the same matrix; lane l keeps
//                         row l mod 9 of the accumulated rotation, so the
//                         eigenvector is nine lane reads), projects to rank 2,
//                         recounts, applies the keep rule, writes F, info and
//                         the mask.
//
// All of the arithmetic is fundamental_solve.h, the text the host compiles for
// posfeat_fundamental_solve7.  Floating-point contraction is off for the whole
// file, so the hypothesis a lane builds and the one the select kernel rebuilds
// are the same operations; the Sampson test uses explicit fma.
#include <math.h>

#include <vector>

#include "common.h"
#include "ransac_plan.h"
#include "fundamental_solve.h"

#pragma clang fp contract(off)

namespace {

using namespace pfransac_plan;

static_assert(sizeof(Pair) == 32, "device table layout");
static_assert(RBLOCK == 256 && RTILE == 256, "one staged match per thread of a workgroup");

#include "ransac_gather.h"  // Norm, block_reduce, pair_count, ransac_gather_kernel, load_norm

// the candidates of iteration `it` of pair `pair`, denormalised; their number
// (0 for a rejected sample); the rows of F past it are NaN and score nothing
__device__ __forceinline__ int candidates(uint64_t seed, int pair, int it, int n,
                                          const float4* __restrict__ mp, const Norm& nm,
                                          double (&F)[3][9]) {
  int32_t idx[7];
  sample_k<7>(seed, pair, it, n, idx);
  double m[7][4];
  bool ok = true;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const float4 r = mp[idx[i]];
    ok = ok && r.x == r.x;  // a match outside its sets (a NaN row) rejects the sample
    m[i][0] = ((double)r.x - nm.cx1) * nm.s1, m[i][1] = ((double)r.y - nm.cy1) * nm.s1;
    m[i][2] = ((double)r.z - nm.cx2) * nm.s2, m[i][3] = ((double)r.w - nm.cy2) * nm.s2;
  }
  double fn[3][9];
  int nc = pffund::solve7(m, fn);
  nc = ok ? nc : 0;
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    pffund::denormalise(fn[r], nm.cx1, nm.cy1, nm.s1, nm.cx2, nm.cy2, nm.s2, F[r]);
    if (r >= nc) {
#pragma unroll
      for (int i = 0; i < 9; ++i) F[r][i] = (double)NAN;
    }
  }
  return nc;
}

__device__ __forceinline__ bool is_inlier(const double (&F)[9], const float4& m, double thr2) {
  return pffund::sampson_inlier(F, (double)m.x, (double)m.y, (double)m.z, (double)m.w, thr2);
}

__global__ __launch_bounds__(256) void fund_hyp_kernel(const Pair* __restrict__ tab,
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
  if (n < FMINSET) {  // the whole workgroup: nothing to sample from
    if (tid == 0) slots[blockIdx.x] = 0;
    return;
  }
  const float4* mp = pts + q.moff;
  const Norm nm = load_norm(norm, p);
  const int it = blk * RBLOCK + tid;
  double F[3][9];
  int nc = 0;
  if (it < iters) nc = candidates(seed, p, it, n, mp, nm, F);
  if (nc == 0) {
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int i = 0; i < 9; ++i) F[r][i] = (double)NAN;  // scores nothing
  }
  int c0 = 0, c1 = 0, c2 = 0;
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
      c0 += pffund::sampson_inlier(F[0], a.x, a.y, b.x, b.y, thr2) ? 1 : 0;
      c1 += pffund::sampson_inlier(F[1], a.x, a.y, b.x, b.y, thr2) ? 1 : 0;
      c2 += pffund::sampson_inlier(F[2], a.x, a.y, b.x, b.y, thr2) ? 1 : 0;
    }
  }
  unsigned long long key = 0ull;
  if (nc > 0) key = slot_key_root(c0, it, 0);
  if (nc > 1) {
    const unsigned long long k1 = slot_key_root(c1, it, 1);
    key = k1 > key ? k1 : key;
  }
  if (nc > 2) {
    const unsigned long long k2 = slot_key_root(c2, it, 2);
    key = k2 > key ? k2 : key;
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

__global__ __launch_bounds__(256) void fund_select_kernel(
    const Pair* __restrict__ tab, const float4* __restrict__ pts, const double* __restrict__ norm,
    const int* __restrict__ counts, const unsigned long long* __restrict__ slots, int nblk,
    double thr2, uint64_t seed, double* __restrict__ Fout, int* __restrict__ info,
    uint8_t* __restrict__ inlier) {
  __shared__ unsigned long long kred[RBLOCK];
  __shared__ int ired[RBLOCK];
  __shared__ double wsum[RBLOCK / 64][45];
  const int p = blockIdx.x, tid = threadIdx.x;
  const Pair q = tab[p];
  const int n = pair_count(counts, p, q);
  uint8_t* ip = inlier + q.moff;
  const unsigned long long mine = tid < nblk ? slots[(long long)p * nblk + tid] : 0ull;
  const unsigned long long key = block_reduce(mine, kred, OpMax());
  if ((key >> 32) == 0) {  // fewer than 7 matches, or every sample rejected
    for (int i = tid; i < q.n1; i += RBLOCK) ip[i] = 0;
    if (tid < 9) Fout[9 * (long long)p + tid] = 0.0;
    if (tid < 4) info[4 * (long long)p + tid] = tid == 0 ? 1 : (tid == 2 ? -1 : 0);
    return;
  }
  const int it = slot_key_iter(key), root = slot_key_rootidx(key);
  const float4* mp = pts + q.moff;
  const Norm nm = load_norm(norm, p);
  double F0[9];
  {
    double Fc[3][9];
    candidates(seed, p, it, n, mp, nm, Fc);  // every thread: the same operations, the same bits
#pragma unroll
    for (int i = 0; i < 9; ++i) F0[i] = root == 0 ? Fc[0][i] : (root == 1 ? Fc[1][i] : Fc[2][i]);
  }
  // inliers of the winner and the upper triangle of the normal matrix over
  // them, each thread over its rows in ascending order
  double a[9][9];
#pragma unroll
  for (int r = 0; r < 9; ++r)
#pragma unroll
    for (int c = r; c < 9; ++c) a[r][c] = 0.0;
  int c0 = 0;
  for (int i = tid; i < n; i += RBLOCK) {
    const float4 m = mp[i];
    const bool in = is_inlier(F0, m, thr2);
    ip[i] = in ? 1 : 0;
    if (!in) continue;
    ++c0;
    double row[9];
    pffund::epi_row(((double)m.x - nm.cx1) * nm.s1, ((double)m.y - nm.cy1) * nm.s1,
                    ((double)m.z - nm.cx2) * nm.s2, ((double)m.w - nm.cy2) * nm.s2, row);
#pragma unroll
    for (int r = 0; r < 9; ++r)
#pragma unroll
      for (int c = r; c < 9; ++c) a[r][c] = a[r][c] + row[r] * row[c];
  }
  c0 = block_reduce(c0, ired, OpAdd());
  // xor butterfly inside the wave (every lane ends with the same bits), then
  // the four waves in order
  {
    int k = 0;
#pragma unroll
    for (int r = 0; r < 9; ++r)
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
    for (int r = 0; r < 9; ++r)
#pragma unroll
      for (int c = r; c < 9; ++c, ++k) {
        double v = wsum[0][k];
#pragma unroll
        for (int w = 1; w < RBLOCK / 64; ++w) v = v + wsum[w][k];
        a[r][c] = v;
      }
  }
  // the eigenvector of the smallest eigenvalue: lane l holds row l mod 9 of
  // the rotation, lanes 0..8 of each wave hand over the column's entries
  double F1[9];
  {
    double v[1][9];
    const int myrow = (tid & 63) % 9;
#pragma unroll
    for (int j = 0; j < 9; ++j) v[0][j] = j == myrow ? 1.0 : 0.0;
    pffund::jacobi_sym<9, 1>(a, v);
    const int jm = pffund::min_diag<9>(a);
    double e = 0.0;
#pragma unroll
    for (int j = 0; j < 9; ++j) e = jm == j ? v[0][j] : e;
    double fn[9];
#pragma unroll
    for (int r = 0; r < 9; ++r) fn[r] = pf_shfl(e, r, 64);
    pffund::rank2(fn);
    pffund::denormalise(fn, nm.cx1, nm.cy1, nm.s1, nm.cx2, nm.cy2, nm.s2, F1);
  }
  double ss1 = 0.0;
#pragma unroll
  for (int i = 0; i < 9; ++i) ss1 = ss1 + F1[i] * F1[i];
  // fewer than 8 inliers leave the 8-point fit under-determined: no refit
  const bool ok1 = c0 >= 8 && ss1 > 0.0 && ss1 < (double)INFINITY;
  int c1 = 0;
  for (int i = tid; i < n; i += RBLOCK) c1 += is_inlier(F1, mp[i], thr2) ? 1 : 0;
  c1 = block_reduce(c1, ired, OpAdd());
  const bool keep = ok1 && c1 >= c0;
  if (keep)
    for (int i = tid; i < n; i += RBLOCK) ip[i] = is_inlier(F1, mp[i], thr2) ? 1 : 0;
  for (int i = n + tid; i < q.n1; i += RBLOCK) ip[i] = 0;
  if (tid == 0) {
#pragma unroll
    for (int i = 0; i < 9; ++i) F0[i] = keep ? F1[i] : F0[i];
    pffund::unit_sign(F0);
#pragma unroll
    for (int i = 0; i < 9; ++i) Fout[9 * (long long)p + i] = F0[i];
    int* o = info + 4 * (long long)p;
    o[0] = 0, o[1] = keep ? c1 : c0, o[2] = it, o[3] = (keep ? 1 : 0) | (root << 8);
  }
}

}  // namespace

extern "C" int posfeat_ransac_sample_k(uint64_t seed, int pair, int iter, int n, int k,
                                       int32_t* out) {
  if (!out || k < 4 || k > 8 || n < k || pair < 0 || iter < 0) return POSFEAT_E_INVALID;
  switch (k) {
    case 4: pfransac_plan::sample_k<4>(seed, pair, iter, n, *reinterpret_cast<int32_t(*)[4]>(out)); break;
    case 5: pfransac_plan::sample_k<5>(seed, pair, iter, n, *reinterpret_cast<int32_t(*)[5]>(out)); break;
    case 6: pfransac_plan::sample_k<6>(seed, pair, iter, n, *reinterpret_cast<int32_t(*)[6]>(out)); break;
    case 7: pfransac_plan::sample_k<7>(seed, pair, iter, n, *reinterpret_cast<int32_t(*)[7]>(out)); break;
    default: pfransac_plan::sample_k<8>(seed, pair, iter, n, *reinterpret_cast<int32_t(*)[8]>(out)); break;
  }
  return POSFEAT_OK;
}

extern "C" int posfeat_fundamental_solve7(const double* m, double* F) {
  if (!m || !F) return POSFEAT_E_INVALID;
  double mm[7][4], fn[3][9];
  for (int i = 0; i < 7; ++i)
    for (int k = 0; k < 4; ++k) mm[i][k] = m[4 * i + k];
  int nc = pffund::solve7(mm, fn);
  for (int r = 0; r < nc; ++r)
    if (!pffund::unit_sign(fn[r])) nc = 0;
  for (int r = 0; r < nc; ++r)
    for (int i = 0; i < 9; ++i) F[9 * r + i] = fn[r][i];
  return nc;
}

extern "C" size_t posfeat_ransac_fundamental_workspace(const int32_t* set_off, int nsets,
                                                       const int32_t* pairs, int npairs,
                                                       int iters) {
  Plan pl;
  if (nsets <= 0 || npairs <= 0 ||
      build_plan_fundamental(set_off, nsets, pairs, npairs, iters, pl) != 0)
    return 0;
  return pl.total_bytes;
}

extern "C" int posfeat_ransac_fundamental(const float* kp, const int32_t* set_off, int nsets,
                                          const int32_t* pairs, int npairs, const int32_t* matches,
                                          const int32_t* counts, int iters, double thr,
                                          uint64_t seed, double* F, int32_t* info, uint8_t* inlier,
                                          void* ws, size_t ws_bytes, void* stream) {
  if (!kp || !set_off || !pairs || !matches || !counts || !F || !info || !inlier || !ws ||
      nsets <= 0 || npairs <= 0)
    return POSFEAT_E_INVALID;
  if (!(thr > 0.0) || !(thr < (double)INFINITY)) return POSFEAT_E_INVALID;
  if ((reinterpret_cast<uintptr_t>(ws) & 255) || (reinterpret_cast<uintptr_t>(F) & 7) ||
      (reinterpret_cast<uintptr_t>(info) & 3))
    return POSFEAT_E_INVALID;
  Plan pl;
  if (build_plan_fundamental(set_off, nsets, pairs, npairs, iters, pl) != 0)
    return POSFEAT_E_INVALID;
  if ((int64_t)npairs * pl.nblk > INT32_MAX) return POSFEAT_E_INVALID;
  if (ws_bytes < pl.total_bytes) return POSFEAT_E_WORKSPACE;
  hipStream_t st = pf_stream(stream);
  char* w = static_cast<char*>(ws);
  // the runtime has read a pageable source when the copy call returns (as
  // posfeat_ransac_homography relies on), so the plan may die with us
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
  hipLaunchKernelGGL(fund_hyp_kernel, dim3((unsigned)(npairs * pl.nblk)), dim3(RBLOCK), 0, st, tab,
                     pts, norm, counts, iters, pl.nblk, thr * thr, seed, slots);
  PF_CHECK_LAUNCH();
  hipLaunchKernelGGL(fund_select_kernel, dim3(npairs), dim3(RBLOCK), 0, st, tab, pts, norm, counts,
                     slots, pl.nblk, thr * thr, seed, F, info, inlier);
  PF_CHECK_LAUNCH();
  return POSFEAT_OK;
}
