// essential.hip -- five-point RANSAC essential matrices and relative poses for
// every calibrated pair of a pair list, on gfx950: the counterpart of
// fundamental.hip between two cameras with known intrinsics, on the same Pair
// table, in four launches whatever the number of pairs:
//
//   ess_gather_kernel  one workgroup per pair: the matched keypoints,
//                      undistorted on both sides (pftri::undistort), as fp64
//                      rows (x, y, u, v) in normalised camera coordinates; a
//                      match outside its sets or with a non-finite point is a
//                      NaN row.
//   ess_solve_kernel   one workgroup per (pair, block of 256 iterations), one
//                      sample per lane: five matches (sample_k<5>), the
//                      five-point solve of essential_solve.h, whose 10x20
//                      system and run-time pivoting live in private memory.
//                      The lane's real candidates leave as records (iteration
//                      << 4 | root, E[9]) packed behind those of the lower
//                      lanes of its block, so the record order is fixed.
//   ess_score_kernel   one workgroup per (pair, block, 256 records), one
//                      record per lane with E in registers: the pair's rows go
//                      through LDS in tiles of RTILE (8 KB, read as a
//                      broadcast) and the lane counts the division-free
//                      Sampson inliers of its candidate.  A wave then a block
//                      reduction of the (count, iteration, root) key fills the
//                      slot; a workgroup past its block's records writes 0.
//   ess_select_kernel  one workgroup per pair: reduces the slots, fetches the
//                      winner's record, marks its inliers, accumulates the 9x9
//                      normal matrix in a fixed order, runs the Jacobi
//                      eigen-solve as fund_select_kernel does, projects onto
//                      the essential manifold, recounts, applies the keep rule,
//                      decomposes, counts the matches in front of both cameras
//                      for the four poses and writes every output.
//
// Floating-point contraction is off for the whole file; the Sampson test uses
// explicit fma (pffund::sampson_inlier).
#include <math.h>

#include <vector>

#include "common.h"
#include "ransac_plan.h"
#include "essential_solve.h"

#pragma clang fp contract(off)

namespace {

using namespace pfransac_plan;

static_assert(sizeof(Pair) == 32, "device table layout");
static_assert(RBLOCK == 256 && RTILE == 256, "one staged match per thread of a workgroup");

struct Rec {  // EREC_DOUBLES doubles
  unsigned long long id;  // iteration << 4 | root
  double E[9];
};
static_assert(sizeof(Rec) == EREC_DOUBLES * 8, "record layout");

// fixed-order tree over the 256 threads; every thread gets the result
template <class T, class Op>
__device__ __forceinline__ T block_reduce(T v, T* red, Op op) {
  const int tid = threadIdx.x;
  __syncthreads();  // red may still be read from the call before
  red[tid] = v;
  __syncthreads();
#pragma unroll
  for (int s = RBLOCK / 2; s > 0; s >>= 1) {
    if (tid < s) red[tid] = op(red[tid], red[tid + s]);
    __syncthreads();
  }
  return red[0];
}
struct OpAdd {
  template <class T>
  __device__ T operator()(T a, T b) const { return a + b; }
};
struct OpMax {
  template <class T>
  __device__ T operator()(T a, T b) const { return a > b ? a : b; }
};

__device__ __forceinline__ int pair_count(const int* __restrict__ counts, int p, const Pair& q) {
  return max(0, min(counts[p], q.n1));
}

__device__ __forceinline__ double pair_thr2(const double* __restrict__ cams, const Pair& q,
                                            double thr) {
  return pfess::thr_norm2(cams + 8 * (long long)q.pad[0], cams + 8 * (long long)q.pad[1], thr);
}

__global__ __launch_bounds__(256) void ess_gather_kernel(const float* __restrict__ kp,
                                                         const double* __restrict__ cams,
                                                         const Pair* __restrict__ tab,
                                                         const int* __restrict__ matches,
                                                         const int* __restrict__ counts,
                                                         double* __restrict__ rows) {
  const int p = blockIdx.x, tid = threadIdx.x;
  const Pair q = tab[p];
  const int n = pair_count(counts, p, q);
  const int* mp = matches + 2 * (long long)q.moff;
  double* op = rows + 4 * (long long)q.moff;
  const double* cam1 = cams + 8 * (long long)q.pad[0];
  const double* cam2 = cams + 8 * (long long)q.pad[1];
  for (int i = tid; i < n; i += RBLOCK) {
    const int ia = mp[2 * i], ib = mp[2 * i + 1];
    double x = (double)NAN, y = (double)NAN, u = (double)NAN, v = (double)NAN;
    if ((unsigned)ia < (unsigned)q.n1 && (unsigned)ib < (unsigned)q.n2) {
      const float* pa = kp + 2 * ((long long)q.a_off + ia);
      const float* pb = kp + 2 * ((long long)q.b_off + ib);
      pftri::undistort(cam1, (double)pa[0], (double)pa[1], x, y);
      pftri::undistort(cam2, (double)pb[0], (double)pb[1], u, v);
      if (!(pffund::finite_d(x) && pffund::finite_d(y) && pffund::finite_d(u) &&
            pffund::finite_d(v)))
        x = y = u = v = (double)NAN;
    }
    double2* o = reinterpret_cast<double2*>(op + 4 * (long long)i);
    o[0] = make_double2(x, y);
    o[1] = make_double2(u, v);
  }
}

__global__ __launch_bounds__(256) void ess_solve_kernel(const Pair* __restrict__ tab,
                                                        const double* __restrict__ rows,
                                                        const int* __restrict__ counts, int iters,
                                                        int nblk, uint64_t seed,
                                                        int* __restrict__ cnt,
                                                        Rec* __restrict__ recs) {
  __shared__ int lc[RBLOCK];
  const int p = blockIdx.x / nblk, blk = blockIdx.x - p * nblk, tid = threadIdx.x;
  const Pair q = tab[p];
  const int n = pair_count(counts, p, q);
  if (n < EMINSET) {  // the whole workgroup: nothing to sample from
    if (tid == 0) cnt[blockIdx.x] = 0;
    return;
  }
  const double* mp = rows + 4 * (long long)q.moff;
  const int it = blk * RBLOCK + tid;
  double E[pfess::MAXCAND][9];
  int nc = 0;
  if (it < iters) {
    int32_t idx[5];
    sample_k<5>(seed, p, it, n, idx);
    double m[5][4];
    bool ok = true;
    for (int i = 0; i < 5; ++i) {
      const double2 a = *reinterpret_cast<const double2*>(mp + 4 * (long long)idx[i]);
      const double2 b = *reinterpret_cast<const double2*>(mp + 4 * (long long)idx[i] + 2);
      ok = ok && a.x == a.x;  // a NaN row rejects the sample
      m[i][0] = a.x, m[i][1] = a.y, m[i][2] = b.x, m[i][3] = b.y;
    }
    if (ok) nc = pfess::solve5(m, E);
  }
  lc[tid] = nc;
  __syncthreads();
  int off = 0;
  for (int l = 0; l < tid; ++l) off += lc[l];
  Rec* out = recs + (long long)blockIdx.x * EBLOCK_RECS + off;
  for (int r = 0; r < nc; ++r) {
    out[r].id = ((unsigned long long)(unsigned)it << 4) | (unsigned)r;
    for (int k = 0; k < 9; ++k) out[r].E[k] = E[r][k];
  }
  if (tid == RBLOCK - 1) cnt[blockIdx.x] = off + nc;
}

__global__ __launch_bounds__(256) void ess_score_kernel(const Pair* __restrict__ tab,
                                                        const double* __restrict__ rows,
                                                        const double* __restrict__ cams,
                                                        const int* __restrict__ counts,
                                                        const int* __restrict__ cnt,
                                                        const Rec* __restrict__ recs, int nblk,
                                                        double thr,
                                                        unsigned long long* __restrict__ slots) {
  __shared__ __attribute__((aligned(16))) double tile[RTILE * 4];  // 8 KB
  __shared__ unsigned long long wbest[RBLOCK / 64];
  const int hb = blockIdx.x / ESUB, sub = blockIdx.x - hb * ESUB, tid = threadIdx.x;
  const int nrec = cnt[hb];
  if (sub * RBLOCK >= nrec) {  // the whole workgroup: no record of its own
    if (tid == 0) slots[blockIdx.x] = 0;
    return;
  }
  const int p = hb / nblk;
  const Pair q = tab[p];
  const int n = pair_count(counts, p, q);
  const double thr2 = pair_thr2(cams, q, thr);
  const double* mp = rows + 4 * (long long)q.moff;
  const int ri = sub * RBLOCK + tid;
  const bool valid = ri < nrec;
  double E[9];
  unsigned id = 0;
  {
    const Rec* r = recs + (long long)hb * EBLOCK_RECS + (valid ? ri : 0);
    id = (unsigned)r->id;
#pragma unroll
    for (int k = 0; k < 9; ++k) E[k] = valid ? r->E[k] : (double)NAN;  // NaN scores nothing
  }
  int c = 0;
  for (int base = 0; base < n; base += RTILE) {
    __syncthreads();
    if (base + tid < n) {
      const double2* s = reinterpret_cast<const double2*>(mp + 4 * (long long)(base + tid));
      double2* t = reinterpret_cast<double2*>(tile + 4 * tid);
      t[0] = s[0];
      t[1] = s[1];
    }
    __syncthreads();
    const int lim = min(RTILE, n - base);
    for (int j = 0; j < lim; ++j) {
      const double2 a = *reinterpret_cast<const double2*>(tile + 4 * j);
      const double2 b = *reinterpret_cast<const double2*>(tile + 4 * j + 2);
      c += pffund::sampson_inlier(E, a.x, a.y, b.x, b.y, thr2) ? 1 : 0;
    }
  }
  unsigned long long key = valid ? slot_key_root4(c, (int)(id >> 4), (int)(id & 15u)) : 0ull;
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

__device__ __forceinline__ bool row_inlier(const double (&E)[9], const double* __restrict__ mp,
                                           int i, double thr2) {
  const double2 a = *reinterpret_cast<const double2*>(mp + 4 * (long long)i);
  const double2 b = *reinterpret_cast<const double2*>(mp + 4 * (long long)i + 2);
  return pffund::sampson_inlier(E, a.x, a.y, b.x, b.y, thr2);
}

__global__ __launch_bounds__(256) void ess_select_kernel(
    const Pair* __restrict__ tab, const double* __restrict__ rows, const double* __restrict__ cams,
    const int* __restrict__ counts, const int* __restrict__ cnt, const Rec* __restrict__ recs,
    const unsigned long long* __restrict__ slots, int nblk, double thr, double* __restrict__ Eout,
    double* __restrict__ pose, int* __restrict__ info, int* __restrict__ cheir,
    uint8_t* __restrict__ inlier) {
  __shared__ unsigned long long kred[RBLOCK];
  __shared__ int ired[RBLOCK];
  __shared__ double wsum[RBLOCK / 64][45];
  __shared__ double ewin[9];
  const int p = blockIdx.x, tid = threadIdx.x;
  const Pair q = tab[p];
  const int n = pair_count(counts, p, q);
  uint8_t* ip = inlier + q.moff;
  unsigned long long mine = 0ull;
  for (int s = tid; s < nblk * ESUB; s += RBLOCK) {
    const unsigned long long k = slots[(long long)p * nblk * ESUB + s];
    mine = k > mine ? k : mine;
  }
  const unsigned long long key = block_reduce(mine, kred, OpMax());
  if ((key >> 32) == 0) {  // fewer than 5 matches, or every sample rejected
    for (int i = tid; i < q.n1; i += RBLOCK) ip[i] = 0;
    if (tid < 9) Eout[9 * (long long)p + tid] = 0.0;
    if (tid < 12) pose[12 * (long long)p + tid] = 0.0;
    if (tid < 4) info[4 * (long long)p + tid] = tid == 0 ? 1 : (tid == 2 ? -1 : 0);
    if (tid < 2) cheir[2 * (long long)p + tid] = tid == 0 ? -1 : 0;
    return;
  }
  const int it = slot_key_iter4(key), root = slot_key_rootidx4(key);
  {  // the winner's record: exactly one of its block's records carries the id
    const long long hb = (long long)p * nblk + it / RBLOCK;
    const int nrec = cnt[hb];
    const unsigned long long id = ((unsigned long long)(unsigned)it << 4) | (unsigned)root;
    const Rec* r = recs + hb * EBLOCK_RECS;
    for (int i = tid; i < nrec; i += RBLOCK)
      if (r[i].id == id) {
#pragma unroll
        for (int k = 0; k < 9; ++k) ewin[k] = r[i].E[k];
      }
    __syncthreads();
  }
  const double* mp = rows + 4 * (long long)q.moff;
  const double thr2 = pair_thr2(cams, q, thr);
  double E0[9];
#pragma unroll
  for (int k = 0; k < 9; ++k) E0[k] = ewin[k];
  // inliers of the winner and the upper triangle of the normal matrix over
  // them, each thread over its rows in ascending order
  double a[9][9];
#pragma unroll
  for (int r = 0; r < 9; ++r)
#pragma unroll
    for (int c = r; c < 9; ++c) a[r][c] = 0.0;
  int c0 = 0;
  for (int i = tid; i < n; i += RBLOCK) {
    const bool in = row_inlier(E0, mp, i, thr2);
    ip[i] = in ? 1 : 0;
    if (!in) continue;
    ++c0;
    double row[9];
    pffund::epi_row(mp[4 * (long long)i], mp[4 * (long long)i + 1], mp[4 * (long long)i + 2],
                    mp[4 * (long long)i + 3], row);
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
  double E1[9];
  bool fin1 = true;
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
#pragma unroll
    for (int r = 0; r < 9; ++r) E1[r] = pf_shfl(e, r, 64);
    pffund::rank2(E1);
    pfess::project(E1);
#pragma unroll
    for (int k = 0; k < 9; ++k) fin1 = fin1 && pffund::finite_d(E1[k]);
    fin1 = pffund::unit_sign(E1) && fin1;
  }
  // fewer than 8 inliers leave the linear fit under-determined: no refit
  const bool ok1 = c0 >= pfess::REFIT_MIN && fin1;
  int c1 = 0;
  for (int i = tid; i < n; i += RBLOCK) c1 += row_inlier(E1, mp, i, thr2) ? 1 : 0;
  c1 = block_reduce(c1, ired, OpAdd());
  const bool keep = ok1 && c1 >= c0;
  if (keep) {
#pragma unroll
    for (int k = 0; k < 9; ++k) E0[k] = E1[k];
    for (int i = tid; i < n; i += RBLOCK) ip[i] = row_inlier(E0, mp, i, thr2) ? 1 : 0;
  }
  for (int i = n + tid; i < q.n1; i += RBLOCK) ip[i] = 0;
  // the four poses (every thread the same operations) and the matches in front
  // of both cameras among the inliers
  double P[4][12];
  pfess::decompositions(E0, P);
  int f0 = 0, f1 = 0, f2 = 0, f3 = 0;
  for (int i = tid; i < n; i += RBLOCK) {
    if (!row_inlier(E0, mp, i, thr2)) continue;
    const double x = mp[4 * (long long)i], y = mp[4 * (long long)i + 1];
    const double u = mp[4 * (long long)i + 2], v = mp[4 * (long long)i + 3];
    f0 += pfess::in_front(P[0], x, y, u, v) ? 1 : 0;
    f1 += pfess::in_front(P[1], x, y, u, v) ? 1 : 0;
    f2 += pfess::in_front(P[2], x, y, u, v) ? 1 : 0;
    f3 += pfess::in_front(P[3], x, y, u, v) ? 1 : 0;
  }
  f0 = block_reduce(f0, ired, OpAdd());
  f1 = block_reduce(f1, ired, OpAdd());
  f2 = block_reduce(f2, ired, OpAdd());
  f3 = block_reduce(f3, ired, OpAdd());
  if (tid == 0) {
    int best = 0, nf = f0;
    if (f1 > nf) best = 1, nf = f1;
    if (f2 > nf) best = 2, nf = f2;
    if (f3 > nf) best = 3, nf = f3;
#pragma unroll
    for (int i = 0; i < 9; ++i) Eout[9 * (long long)p + i] = E0[i];
#pragma unroll
    for (int i = 0; i < 12; ++i)
      pose[12 * (long long)p + i] =
          best == 0 ? P[0][i] : (best == 1 ? P[1][i] : (best == 2 ? P[2][i] : P[3][i]));
    int* o = info + 4 * (long long)p;
    o[0] = 0, o[1] = keep ? c1 : c0, o[2] = it, o[3] = (keep ? 1 : 0) | (root << 8);
    cheir[2 * (long long)p] = best, cheir[2 * (long long)p + 1] = nf;
  }
}

}  // namespace

extern "C" int posfeat_essential_solve5(const double* m, double* E) {
  if (!m || !E) return POSFEAT_E_INVALID;
  double mm[5][4], e[pfess::MAXCAND][9];
  for (int i = 0; i < 5; ++i)
    for (int k = 0; k < 4; ++k) {
      mm[i][k] = m[4 * i + k];
      if (!pffund::finite_d(mm[i][k])) return 0;
    }
  const int nc = pfess::solve5(mm, e);
  for (int r = 0; r < nc; ++r)
    for (int i = 0; i < 9; ++i) E[9 * r + i] = e[r][i];
  return nc;
}

extern "C" int posfeat_essential_decompose(const double* E, const double* m, int n, double* pose,
                                           int32_t* front) {
  if (!E || !pose || !front || n < 0 || (n > 0 && !m)) return POSFEAT_E_INVALID;
  double e[9], P[4][12];
  for (int i = 0; i < 9; ++i) e[i] = E[i];
  pfess::decompositions(e, P);
  for (int k = 0; k < 4; ++k)
    for (int i = 0; i < 12; ++i)
      if (!pffund::finite_d(P[k][i])) return POSFEAT_E_INVALID;
  int best = 0, nf = -1;
  for (int k = 0; k < 4; ++k) {
    int f = 0;
    for (int i = 0; i < n; ++i)
      f += pfess::in_front(P[k], m[4 * i], m[4 * i + 1], m[4 * i + 2], m[4 * i + 3]) ? 1 : 0;
    if (f > nf) best = k, nf = f;
  }
  for (int i = 0; i < 12; ++i) pose[i] = P[best][i];
  front[0] = best, front[1] = nf;
  return POSFEAT_OK;
}

extern "C" size_t posfeat_ransac_essential_workspace(const int32_t* set_off, int nsets,
                                                     const int32_t* pairs, int npairs, int iters) {
  EssPlan pl;
  if (nsets <= 0 || npairs <= 0 ||
      build_plan_essential(set_off, nsets, pairs, npairs, iters, pl) != 0)
    return 0;
  return pl.total_bytes;
}

extern "C" int posfeat_ransac_essential(const float* kp, const double* cams,
                                        const int32_t* set_off, int nsets, const int32_t* pairs,
                                        int npairs, const int32_t* matches, const int32_t* counts,
                                        int iters, double thr, uint64_t seed, double* E,
                                        double* pose, int32_t* info, int32_t* cheir,
                                        uint8_t* inlier, void* ws, size_t ws_bytes, void* stream) {
  if (!kp || !cams || !set_off || !pairs || !matches || !counts || !E || !pose || !info ||
      !cheir || !inlier || !ws || nsets <= 0 || npairs <= 0)
    return POSFEAT_E_INVALID;
  if (!(thr > 0.0) || !(thr < (double)INFINITY)) return POSFEAT_E_INVALID;
  if ((reinterpret_cast<uintptr_t>(ws) & 255) || (reinterpret_cast<uintptr_t>(E) & 7) ||
      (reinterpret_cast<uintptr_t>(pose) & 7) || (reinterpret_cast<uintptr_t>(cams) & 7) ||
      (reinterpret_cast<uintptr_t>(info) & 3) || (reinterpret_cast<uintptr_t>(cheir) & 3))
    return POSFEAT_E_INVALID;
  EssPlan pl;
  if (build_plan_essential(set_off, nsets, pairs, npairs, iters, pl) != 0)
    return POSFEAT_E_INVALID;
  if (ws_bytes < pl.total_bytes) return POSFEAT_E_WORKSPACE;
  hipStream_t st = pf_stream(stream);
  char* w = static_cast<char*>(ws);
  const int nblk = pl.base.nblk;
  // the runtime has read a pageable source when the copy call returns (as
  // posfeat_ransac_homography relies on), so the plan may die with us
  if (hipMemcpyAsync(w, pl.base.tab.data(), pl.base.tab.size() * sizeof(Pair),
                     hipMemcpyHostToDevice, st) != hipSuccess)
    return POSFEAT_E_HIP;
  const Pair* tab = reinterpret_cast<const Pair*>(w);
  double* rows = reinterpret_cast<double*>(w + pl.base.pts_off);
  int* cnt = reinterpret_cast<int*>(w + pl.cnt_off);
  Rec* recs = reinterpret_cast<Rec*>(w + pl.rec_off);
  unsigned long long* slots = reinterpret_cast<unsigned long long*>(w + pl.slot_off);
  const unsigned blocks = (unsigned)(npairs * nblk);
  hipLaunchKernelGGL(ess_gather_kernel, dim3(npairs), dim3(RBLOCK), 0, st, kp, cams, tab, matches,
                     counts, rows);
  PF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ess_solve_kernel, dim3(blocks), dim3(RBLOCK), 0, st, tab, rows, counts, iters,
                     nblk, seed, cnt, recs);
  PF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ess_score_kernel, dim3(blocks * ESUB), dim3(RBLOCK), 0, st, tab, rows, cams,
                     counts, cnt, recs, nblk, thr, slots);
  PF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ess_select_kernel, dim3(npairs), dim3(RBLOCK), 0, st, tab, rows, cams, counts,
                     cnt, recs, slots, nblk, thr, E, pose, info, cheir, inlier);
  PF_CHECK_LAUNCH();
  return POSFEAT_OK;
}
