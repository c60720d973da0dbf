// triangulate.hip -- feature tracks and one robustly triangulated 3-D point per
// track from verified matches and known cameras, on gfx950: what the
// reference's Aachen pipeline asks of `colmap point_triangulator`.  Nine
// launches whatever the number of rows, edges and tracks:
//
//   tri_init_kernel     per row: its set (binary search in the uploaded table),
//                       its undistorted normalised point, parent = itself,
//                       size / cursor 0, point_of_row -1; counts 0.
//   tri_hook_kernel     per edge: validity (counted), then lock-free hooking:
//                       both roots by agent-scope relaxed atomic loads, the
//                       larger root linked under the smaller by a 32-bit
//                       compare-and-swap, again on failure (a failed swap means
//                       another edge linked that root: nobody waits for
//                       anybody).  Path halving stores grandparents only, which
//                       are ancestors for good, with atomic stores.
//   tri_flatten_kernel  per row: its root (the smallest row of its component,
//                       since every link points to a smaller row), one integer
//                       atomic add on the root's size.
//   tri_scan_*_kernel   three launches: the exclusive scan over the rows of
//                       (1, size) at the roots of components of 2..max_track
//                       rows, both sums in one 64-bit word.  Gives the track id
//                       and the member offset of a root (ascending root order),
//                       T and the member count; counts the oversized components.
//   tri_fill_kernel     per row of a track: an atomic slot in its track's
//                       member range (any order; the track kernels sort).
//   tri_lane_kernel     tracks of at most LANE_TRACK members, one per lane.
//   tri_wave_kernel     longer tracks, one per wave, a hypothesis per lane.
//
// The two track kernels run the same device functions (triangulate_solve.h);
// both order the members first (rank counting: in registers / in LDS), so
// nothing depends on the order the slots were handed out.  Floating-point
// contraction is off for the whole file: the hypothesis a lane scores and the
// one the winner is rebuilt from are the same operations.
//
// posfeat_split_tracks (further down, with its own launch list) runs the same
// device functions on the members a track's RANSAC left out.
#include <math.h>

#include "common.h"
#include "split_plan.h"
#include "triangulate_solve.h"

#pragma clang fp contract(off)

namespace {

using namespace pftri;

constexpr int LANE_TRACK = 6;   // members a lane-mapped track has at the most (15 hypotheses)
constexpr int WAVE_LDS = 1024;  // = MAX_TRACK: members a wave holds in LDS
static_assert(WAVE_LDS == MAX_TRACK, "the wave kernel holds a whole track in LDS");

__device__ __forceinline__ int ld_relaxed(const int32_t* p) {
  return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void st_relaxed(int32_t* p, int32_t v) {
  __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

__global__ __launch_bounds__(256) void tri_init_kernel(
    const float* __restrict__ kp, const int32_t* __restrict__ set_tab, int nsets, long long n,
    const double* __restrict__ cams, int32_t* __restrict__ setid, int32_t* __restrict__ parent,
    int32_t* __restrict__ size, int32_t* __restrict__ cursor, double* __restrict__ und,
    int32_t* __restrict__ point_of_row, int32_t* __restrict__ counts) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r < 8) counts[r] = 0;
  if (r >= n) return;
  // the set s with set_tab[s] <= r < set_tab[s + 1] (empty sets skipped)
  int lo = 0, hi = nsets;  // invariant: set_tab[lo] <= r < set_tab[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (set_tab[mid] <= r) lo = mid; else hi = mid;
  }
  setid[r] = lo;
  parent[r] = (int32_t)r;
  size[r] = 0;
  cursor[r] = 0;
  point_of_row[r] = -1;
  double xu, yu;
  undistort(cams + 8 * (long long)lo, (double)kp[2 * r], (double)kp[2 * r + 1], xu, yu);
  und[2 * r] = xu, und[2 * r + 1] = yu;
}

__device__ __forceinline__ int find_root(int32_t* parent, int x) {
  for (;;) {
    const int p = ld_relaxed(parent + x);
    if (p == x) return x;
    const int g = ld_relaxed(parent + p);
    if (g != p) st_relaxed(parent + x, g);  // an ancestor of x for good
    x = p;
  }
}

__global__ __launch_bounds__(256) void tri_hook_kernel(const int32_t* __restrict__ edges,
                                                       long long nedges, long long n,
                                                       const int32_t* __restrict__ setid,
                                                       int32_t* parent,
                                                       int32_t* __restrict__ counts) {
  const long long stride = (long long)gridDim.x * 256;
  int ignored = 0;
  for (long long e = (long long)blockIdx.x * 256 + threadIdx.x; e < nedges; e += stride) {
    const int a = edges[2 * e], b = edges[2 * e + 1];
    if (a < 0 || b < 0 || a >= n || b >= n || a == b || setid[a] == setid[b]) {
      ++ignored;
      continue;
    }
    for (;;) {
      int ra = find_root(parent, a), rb = find_root(parent, b);
      if (ra == rb) break;
      if (ra < rb) {
        const int t = ra;
        ra = rb, rb = t;
      }
      int expect = ra;  // the larger root goes under the smaller
      if (__hip_atomic_compare_exchange_strong(parent + ra, &expect, rb, __ATOMIC_RELAXED,
                                               __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT))
        break;
    }
  }
  if (ignored) atomicAdd(counts + 5, ignored);
}

__global__ __launch_bounds__(256) void tri_flatten_kernel(long long n, int32_t* parent,
                                                          int32_t* __restrict__ size) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  int x = (int)r;
  for (;;) {  // the links are final; only the shortcuts below still move
    const int p = ld_relaxed(parent + x);
    if (p == x) break;
    x = p;
  }
  st_relaxed(parent + r, x);
  atomicAdd(size + x, 1);
}

// (1 << 32 | size) at the root of a track, else 0
__device__ __forceinline__ unsigned long long scan_value(long long r, long long n,
                                                         const int32_t* __restrict__ parent,
                                                         const int32_t* __restrict__ size,
                                                         int max_track) {
  if (r >= n || parent[r] != r) return 0ull;
  const int s = size[r];
  return s >= 2 && s <= max_track ? ((1ull << 32) | (unsigned)s) : 0ull;
}

// exclusive scan of one value per thread over the workgroup (256 threads)
__device__ __forceinline__ unsigned long long block_exscan(unsigned long long v,
                                                           unsigned long long* sh,
                                                           unsigned long long& total) {
  const int tid = threadIdx.x;
  sh[tid] = v;
  __syncthreads();
  for (int o = 1; o < 256; o <<= 1) {
    const unsigned long long add = tid >= o ? sh[tid - o] : 0ull;
    __syncthreads();
    sh[tid] += add;
    __syncthreads();
  }
  total = sh[255];
  const unsigned long long ex = sh[tid] - v;
  __syncthreads();
  return ex;
}

constexpr int ROWS_PER_THREAD = SCAN_ROWS / 256;

__global__ __launch_bounds__(256) void tri_scan_sum_kernel(long long n,
                                                           const int32_t* __restrict__ parent,
                                                           const int32_t* __restrict__ size,
                                                           int max_track,
                                                           unsigned long long* __restrict__ bsum) {
  __shared__ unsigned long long sh[256];
  const long long base = (long long)blockIdx.x * SCAN_ROWS + threadIdx.x * ROWS_PER_THREAD;
  unsigned long long v = 0;
#pragma unroll
  for (int k = 0; k < ROWS_PER_THREAD; ++k) v += scan_value(base + k, n, parent, size, max_track);
  unsigned long long total;
  block_exscan(v, sh, total);
  if (threadIdx.x == 0) bsum[blockIdx.x] = total;
}

// one workgroup: bsum <- its exclusive scan; T, the member count, track_off[T]
__global__ __launch_bounds__(256) void tri_scan_top_kernel(long long nblk,
                                                           unsigned long long* __restrict__ bsum,
                                                           int32_t* __restrict__ counts,
                                                           int32_t* __restrict__ track_off) {
  __shared__ unsigned long long sh[256];
  unsigned long long carry = 0;
  for (long long base = 0; base < nblk; base += 256) {
    const long long i = base + threadIdx.x;
    const unsigned long long v = i < nblk ? bsum[i] : 0ull;
    unsigned long long total;
    const unsigned long long ex = block_exscan(v, sh, total);
    if (i < nblk) bsum[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    const int T = (int)(carry >> 32), members = (int)(unsigned)carry;
    counts[0] = T, counts[1] = members;
    track_off[T] = members;
  }
}

__global__ __launch_bounds__(256) void tri_scan_apply_kernel(
    long long n, const int32_t* __restrict__ parent, const int32_t* __restrict__ size,
    int max_track, const unsigned long long* __restrict__ bsum, int32_t* __restrict__ tid_of,
    int32_t* __restrict__ track_off, int32_t* __restrict__ counts) {
  __shared__ unsigned long long sh[256];
  const long long base = (long long)blockIdx.x * SCAN_ROWS + threadIdx.x * ROWS_PER_THREAD;
  unsigned long long val[ROWS_PER_THREAD], v = 0;
#pragma unroll
  for (int k = 0; k < ROWS_PER_THREAD; ++k) {
    val[k] = scan_value(base + k, n, parent, size, max_track);
    v += val[k];
  }
  unsigned long long total;
  unsigned long long at = block_exscan(v, sh, total) + bsum[blockIdx.x];
  int dropped = 0;
#pragma unroll
  for (int k = 0; k < ROWS_PER_THREAD; ++k) {
    const long long r = base + k;
    if (r >= n) break;
    if (val[k]) {
      const int t = (int)(at >> 32);
      tid_of[r] = t;
      track_off[t] = (int32_t)(unsigned)at;
    } else {
      tid_of[r] = -1;
      dropped += parent[r] == r && size[r] > max_track ? 1 : 0;
    }
    at += val[k];
  }
  if (dropped) atomicAdd(counts + 4, dropped);
}

__global__ __launch_bounds__(256) void tri_fill_kernel(long long n,
                                                       const int32_t* __restrict__ parent,
                                                       const int32_t* __restrict__ tid_of,
                                                       const int32_t* __restrict__ track_off,
                                                       int32_t* __restrict__ cursor,
                                                       int32_t* __restrict__ track_rows) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r >= n) return;
  const int root = parent[r], t = tid_of[root];
  if (t < 0) return;
  track_rows[track_off[t] + atomicAdd(cursor + root, 1)] = (int32_t)r;
}

struct Scene {
  const float* kp;
  const int32_t* setid;
  const double* und;
  const double* cams;
  const double* poses;
  uint64_t seed;
  int iters;
  double thr2, cosmin;
};

__device__ __forceinline__ const double* pose_of(const Scene& sc, int row) {
  return sc.poses + 12 * (long long)sc.setid[row];
}

// squared reprojection error and depth of X in the view of `row`
__device__ __forceinline__ double row_reproj2(const Scene& sc, int row, const double (&X)[3],
                                              double& z) {
  const long long s = sc.setid[row];
  return reproj2(sc.cams + 8 * s, sc.poses + 12 * s, X, (double)sc.kp[2 * (long long)row],
                 (double)sc.kp[2 * (long long)row + 1], z);
}

__device__ __forceinline__ bool row_inlier(const Scene& sc, int row, const double (&X)[3]) {
  double z;
  const double e2 = row_reproj2(sc, row, X, z);
  return inlier_of(e2, z, sc.thr2);
}

__device__ __forceinline__ void row_dlt_add(const Scene& sc, int row, double (&nm)[4][4]) {
  dlt_add(nm, sc.und[2 * (long long)row], sc.und[2 * (long long)row + 1], pose_of(sc, row));
}

// z > 0 in both views and the angle at X passes
__device__ __forceinline__ bool pair_ok(const Scene& sc, int ri, int rj, const double (&X)[3]) {
  const double *Pi = pose_of(sc, ri), *Pj = pose_of(sc, rj);
  double Ci[3], Cj[3];
  centre(Pi, Ci);
  centre(Pj, Cj);
  return depth(Pi, X) > 0.0 && depth(Pj, X) > 0.0 && angle_ok(X, Ci, Cj, sc.cosmin);
}

// hypothesis h of the track whose ordered members are rows[0..m): its point,
// the rows of its pair; false when rejected
__device__ __forceinline__ bool hypothesis(const Scene& sc, const int32_t* rows, int m, int h,
                                           double (&X)[3], int& ri, int& rj) {
  int i, j;
  hyp_pair(sc.seed, rows[0], h, m, sc.iters, i, j);
  ri = rows[i], rj = rows[j];
  double nm[4][4];
  dlt_zero(nm);
  row_dlt_add(sc, ri, nm);
  row_dlt_add(sc, rj, nm);
  X[0] = X[1] = X[2] = 0.0;
  return dlt_solve(nm, X) && pair_ok(sc, ri, rj, X);
}

__device__ __forceinline__ unsigned long long hyp_key(int cnt, int h) {
  return ((unsigned long long)(unsigned)(cnt + 1) << 32) | (0xffffffffu - (unsigned)h);
}

struct TrackOut {
  double* points;
  double* err;
  int32_t* tinfo;
  uint8_t* obs_inlier;
  int32_t* point_of_row;
  int32_t* counts;
};

__device__ __forceinline__ void write_track(const TrackOut& o, int t, int status, const double* X,
                                            double err, int nin, int best_h, int kept) {
  o.points[3 * (long long)t] = X[0], o.points[3 * (long long)t + 1] = X[1];
  o.points[3 * (long long)t + 2] = X[2];
  o.err[t] = err;
  int32_t* q = o.tinfo + 4 * (long long)t;
  q[0] = status, q[1] = nin, q[2] = best_h, q[3] = kept;
  if (status == 0) {
    atomicAdd(o.counts + 2, 1);
    atomicAdd(o.counts + 3, nin);
  }
}

// one track per lane: everything in the lane, members in registers
__global__ __launch_bounds__(64) void tri_lane_kernel(Scene sc, const int32_t* __restrict__ track_off,
                                                      int32_t* track_rows, TrackOut o) {
  const int T = o.counts[0];
  const int stride = gridDim.x * 64;
  for (int t = blockIdx.x * 64 + threadIdx.x; t < T; t += stride) {
    const int off = track_off[t], m = track_off[t + 1] - off;
    if (m > LANE_TRACK) continue;
    int32_t* rows = track_rows + off;
    {  // ascending rows by rank counting (the rows are distinct)
      int32_t r[LANE_TRACK];
#pragma unroll
      for (int k = 0; k < LANE_TRACK; ++k) r[k] = k < m ? rows[k] : INT32_MAX;
#pragma unroll
      for (int k = 0; k < LANE_TRACK; ++k) {
        int rank = 0;
#pragma unroll
        for (int j = 0; j < LANE_TRACK; ++j) rank += r[j] < r[k] ? 1 : 0;
        if (k < m) rows[rank] = r[k];
      }
    }
    const int H = num_hyp(m, sc.iters);
    unsigned long long best = 0ull;
    for (int h = 0; h < H; ++h) {
      double X[3];
      int ri, rj;
      if (!hypothesis(sc, rows, m, h, X, ri, rj)) continue;
      int cnt = 0;
      for (int k = 0; k < m; ++k) cnt += row_inlier(sc, rows[k], X) ? 1 : 0;
      const unsigned long long key = hyp_key(cnt, h);
      best = key > best ? key : best;
    }
    double X[3] = {0.0, 0.0, 0.0};
    if (best == 0ull) {
      for (int k = 0; k < m; ++k) o.obs_inlier[off + k] = 0;
      write_track(o, t, 1, X, 0.0, 0, -1, 0);
      continue;
    }
    const int h0 = (int)(0xffffffffu - (unsigned)best), c0 = (int)(best >> 32) - 1;
    int ri, rj;
    hypothesis(sc, rows, m, h0, X, ri, rj);
    double nm[4][4], X1[3] = {0.0, 0.0, 0.0};
    dlt_zero(nm);
    for (int k = 0; k < m; ++k)
      if (row_inlier(sc, rows[k], X)) row_dlt_add(sc, rows[k], nm);
    bool keep = dlt_solve(nm, X1);
    if (keep) {
      int c1 = 0;
      for (int k = 0; k < m; ++k) c1 += row_inlier(sc, rows[k], X1) ? 1 : 0;
      keep = c1 >= c0 && pair_ok(sc, ri, rj, X1);
    }
    if (keep) X[0] = X1[0], X[1] = X1[1], X[2] = X1[2];
    double sum = 0.0;
    int nin = 0;
    for (int k = 0; k < m; ++k) {
      double z;
      const double e2 = row_reproj2(sc, rows[k], X, z);
      const bool in = inlier_of(e2, z, sc.thr2);
      o.obs_inlier[off + k] = in ? 1 : 0;
      if (in) {
        sum = sum + sqrt(e2);
        ++nin;
        o.point_of_row[rows[k]] = t;
      }
    }
    write_track(o, t, 0, X, nin > 0 ? sum / (double)nin : 0.0, nin, h0, keep ? 1 : 0);
  }
}

__device__ __forceinline__ unsigned long long wave_max(unsigned long long v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = pf_shfl_xor(v, o, 64);
    v = other > v ? other : v;
  }
  return v;
}
__device__ __forceinline__ int wave_add(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += pf_shfl_xor(v, o, 64);
  return v;
}

// one track per wave (a workgroup is one wave): a hypothesis per lane, the
// members in LDS.  A workgroup takes 64 consecutive tracks at a time and works
// through those that are its kind.
__global__ __launch_bounds__(64) void tri_wave_kernel(Scene sc, const int32_t* __restrict__ track_off,
                                                      int32_t* track_rows, TrackOut o) {
  __shared__ int32_t srt[WAVE_LDS];   // the ordered members
  __shared__ int32_t aux[WAVE_LDS];   // the members as filled, then the inlier flags
  __shared__ double ebuf[WAVE_LDS];   // the final reprojection errors
  const int T = o.counts[0], lane = threadIdx.x;
  for (long long base = (long long)blockIdx.x * 64; base < T; base += (long long)gridDim.x * 64) {
    const long long mine = base + lane;
    const int mm = mine < T ? track_off[mine + 1] - track_off[mine] : 0;
    unsigned long long todo = __ballot(mm > LANE_TRACK);
    while (todo) {
      const int t = (int)base + (__ffsll((long long)todo) - 1);
      todo &= todo - 1;
      const int off = track_off[t], m = track_off[t + 1] - off;  // m <= MAX_TRACK = WAVE_LDS
      __syncthreads();
      for (int k = lane; k < m; k += 64) aux[k] = track_rows[off + k];
      __syncthreads();
      for (int k = lane; k < m; k += 64) {
        const int r = aux[k];
        int rank = 0;
        for (int j = 0; j < m; ++j) rank += aux[j] < r ? 1 : 0;
        srt[rank] = r;
      }
      __syncthreads();
      for (int k = lane; k < m; k += 64) track_rows[off + k] = srt[k];
      const int H = num_hyp(m, sc.iters);
      unsigned long long best = 0ull;
      for (int h = lane; h < H; h += 64) {
        double X[3];
        int ri, rj;
        if (!hypothesis(sc, srt, m, h, X, ri, rj)) continue;
        int cnt = 0;
        for (int k = 0; k < m; ++k) cnt += row_inlier(sc, srt[k], X) ? 1 : 0;
        const unsigned long long key = hyp_key(cnt, h);
        best = key > best ? key : best;
      }
      best = wave_max(best);
      double X[3] = {0.0, 0.0, 0.0};
      if (best == 0ull) {  // the whole wave
        for (int k = lane; k < m; k += 64) o.obs_inlier[off + k] = 0;
        if (lane == 0) write_track(o, t, 1, X, 0.0, 0, -1, 0);
        continue;
      }
      const int h0 = (int)(0xffffffffu - (unsigned)best), c0 = (int)(best >> 32) - 1;
      int ri, rj;
      hypothesis(sc, srt, m, h0, X, ri, rj);  // every lane: the same operations, the same bits
      for (int k = lane; k < m; k += 64) aux[k] = row_inlier(sc, srt[k], X) ? 1 : 0;
      __syncthreads();
      double nm[4][4], X1[3] = {0.0, 0.0, 0.0};
      dlt_zero(nm);
      for (int k = 0; k < m; ++k)  // member order, every lane the same sum
        if (aux[k]) row_dlt_add(sc, srt[k], nm);
      bool keep = dlt_solve(nm, X1);
      int c1 = 0;
      for (int k = lane; k < m; k += 64) c1 += row_inlier(sc, srt[k], X1) ? 1 : 0;
      c1 = wave_add(c1);
      keep = keep && c1 >= c0 && pair_ok(sc, ri, rj, X1);
      if (keep) X[0] = X1[0], X[1] = X1[1], X[2] = X1[2];
      __syncthreads();
      for (int k = lane; k < m; k += 64) {
        double z;
        const double e2 = row_reproj2(sc, srt[k], X, z);
        const bool in = inlier_of(e2, z, sc.thr2);
        aux[k] = in ? 1 : 0;
        ebuf[k] = in ? sqrt(e2) : 0.0;
        o.obs_inlier[off + k] = in ? 1 : 0;
        if (in) o.point_of_row[srt[k]] = t;
      }
      __syncthreads();
      if (lane == 0) {
        double sum = 0.0;
        int nin = 0;
        for (int k = 0; k < m; ++k)
          if (aux[k]) sum = sum + ebuf[k], ++nin;
        write_track(o, t, 0, X, nin > 0 ? sum / (double)nin : 0.0, nin, h0, keep ? 1 : 0);
      }
    }
  }
}

unsigned grid_for(long long items, int per_block, unsigned cap) {
  long long g = (items + per_block - 1) / per_block;
  if (g < 1) g = 1;
  return (unsigned)(g > (long long)cap ? cap : g);
}

// ---- posfeat_split_tracks: sequential RANSAC over a track's left-over members ----
//
// Seven launches whatever the number of parents:
//
//   split_init_kernel        per row: its set, its undistorted point,
//                            point_of_row -1; marks, child counts, counts 0.
//   split_lane_kernel        per parent: |L1| (-1 for a carried parent); parents
//                            whose L1 has at most LANE_TRACK rows, one per lane:
//                            the list in the workspace (the parent's own range),
//                            the members' positions packed in one 64-bit word.
//   split_wave_kernel        parents with a longer L1, one per wave, the list
//                            and the positions in LDS; L_{g+1} is compacted from
//                            L_g by ballot and prefix count, in member order.
//   split_scan_sum / _top / _apply   the exclusive scan of (1 + children) over
//                            the parents; the apply launch numbers the output
//                            tracks (split_plan.h) and writes what is per track.
//   split_emit_kernel        per parent: its range of track_rows dealt out to
//                            the parent and its children, in member order.
//
// The generation loop runs inside the two track kernels, on the device
// functions the triangulate kernels run, behind a test of the member row.

struct SplitIn {
  const double* points;
  const double* err;
  const int32_t* tinfo;
  const int32_t* track_off;
  const int32_t* track_rows;
  const uint8_t* flags;
  const int32_t* counts;
  long long n, mmax;
  int tmax, tmax_out, rounds;
};

struct SplitWs {
  int32_t* list;
  uint8_t* mark;
  int32_t* nleft;
  int32_t* nchild;
  int32_t* ids;
  int32_t* ncreated;
  double* cpoint;
  double* cerr;
  int32_t* cinfo;
  unsigned long long* bsum;
};

struct SplitOut {
  double* points;
  double* err;
  int32_t* tinfo;
  int32_t* track_off;
  int32_t* track_rows;
  uint8_t* obs_inlier;
  int32_t* point_of_row;
  int32_t* parent_of;
  int32_t* generation;
  int32_t* counts;
};

__device__ __forceinline__ int split_tracks_of(const SplitIn& in) {
  const int T = in.counts[0];
  return T < 0 ? 0 : (T > in.tmax ? in.tmax : T);
}

// posfeat_refine_points' rule: inside the member buffers, at most MAX_TRACK
__device__ __forceinline__ bool split_range_ok(const SplitIn& in, int off, int m) {
  return off >= 0 && m >= 0 && (long long)off + m <= in.mmax && m <= MAX_TRACK;
}

__device__ __forceinline__ bool split_row_valid(const SplitIn& in, int row) {
  return row >= 0 && row < in.n;
}

__global__ __launch_bounds__(256) void split_init_kernel(
    const float* __restrict__ kp, const int32_t* __restrict__ set_tab, int nsets,
    const double* __restrict__ cams, SplitIn in, int32_t* __restrict__ setid,
    double* __restrict__ und, SplitWs w, int32_t* __restrict__ point_of_row,
    int32_t* __restrict__ counts) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r < 8) counts[r] = 0;
  if (r < in.tmax) w.nchild[r] = 0, w.nleft[r] = -1;
  if (r < in.mmax) w.mark[r] = 0;
  if (r >= in.n) return;
  int lo = 0, hi = nsets;  // invariant: set_tab[lo] <= r < set_tab[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (set_tab[mid] <= r) lo = mid; else hi = mid;
  }
  setid[r] = lo;
  point_of_row[r] = -1;
  double xu, yu;
  undistort(cams + 8 * (long long)lo, (double)kp[2 * r], (double)kp[2 * r + 1], xu, yu);
  und[2 * r] = xu, und[2 * r + 1] = yu;
}

// hypothesis(), a pair with a row outside the pool rejected before it is read
__device__ __forceinline__ bool split_hypothesis(const Scene& sc, const SplitIn& in,
                                                 const int32_t* rows, int m, int h, double (&X)[3],
                                                 int& ri, int& rj) {
  int i, j;
  hyp_pair(sc.seed, rows[0], h, m, sc.iters, i, j);
  ri = rows[i], rj = rows[j];
  X[0] = X[1] = X[2] = 0.0;
  if (!split_row_valid(in, ri) || !split_row_valid(in, rj)) return false;
  double nm[4][4];
  dlt_zero(nm);
  row_dlt_add(sc, ri, nm);
  row_dlt_add(sc, rj, nm);
  return dlt_solve(nm, X) && pair_ok(sc, ri, rj, X);
}

__device__ __forceinline__ bool split_row_inlier(const Scene& sc, const SplitIn& in, int row,
                                                 const double (&X)[3]) {
  return split_row_valid(in, row) && row_inlier(sc, row, X);
}

__device__ __forceinline__ void split_store_child(const SplitWs& w, int t, int g,
                                                  const double (&X)[3], double err, int nin,
                                                  int best_h, int kept) {
  const long long c = 4 * (long long)t + (g - 1);
  w.cpoint[3 * c] = X[0], w.cpoint[3 * c + 1] = X[1], w.cpoint[3 * c + 2] = X[2];
  w.cerr[c] = err;
  int32_t* q = w.cinfo + 4 * c;
  q[0] = 0, q[1] = nin, q[2] = best_h, q[3] = kept;
}

// |L1| of every parent that may split; the generations of those a lane can hold
__global__ __launch_bounds__(64) void split_lane_kernel(Scene sc, SplitIn in, SplitWs w) {
  const int T = split_tracks_of(in);
  const int stride = gridDim.x * 64;
  for (int t = blockIdx.x * 64 + threadIdx.x; t < T; t += stride) {
    const int off = in.track_off[t], m = in.track_off[t + 1] - off;
    if (!split_range_ok(in, off, m) || in.tinfo[4 * (long long)t] != 0) continue;
    int len = 0;
    for (int k = 0; k < m; ++k) len += in.flags[off + k] == 0 ? 1 : 0;
    if (len < 2) continue;
    w.nleft[t] = len;
    if (len > LANE_TRACK) continue;
    int32_t* rows = w.list + off;  // len <= m entries of the parent's own range
    unsigned long long pos = 0ull;  // ten bits per entry: its member number
    {
      int a = 0;
      for (int k = 0; k < m; ++k)
        if (in.flags[off + k] == 0) {
          rows[a] = in.track_rows[off + k];
          pos |= (unsigned long long)k << (10 * a);
          ++a;
        }
    }
    int c = 0;
    for (int g = 1; g <= in.rounds && len >= 2; ++g) {
      const int H = num_hyp(len, sc.iters);
      unsigned long long best = 0ull;
      for (int h = 0; h < H; ++h) {
        double X[3];
        int ri, rj;
        if (!split_hypothesis(sc, in, rows, len, h, X, ri, rj)) continue;
        int cnt = 0;
        for (int k = 0; k < len; ++k) cnt += split_row_inlier(sc, in, rows[k], X) ? 1 : 0;
        const unsigned long long key = hyp_key(cnt, h);
        best = key > best ? key : best;
      }
      if (best == 0ull) break;
      const int h0 = (int)(0xffffffffu - (unsigned)best), c0 = (int)(best >> 32) - 1;
      double X[3];
      int ri, rj;
      split_hypothesis(sc, in, rows, len, h0, X, ri, rj);
      double nm[4][4], X1[3] = {0.0, 0.0, 0.0};
      dlt_zero(nm);
      for (int k = 0; k < len; ++k)
        if (split_row_inlier(sc, in, rows[k], X)) row_dlt_add(sc, rows[k], nm);
      bool keep = dlt_solve(nm, X1);
      if (keep) {
        int c1 = 0;
        for (int k = 0; k < len; ++k) c1 += split_row_inlier(sc, in, rows[k], X1) ? 1 : 0;
        keep = c1 >= c0 && pair_ok(sc, ri, rj, X1);
      }
      if (keep) X[0] = X1[0], X[1] = X1[1], X[2] = X1[2];
      double sum = 0.0;
      int nin = 0;
      unsigned mask = 0u;
      for (int k = 0; k < len; ++k) {
        if (!split_row_valid(in, rows[k])) continue;
        double z;
        const double e2 = row_reproj2(sc, rows[k], X, z);
        if (inlier_of(e2, z, sc.thr2)) {
          sum = sum + sqrt(e2);
          ++nin;
          mask |= 1u << k;
        }
      }
      if (nin < 2) break;
      split_store_child(w, t, g, X, sum / (double)nin, nin, h0, keep ? 1 : 0);
      int b = 0;
      unsigned long long npos = 0ull;
      for (int k = 0; k < len; ++k) {
        const unsigned long long p = (pos >> (10 * k)) & 1023ull;
        if ((mask >> k) & 1u) {
          w.mark[off + (int)p] = (uint8_t)g;
        } else {
          rows[b] = rows[k];
          npos |= p << (10 * b);
          ++b;
        }
      }
      pos = npos, len = b, c = g;
    }
    w.nchild[t] = c;
  }
}

__device__ __forceinline__ int lanes_below(unsigned long long bal, int lane) {
  return __popcll(bal & ((1ull << lane) - 1ull));
}

// one parent per wave (a workgroup is one wave): a hypothesis per lane, the
// list in LDS.  A workgroup takes 64 consecutive parents at a time and works
// through those whose L1 is longer than a lane holds; such a parent finishes
// here however short its list becomes.
__global__ __launch_bounds__(64) void split_wave_kernel(Scene sc, SplitIn in, SplitWs w) {
  __shared__ int32_t srt[WAVE_LDS];    // the list, in member order
  __shared__ uint16_t spos[WAVE_LDS];  // the member number of a list entry
  __shared__ int32_t aux[WAVE_LDS];    // the inlier flags
  __shared__ double ebuf[WAVE_LDS];    // the final reprojection errors
  const int T = split_tracks_of(in), lane = threadIdx.x;
  for (long long base = (long long)blockIdx.x * 64; base < T; base += (long long)gridDim.x * 64) {
    const long long mine = base + lane;
    unsigned long long todo = __ballot(mine < T && w.nleft[mine] > LANE_TRACK);
    while (todo) {
      const int t = (int)base + (__ffsll((long long)todo) - 1);
      todo &= todo - 1;
      const int off = in.track_off[t], m = in.track_off[t + 1] - off;  // the range is usable
      __syncthreads();  // the parent before is done with the LDS
      int len = 0;
      for (int kb = 0; kb < m; kb += 64) {
        const int k = kb + lane;
        const bool left = k < m && in.flags[off + k] == 0;
        const unsigned long long bal = __ballot(left);
        if (left) {
          const int d = len + lanes_below(bal, lane);
          srt[d] = in.track_rows[off + k];
          spos[d] = (uint16_t)k;
        }
        len += __popcll(bal);
      }
      __syncthreads();
      int c = 0;
      for (int g = 1; g <= in.rounds && len >= 2; ++g) {  // uniform: every exit is on wave-wide values
        const int H = num_hyp(len, sc.iters);
        unsigned long long best = 0ull;
        for (int h = lane; h < H; h += 64) {
          double X[3];
          int ri, rj;
          if (!split_hypothesis(sc, in, srt, len, h, X, ri, rj)) continue;
          int cnt = 0;
          for (int k = 0; k < len; ++k) cnt += split_row_inlier(sc, in, srt[k], X) ? 1 : 0;
          const unsigned long long key = hyp_key(cnt, h);
          best = key > best ? key : best;
        }
        best = wave_max(best);
        if (best == 0ull) break;
        const int h0 = (int)(0xffffffffu - (unsigned)best), c0 = (int)(best >> 32) - 1;
        double X[3];
        int ri, rj;
        split_hypothesis(sc, in, srt, len, h0, X, ri, rj);  // every lane: the same bits
        for (int k = lane; k < len; k += 64) aux[k] = split_row_inlier(sc, in, srt[k], X) ? 1 : 0;
        __syncthreads();
        double nm[4][4], X1[3] = {0.0, 0.0, 0.0};
        dlt_zero(nm);
        for (int k = 0; k < len; ++k)  // member order, every lane the same sum
          if (aux[k]) row_dlt_add(sc, srt[k], nm);
        bool keep = dlt_solve(nm, X1);
        int c1 = 0;
        for (int k = lane; k < len; k += 64) c1 += split_row_inlier(sc, in, srt[k], X1) ? 1 : 0;
        c1 = wave_add(c1);
        keep = keep && c1 >= c0 && pair_ok(sc, ri, rj, X1);
        if (keep) X[0] = X1[0], X[1] = X1[1], X[2] = X1[2];
        __syncthreads();
        int nin = 0;
        for (int k = lane; k < len; k += 64) {
          bool inl = false;
          double e2 = 0.0;
          if (split_row_valid(in, srt[k])) {
            double z;
            e2 = row_reproj2(sc, srt[k], X, z);
            inl = inlier_of(e2, z, sc.thr2);
          }
          aux[k] = inl ? 1 : 0;
          ebuf[k] = inl ? sqrt(e2) : 0.0;
          nin += inl ? 1 : 0;
        }
        nin = wave_add(nin);
        __syncthreads();
        if (nin < 2) break;
        if (lane == 0) {
          double sum = 0.0;
          for (int k = 0; k < len; ++k)  // member order
            if (aux[k]) sum = sum + ebuf[k];
          split_store_child(w, t, g, X, sum / (double)nin, nin, h0, keep ? 1 : 0);
        }
        int kept = 0;
        for (int kb = 0; kb < len; kb += 64) {
          const int k = kb + lane;
          const bool have = k < len;
          const int row = have ? srt[k] : 0;
          const uint16_t p = have ? spos[k] : (uint16_t)0;
          const bool inl = have && aux[k] != 0;
          if (inl) w.mark[off + p] = (uint8_t)g;
          const bool left = have && !inl;
          const unsigned long long bal = __ballot(left);
          __syncthreads();  // the chunk is in registers before an entry of it is overwritten
          if (left) {
            const int d = kept + lanes_below(bal, lane);  // d <= k
            srt[d] = row;
            spos[d] = p;
          }
          kept += __popcll(bal);
        }
        __syncthreads();
        len = kept, c = g;
      }
      if (lane == 0) w.nchild[t] = c;
    }
  }
}

constexpr int PARENTS_PER_THREAD = pfsplit::SCAN_PARENTS / 256;

__device__ __forceinline__ unsigned long long split_scan_value(long long t, int T,
                                                               const int32_t* __restrict__ nchild) {
  return t < T ? 1ull + (unsigned long long)nchild[t] : 0ull;
}

__global__ __launch_bounds__(256) void split_scan_sum_kernel(SplitIn in, SplitWs w) {
  __shared__ unsigned long long sh[256];
  const int T = split_tracks_of(in);
  const long long base =
      (long long)blockIdx.x * pfsplit::SCAN_PARENTS + threadIdx.x * PARENTS_PER_THREAD;
  unsigned long long v = 0;
#pragma unroll
  for (int k = 0; k < PARENTS_PER_THREAD; ++k) v += split_scan_value(base + k, T, w.nchild);
  unsigned long long total;
  block_exscan(v, sh, total);
  if (threadIdx.x == 0) w.bsum[blockIdx.x] = total;
}

// one workgroup: bsum <- its exclusive scan; T', the counts that follow from
// it, track_off[T']
__global__ __launch_bounds__(256) void split_scan_top_kernel(long long nblk, SplitIn in, SplitWs w,
                                                             SplitOut o) {
  __shared__ unsigned long long sh[256];
  unsigned long long carry = 0;
  for (long long base = 0; base < nblk; base += 256) {
    const long long i = base + threadIdx.x;
    const unsigned long long v = i < nblk ? w.bsum[i] : 0ull;
    unsigned long long total;
    const unsigned long long ex = block_exscan(v, sh, total);
    if (i < nblk) w.bsum[i] = carry + ex;
    carry += total;
  }
  if (threadIdx.x == 0) {
    const int T = split_tracks_of(in);
    const long long all = (long long)carry;
    const long long Tp = all < in.tmax_out ? all : in.tmax_out;  // T <= tmax <= tmax_out
    o.counts[0] = (int32_t)Tp, o.counts[1] = in.counts[1];
    o.counts[4] = (int32_t)(all - Tp), o.counts[6] = (int32_t)(Tp - T);
    o.track_off[Tp] = in.track_off[T];
  }
}

__global__ __launch_bounds__(256) void split_scan_apply_kernel(SplitIn in, SplitWs w, SplitOut o) {
  __shared__ unsigned long long sh[256];
  const int T = split_tracks_of(in);
  const long long base =
      (long long)blockIdx.x * pfsplit::SCAN_PARENTS + threadIdx.x * PARENTS_PER_THREAD;
  unsigned long long val[PARENTS_PER_THREAD], v = 0;
#pragma unroll
  for (int k = 0; k < PARENTS_PER_THREAD; ++k) {
    val[k] = split_scan_value(base + k, T, w.nchild);
    v += val[k];
  }
  unsigned long long total;
  unsigned long long at = block_exscan(v, sh, total) + w.bsum[blockIdx.x];
  int npoints = 0, nobs = 0, nsplit = 0;
#pragma unroll
  for (int k = 0; k < PARENTS_PER_THREAD; ++k) {
    const long long t = base + k;
    if (t >= T) break;
    const long long id = pfsplit::parent_id((long long)at, t, T, in.tmax_out);
    const int cr = pfsplit::children_created((long long)at, (int)(val[k] - 1ull), t, T, in.tmax_out);
    at += val[k];
    w.ids[t] = (int32_t)id, w.ncreated[t] = cr;
#pragma unroll
    for (int c = 0; c < 3; ++c) o.points[3 * id + c] = in.points[3 * t + c];
    o.err[id] = in.err[t];
#pragma unroll
    for (int c = 0; c < 4; ++c) o.tinfo[4 * id + c] = in.tinfo[4 * t + c];
    o.track_off[id] = in.track_off[t];
    o.parent_of[id] = (int32_t)t, o.generation[id] = 0;
    if (in.tinfo[4 * t] == 0) ++npoints, nobs += in.tinfo[4 * t + 1];
    for (int g = 1; g <= cr; ++g) {
      const long long c = 4 * t + (g - 1), d = id + g;
#pragma unroll
      for (int i = 0; i < 3; ++i) o.points[3 * d + i] = w.cpoint[3 * c + i];
      o.err[d] = w.cerr[c];
#pragma unroll
      for (int i = 0; i < 4; ++i) o.tinfo[4 * d + i] = w.cinfo[4 * c + i];
      o.parent_of[d] = (int32_t)t, o.generation[d] = g;
      ++npoints, nobs += w.cinfo[4 * c + 1];
    }
    nsplit += cr > 0 ? 1 : 0;
  }
  if (npoints) atomicAdd(o.counts + 2, npoints);
  if (nobs) atomicAdd(o.counts + 3, nobs);
  if (nsplit) atomicAdd(o.counts + 7, nsplit);
}

constexpr int EMIT_LANE = 8;  // members of a parent a lane deals out on its own

__device__ __forceinline__ void split_emit(const SplitIn& in, const SplitOut& o, int dst, int row,
                                           uint8_t flag, int g, int id, bool parent_ok) {
  o.track_rows[dst] = row;
  o.obs_inlier[dst] = g == 0 ? flag : (uint8_t)1;
  if (!split_row_valid(in, row)) return;
  if (g > 0) o.point_of_row[row] = id + g;
  else if (flag != 0 && parent_ok) o.point_of_row[row] = id;
}

// the parent's range of track_rows: the members no created child claimed, then
// child 1's, child 2's, ..., each in member order
__global__ __launch_bounds__(64) void split_emit_kernel(SplitIn in, SplitWs w, SplitOut o) {
  const int T = split_tracks_of(in), lane = threadIdx.x;
  for (long long base = (long long)blockIdx.x * 64; base < T; base += (long long)gridDim.x * 64) {
    const long long mine = base + lane;
    bool wave_kind = false;
    if (mine < T) {
      const int t = (int)mine;
      const int off = in.track_off[t], m = in.track_off[t + 1] - off;
      const bool usable = split_range_ok(in, off, m);
      wave_kind = usable && m > EMIT_LANE;
      if (usable && m <= EMIT_LANE) {
        const int id = w.ids[t], cr = w.ncreated[t];
        const bool parent_ok = in.tinfo[4 * (long long)t] == 0;
        int at = off;
        for (int g = 0; g <= cr; ++g) {
          if (g > 0) o.track_off[id + g] = at;
          for (int k = 0; k < m; ++k) {
            const int mk = w.mark[off + k];
            if ((mk <= cr ? mk : 0) != g) continue;
            split_emit(in, o, at, in.track_rows[off + k], in.flags[off + k], g, id, parent_ok);
            ++at;
          }
        }
      }
    }
    unsigned long long todo = __ballot(wave_kind);
    while (todo) {
      const int t = (int)base + (__ffsll((long long)todo) - 1);
      todo &= todo - 1;
      const int off = in.track_off[t], m = in.track_off[t + 1] - off;
      const int id = w.ids[t], cr = w.ncreated[t];
      const bool parent_ok = in.tinfo[4 * (long long)t] == 0;
      int at = off;
      for (int g = 0; g <= cr; ++g) {
        if (g > 0 && lane == 0) o.track_off[id + g] = at;
        for (int kb = 0; kb < m; kb += 64) {
          const int k = kb + lane;
          bool take = false;
          if (k < m) {
            const int mk = w.mark[off + k];
            take = (mk <= cr ? mk : 0) == g;
          }
          const unsigned long long bal = __ballot(take);
          if (take)
            split_emit(in, o, at + lanes_below(bal, lane), in.track_rows[off + k], in.flags[off + k],
                       g, id, parent_ok);
          at += __popcll(bal);
        }
      }
    }
  }
}

}  // namespace

extern "C" int posfeat_triangulate_dlt(const double* obs, int n, double* X) {
  if (!obs || !X || n < 1) return POSFEAT_E_INVALID;
  double nm[4][4], x[3] = {0.0, 0.0, 0.0};
  pftri::dlt_zero(nm);
  for (int i = 0; i < n; ++i) pftri::dlt_add(nm, obs[14 * i], obs[14 * i + 1], obs + 14 * i + 2);
  const bool ok = pftri::dlt_solve(nm, x);
  X[0] = x[0], X[1] = x[1], X[2] = x[2];
  return ok ? 0 : 1;
}

extern "C" size_t posfeat_triangulate_workspace(const int32_t* set_off, int nsets,
                                                long long nedges, int max_track) {
  pftri::Layout L;
  if (max_track < MIN_TRACK || max_track > MAX_TRACK || pftri::layout(set_off, nsets, nedges, L) != 0)
    return 0;
  return L.total;
}

extern "C" int posfeat_triangulate(const float* kp, const int32_t* set_off, int nsets,
                                   const double* cams, const double* poses, const int32_t* edges,
                                   long long nedges, int iters, double thr, double min_angle_deg,
                                   int max_track, uint64_t seed, double* points, double* err,
                                   int32_t* tinfo, int32_t* track_off, int32_t* track_rows,
                                   uint8_t* obs_inlier, int32_t* point_of_row, int32_t* counts,
                                   void* ws, size_t ws_bytes, void* stream) {
  pftri::Layout L;
  if (pftri::layout(set_off, nsets, nedges, L) != 0) return POSFEAT_E_INVALID;
  if ((!kp && L.n > 0) || ((!cams || !poses) && nsets > 0) || (!edges && nedges > 0) || !points ||
      !err || !tinfo || !track_off || !track_rows || !obs_inlier || !point_of_row || !counts || !ws)
    return POSFEAT_E_INVALID;
  if (iters < MIN_ITERS || iters > MAX_ITERS || max_track < MIN_TRACK || max_track > MAX_TRACK)
    return POSFEAT_E_INVALID;
  if (!(thr > 0.0) || !(thr < (double)INFINITY)) return POSFEAT_E_INVALID;
  if (!(min_angle_deg >= 0.0) || !(min_angle_deg < 90.0)) return POSFEAT_E_INVALID;
  if ((reinterpret_cast<uintptr_t>(ws) & 255) || (reinterpret_cast<uintptr_t>(points) & 7) ||
      (reinterpret_cast<uintptr_t>(err) & 7))
    return POSFEAT_E_INVALID;
  if (ws_bytes < L.total) return POSFEAT_E_WORKSPACE;
  hipStream_t st = pf_stream(stream);
  char* w = static_cast<char*>(ws);
  // the runtime has read a pageable source when the copy call returns (as
  // posfeat_ransac_homography relies on)
  if (hipMemcpyAsync(w + L.set_off, set_off, (size_t)(nsets + 1) * 4, hipMemcpyHostToDevice, st) !=
      hipSuccess)
    return POSFEAT_E_HIP;
  const int32_t* set_tab = reinterpret_cast<const int32_t*>(w + L.set_off);
  int32_t* setid = reinterpret_cast<int32_t*>(w + L.setid);
  int32_t* parent = reinterpret_cast<int32_t*>(w + L.parent);
  int32_t* size = reinterpret_cast<int32_t*>(w + L.size);
  int32_t* tid_of = reinterpret_cast<int32_t*>(w + L.tid);
  int32_t* cursor = reinterpret_cast<int32_t*>(w + L.cursor);
  double* und = reinterpret_cast<double*>(w + L.und);
  unsigned long long* bsum = reinterpret_cast<unsigned long long*>(w + L.bsum);
  const long long n = L.n;
  const unsigned row_grid = grid_for(n, 256, 0x7fffffffu);
  const unsigned scan_grid = grid_for(n, SCAN_ROWS, 0x7fffffffu);
  hipLaunchKernelGGL(tri_init_kernel, dim3(row_grid), dim3(256), 0, st, kp, set_tab, nsets, n, cams,
                     setid, parent, size, cursor, und, point_of_row, counts);
  PF_CHECK_LAUNCH();
  hipLaunchKernelGGL(tri_hook_kernel, dim3(grid_for(nedges, 256, 1u << 16)), dim3(256), 0, st,
                     edges, nedges, n, setid, parent, counts);
  PF_CHECK_LAUNCH();
  hipLaunchKernelGGL(tri_flatten_kernel, dim3(row_grid), dim3(256), 0, st, n, parent, size);
  PF_CHECK_LAUNCH();
  hipLaunchKernelGGL(tri_scan_sum_kernel, dim3(scan_grid), dim3(256), 0, st, n, parent, size,
                     max_track, bsum);
  PF_CHECK_LAUNCH();
  hipLaunchKernelGGL(tri_scan_top_kernel, dim3(1), dim3(256), 0, st, L.nblk, bsum, counts,
                     track_off);
  PF_CHECK_LAUNCH();
  hipLaunchKernelGGL(tri_scan_apply_kernel, dim3(scan_grid), dim3(256), 0, st, n, parent, size,
                     max_track, bsum, tid_of, track_off, counts);
  PF_CHECK_LAUNCH();
  hipLaunchKernelGGL(tri_fill_kernel, dim3(row_grid), dim3(256), 0, st, n, parent, tid_of,
                     track_off, cursor, track_rows);
  PF_CHECK_LAUNCH();
  Scene sc{kp, setid, und, cams, poses, seed, iters, thr * thr,
           cos(min_angle_deg * 3.14159265358979323846 / 180.0)};
  TrackOut o{points, err, tinfo, obs_inlier, point_of_row, counts};
  hipLaunchKernelGGL(tri_lane_kernel, dim3(grid_for(L.tmax, 64, 8192)), dim3(64), 0, st, sc,
                     track_off, track_rows, o);
  PF_CHECK_LAUNCH();
  // a workgroup per 64 consecutive tracks, which is how the kernel deals them
  hipLaunchKernelGGL(tri_wave_kernel, dim3(grid_for(L.tmax, 64, 1u << 16)), dim3(64), 0, st, sc,
                     track_off, track_rows, o);
  PF_CHECK_LAUNCH();
  return POSFEAT_OK;
}

extern "C" size_t posfeat_split_tracks_workspace(const int32_t* set_off, int nsets, long long tmax,
                                                 long long mmax, long long tmax_out) {
  pfsplit::Layout L;
  if (pfsplit::layout(set_off, nsets, tmax, mmax, tmax_out, L) != 0) return 0;
  return L.total;
}

extern "C" int posfeat_split_tracks(const float* kp, const int32_t* set_off, int nsets,
                                    const double* cams, const double* poses, const double* points_in,
                                    const double* err_in, const int32_t* tinfo_in,
                                    const int32_t* track_off_in, const int32_t* track_rows_in,
                                    const uint8_t* inlier_in, const int32_t* counts_in, long long tmax,
                                    long long mmax, int iters, double thr, double min_angle_deg,
                                    uint64_t seed, int rounds, long long tmax_out, double* points,
                                    double* err, int32_t* tinfo, int32_t* track_off,
                                    int32_t* track_rows, uint8_t* obs_inlier, int32_t* point_of_row,
                                    int32_t* parent_of, int32_t* generation, int32_t* counts, void* ws,
                                    size_t ws_bytes, void* stream) {
  pfsplit::Layout L;
  if (pfsplit::layout(set_off, nsets, tmax, mmax, tmax_out, L) != 0) return POSFEAT_E_INVALID;
  if ((!kp && L.n > 0) || ((!cams || !poses) && nsets > 0) || !points_in || !err_in || !tinfo_in ||
      !track_off_in || !track_rows_in || !inlier_in || !counts_in || !points || !err || !tinfo ||
      !track_off || !track_rows || !obs_inlier || !point_of_row || !parent_of || !generation ||
      !counts || !ws)
    return POSFEAT_E_INVALID;
  if (!pfsplit::params_ok(iters, thr, min_angle_deg, rounds)) return POSFEAT_E_INVALID;
  // an output is a buffer of its own
  if (points == points_in || err == err_in || tinfo == tinfo_in || track_off == track_off_in ||
      track_rows == track_rows_in || obs_inlier == inlier_in || counts == counts_in)
    return POSFEAT_E_INVALID;
  const uintptr_t a8 = reinterpret_cast<uintptr_t>(points_in) | reinterpret_cast<uintptr_t>(err_in) |
                       reinterpret_cast<uintptr_t>(points) | reinterpret_cast<uintptr_t>(err) |
                       reinterpret_cast<uintptr_t>(cams) | reinterpret_cast<uintptr_t>(poses);
  const uintptr_t a4 =
      reinterpret_cast<uintptr_t>(tinfo_in) | reinterpret_cast<uintptr_t>(track_off_in) |
      reinterpret_cast<uintptr_t>(track_rows_in) | reinterpret_cast<uintptr_t>(counts_in) |
      reinterpret_cast<uintptr_t>(tinfo) | reinterpret_cast<uintptr_t>(track_off) |
      reinterpret_cast<uintptr_t>(track_rows) | reinterpret_cast<uintptr_t>(point_of_row) |
      reinterpret_cast<uintptr_t>(parent_of) | reinterpret_cast<uintptr_t>(generation) |
      reinterpret_cast<uintptr_t>(counts) | reinterpret_cast<uintptr_t>(kp);
  if ((reinterpret_cast<uintptr_t>(ws) & 255) || (a8 & 7) || (a4 & 3)) return POSFEAT_E_INVALID;
  if (ws_bytes < L.total) return POSFEAT_E_WORKSPACE;
  hipStream_t st = pf_stream(stream);
  char* w = static_cast<char*>(ws);
  // the runtime has read a pageable source when the copy call returns (as
  // posfeat_ransac_homography relies on)
  if (hipMemcpyAsync(w + L.set_off, set_off, (size_t)(nsets + 1) * 4, hipMemcpyHostToDevice, st) !=
      hipSuccess)
    return POSFEAT_E_HIP;
  const int32_t* set_tab = reinterpret_cast<const int32_t*>(w + L.set_off);
  int32_t* setid = reinterpret_cast<int32_t*>(w + L.setid);
  double* und = reinterpret_cast<double*>(w + L.und);
  Scene sc{kp, setid, und, cams, poses, seed, iters, thr * thr,
           cos(min_angle_deg * 3.14159265358979323846 / 180.0)};
  SplitIn in{points_in, err_in, tinfo_in, track_off_in, track_rows_in, inlier_in, counts_in,
             L.n,       mmax,   (int)tmax, (int)tmax_out, rounds};
  SplitWs sw{reinterpret_cast<int32_t*>(w + L.list),     reinterpret_cast<uint8_t*>(w + L.mark),
             reinterpret_cast<int32_t*>(w + L.nleft),    reinterpret_cast<int32_t*>(w + L.nchild),
             reinterpret_cast<int32_t*>(w + L.ids),      reinterpret_cast<int32_t*>(w + L.ncreated),
             reinterpret_cast<double*>(w + L.cpoint),    reinterpret_cast<double*>(w + L.cerr),
             reinterpret_cast<int32_t*>(w + L.cinfo),
             reinterpret_cast<unsigned long long*>(w + L.bsum)};
  SplitOut o{points,     err,          tinfo,     track_off,  track_rows,
             obs_inlier, point_of_row, parent_of, generation, counts};
  long long items = L.n > tmax ? L.n : tmax;
  items = items > mmax ? items : mmax;
  items = items > 8 ? items : 8;
  const unsigned scan_grid = grid_for(tmax, pfsplit::SCAN_PARENTS, 0x7fffffffu);
  hipLaunchKernelGGL(split_init_kernel, dim3(grid_for(items, 256, 0x7fffffffu)), dim3(256), 0, st, kp,
                     set_tab, nsets, cams, in, setid, und, sw, point_of_row, counts);
  PF_CHECK_LAUNCH();
  hipLaunchKernelGGL(split_lane_kernel, dim3(grid_for(tmax, 64, 8192)), dim3(64), 0, st, sc, in, sw);
  PF_CHECK_LAUNCH();
  // a workgroup per 64 consecutive parents, which is how the kernel deals them
  hipLaunchKernelGGL(split_wave_kernel, dim3(grid_for(tmax, 64, 1u << 16)), dim3(64), 0, st, sc, in,
                     sw);
  PF_CHECK_LAUNCH();
  hipLaunchKernelGGL(split_scan_sum_kernel, dim3(scan_grid), dim3(256), 0, st, in, sw);
  PF_CHECK_LAUNCH();
  hipLaunchKernelGGL(split_scan_top_kernel, dim3(1), dim3(256), 0, st, L.nblk, in, sw, o);
  PF_CHECK_LAUNCH();
  hipLaunchKernelGGL(split_scan_apply_kernel, dim3(scan_grid), dim3(256), 0, st, in, sw, o);
  PF_CHECK_LAUNCH();
  hipLaunchKernelGGL(split_emit_kernel, dim3(grid_for(tmax, 64, 1u << 16)), dim3(64), 0, st, in, sw,
                     o);
  PF_CHECK_LAUNCH();
  return POSFEAT_OK;
}
