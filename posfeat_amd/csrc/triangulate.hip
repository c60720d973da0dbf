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
#include <math.h>

#include "common.h"
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
