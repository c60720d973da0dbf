// refine.hip -- points-only bundle adjustment of the tracks posfeat_triangulate
// left on the device, on gfx950: what `colmap point_triangulator` does after the
// algebraic answer with fixed poses and fixed intrinsics.  Per track: rounds of
// Levenberg-Marquardt on the pixel reprojection error over the current inlier
// set, the inlier test over all members at the new point, again while the set
// changes; then COLMAP's triangulation-angle filter over the final inliers.
// Three launches whatever the number of tracks:
//
//   ref_init_kernel   per row: its set (binary search in the uploaded table),
//                     point_of_row -1; counts = {T, 0, ...}.
//   ref_lane_kernel   tracks of at most LANE_TRACK members, one per lane: the
//                     set is a bit mask, the sums run in member order.
//   ref_wave_kernel   longer tracks, one per wave (a workgroup is one wave):
//                     rows, flags and final errors in LDS, members lane-strided
//                     ascending, the ten sums reduced by the xor butterfly of
//                     pose_select_kernel, so every lane solves the same 3x3
//                     system on the same bits and the control flow of the round
//                     is uniform; the angle filter takes the inlier pairs (i, j)
//                     with j lane-strided and stops at the first i that has one.
//
// T and the tracks' ranges are read on the device; the grids are sized for the
// worst case and stride.  Camera and pose rows are read through the caches, not
// staged in LDS: the members of a track lie in different images, so a
// workgroup has no row to reuse.  All of the arithmetic is refine_solve.h, the
// text the host compiles for posfeat_refine_point.  Floating-point contraction
// is off for the whole file.
#include <math.h>

#include "common.h"
#include "refine_solve.h"

#pragma clang fp contract(off)

namespace {

using namespace pfrefine;

struct Scene {
  const float* kp;
  const int32_t* setid;
  const double* cams;
  const double* poses;
  long long n, mmax;
  int tmax, rounds, steps;
  double thr2, cosmin;
};

struct TrackIn {
  const double* points;
  const int32_t* tinfo;
  const int32_t* track_off;
  const int32_t* track_rows;
  const uint8_t* flags;
  const int32_t* counts;
};

struct TrackOut {
  double* points;
  double* err;
  int32_t* tinfo;
  uint8_t* obs_inlier;
  int32_t* point_of_row;
  int32_t* rinfo;
  int32_t* counts;
};

__device__ __forceinline__ int tracks_of(const Scene& sc, const TrackIn& in) {
  const int T = in.counts[0];
  return T < 0 ? 0 : (T > sc.tmax ? sc.tmax : T);
}

__global__ __launch_bounds__(256) void ref_init_kernel(const int32_t* __restrict__ set_tab,
                                                       int nsets, Scene sc, TrackIn in,
                                                       int32_t* __restrict__ setid,
                                                       int32_t* __restrict__ point_of_row,
                                                       int32_t* __restrict__ counts) {
  const long long r = (long long)blockIdx.x * 256 + threadIdx.x;
  if (r < 8) counts[r] = r == 0 ? tracks_of(sc, in) : 0;
  if (r >= sc.n) return;
  int lo = 0, hi = nsets;  // invariant: set_tab[lo] <= r < set_tab[hi]
  while (hi - lo > 1) {
    const int mid = (lo + hi) >> 1;
    if (set_tab[mid] <= r) lo = mid; else hi = mid;
  }
  setid[r] = lo;
  point_of_row[r] = -1;
}

__device__ __forceinline__ bool row_valid(const Scene& sc, int row) {
  return row >= 0 && row < sc.n;
}

// the member's share of the sums at X (the row is valid)
__device__ __forceinline__ bool row_acc(const Scene& sc, int row, const double (&X)[3],
                                        double (&acc)[ACC]) {
  const long long s = sc.setid[row];
  return acc_row(sc.cams + 8 * s, sc.poses + 12 * s, (double)sc.kp[2 * (long long)row],
                 (double)sc.kp[2 * (long long)row + 1], X, acc);
}

// triangulate's inlier rule; e = the pixel error
__device__ __forceinline__ bool row_inlier(const Scene& sc, int row, const double (&X)[3],
                                           double& e) {
  e = 0.0;
  if (!row_valid(sc, row)) return false;
  const long long s = sc.setid[row];
  double z;
  const double e2 = pftri::reproj2(sc.cams + 8 * s, sc.poses + 12 * s, X,
                                   (double)sc.kp[2 * (long long)row],
                                   (double)sc.kp[2 * (long long)row + 1], z);
  const bool in = pftri::inlier_of(e2, z, sc.thr2);
  e = in ? sqrt(e2) : 0.0;
  return in;
}

__device__ __forceinline__ void row_centre(const Scene& sc, int row, double (&C)[3]) {
  pftri::centre(sc.poses + 12 * (long long)sc.setid[row], C);
}

// the track's range is usable: inside the member buffers, at most MAX_TRACK
__device__ __forceinline__ bool range_ok(const Scene& sc, int off, int m) {
  return off >= 0 && m >= 0 && (long long)off + m <= sc.mmax && m <= MAX_TRACK;
}

__device__ __forceinline__ void write_track(const TrackIn& in, const TrackOut& o, int t, int status,
                                            const double (&X)[3], double err, int nin, int rounds,
                                            int taken, int converged, int changed) {
  const bool ok = status == 0;
  double* p = o.points + 3 * (long long)t;
  p[0] = ok ? X[0] : 0.0, p[1] = ok ? X[1] : 0.0, p[2] = ok ? X[2] : 0.0;
  o.err[t] = ok ? err : 0.0;
  const int32_t* qi = in.tinfo + 4 * (long long)t;
  int32_t* q = o.tinfo + 4 * (long long)t;
  q[0] = status, q[1] = ok ? nin : 0, q[2] = qi[2], q[3] = qi[3];
  int32_t* ri = o.rinfo + 4 * (long long)t;
  ri[0] = rounds, ri[1] = taken, ri[2] = converged, ri[3] = changed;
  if (ok) {
    atomicAdd(o.counts + 1, 1);
    atomicAdd(o.counts + 2, nin);
  } else {
    atomicAdd(o.counts + (status == 2 ? 3 : (status == 3 ? 4 : 5)), 1);
  }
  if (changed) atomicAdd(o.counts + 6, 1);
}

// one track per lane: the set is a bit mask, everything in the lane
__global__ __launch_bounds__(64) void ref_lane_kernel(Scene sc, TrackIn in, TrackOut o) {
  const int T = tracks_of(sc, in);
  const int stride = gridDim.x * 64;
  for (int t = blockIdx.x * 64 + threadIdx.x; t < T; t += stride) {
    const int off = in.track_off[t], m = in.track_off[t + 1] - off;
    double X[3] = {0.0, 0.0, 0.0};
    if (!range_ok(sc, off, m)) {  // not a table of posfeat_triangulate: no member is touched
      write_track(in, o, t, 1, X, 0.0, 0, 0, 0, 0, 0);
      continue;
    }
    if (m > LANE_TRACK) continue;
    const int32_t* rows = in.track_rows + off;
    uint8_t* flags = o.obs_inlier + off;
    if (in.tinfo[4 * (long long)t] != 0) {
      for (int k = 0; k < m; ++k) flags[k] = 0;
      write_track(in, o, t, 1, X, 0.0, 0, 0, 0, 0, 0);
      continue;
    }
    unsigned S = 0u, given = 0u;
    for (int k = 0; k < m; ++k) {
      const unsigned f = in.flags[off + k] != 0 ? 1u : 0u;
      given |= f << k;
      S |= (row_valid(sc, rows[k]) ? f : 0u) << k;
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) X[c] = in.points[3 * (long long)t + c];
    auto accumulate = [&](const double (&Y)[3], double (&acc)[ACC]) {
      acc_zero(acc);
      bool ok = true;
      for (int k = 0; k < m; ++k)
        if ((S >> k) & 1u) ok = row_acc(sc, rows[k], Y, acc) && ok;
      return ok;
    };
    int used = 0, taken = 0, converged = 0, status = 0, nin = 0;
    double sum = 0.0;
    for (int round = 0; round < sc.rounds; ++round) {
      ++used;
      if (__popc(S) >= 2) {
        double cost;
        taken += lm_round(X, sc.steps, accumulate, cost);
      }
      unsigned F = 0u;
      sum = 0.0;
      for (int k = 0; k < m; ++k) {
        double e;
        const bool inl = row_inlier(sc, rows[k], X, e);
        F |= (inl ? 1u : 0u) << k;
        if (inl) sum = sum + e;
      }
      const bool same = F == S;
      S = F, nin = __popc(F);
      if (nin < 2) {
        status = 2;
        break;
      }
      if (same) {
        converged = 1;
        break;
      }
    }
    if (status == 0) {  // some pair of inliers subtends the angle
      bool found = false;
      for (int i = 0; i < m && !found; ++i) {
        if (!((S >> i) & 1u)) continue;
        double Ci[3];
        row_centre(sc, rows[i], Ci);
        for (int j = i + 1; j < m && !found; ++j) {
          if (!((S >> j) & 1u)) continue;
          double Cj[3];
          row_centre(sc, rows[j], Cj);
          found = pftri::angle_ok(X, Ci, Cj, sc.cosmin);
        }
      }
      status = found ? 0 : 3;
    }
    for (int k = 0; k < m; ++k) {
      const bool inl = status == 0 && ((S >> k) & 1u);
      flags[k] = inl ? 1 : 0;
      if (inl) o.point_of_row[rows[k]] = t;
    }
    write_track(in, o, t, status, X, sum / (double)(nin > 0 ? nin : 1), nin, used, taken, converged,
                S != given ? 1 : 0);
  }
}

__device__ __forceinline__ int wave_add(int v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += pf_shfl_xor(v, o, 64);
  return v;
}

// one track per wave (a workgroup is one wave).  A workgroup takes 64
// consecutive tracks at a time and works through those that are its kind.
__global__ __launch_bounds__(64) void ref_wave_kernel(Scene sc, TrackIn in, TrackOut o) {
  __shared__ int32_t srow[MAX_TRACK];   // the members
  __shared__ uint8_t sflag[MAX_TRACK];  // the current set
  __shared__ double ebuf[MAX_TRACK];    // the pixel errors of the last test
  const int T = tracks_of(sc, in), lane = threadIdx.x;
  for (long long base = (long long)blockIdx.x * 64; base < T; base += (long long)gridDim.x * 64) {
    const long long mine = base + lane;
    bool todo_mine = false;
    if (mine < T) {
      const int off = in.track_off[mine], m = in.track_off[mine + 1] - off;
      todo_mine = range_ok(sc, off, m) && m > LANE_TRACK;
    }
    unsigned long long todo = __ballot(todo_mine);
    while (todo) {
      const int t = (int)base + (__ffsll((long long)todo) - 1);
      todo &= todo - 1;
      const int off = in.track_off[t], m = in.track_off[t + 1] - off;  // LANE_TRACK < m <= MAX_TRACK
      uint8_t* flags = o.obs_inlier + off;
      double X[3] = {0.0, 0.0, 0.0};
      if (in.tinfo[4 * (long long)t] != 0) {  // the whole wave
        for (int k = lane; k < m; k += 64) flags[k] = 0;
        if (lane == 0) write_track(in, o, t, 1, X, 0.0, 0, 0, 0, 0, 0);
        continue;
      }
      __syncthreads();  // the track before is done with the LDS
      for (int k = lane; k < m; k += 64) {
        const int row = in.track_rows[off + k];
        srow[k] = row;
        sflag[k] = (in.flags[off + k] != 0 && row_valid(sc, row)) ? 1 : 0;
      }
      // a lane reads back only the entries it wrote until the barrier below
      int cnt = 0;
      for (int k = lane; k < m; k += 64) cnt += sflag[k];
      cnt = wave_add(cnt);
#pragma unroll
      for (int c = 0; c < 3; ++c) X[c] = in.points[3 * (long long)t + c];
      // the sums over the set at Y: a lane over its members in ascending order,
      // then the xor butterfly: every lane ends with the same bits
      auto accumulate = [&](const double (&Y)[3], double (&acc)[ACC]) {
        acc_zero(acc);
        bool ok = true;
        for (int k = lane; k < m; k += 64)
          if (sflag[k]) ok = row_acc(sc, srow[k], Y, acc) && ok;
#pragma unroll
        for (int i = 0; i < ACC; ++i) {
          double v = acc[i];
#pragma unroll
          for (int s = 32; s > 0; s >>= 1) v = v + pf_shfl_xor(v, s, 64);
          acc[i] = v;
        }
        return __ballot(!ok) == 0ull;
      };
      int used = 0, taken = 0, converged = 0, status = 0, nin = 0;
      for (int round = 0; round < sc.rounds; ++round) {  // uniform: every exit is on wave-wide values
        ++used;
        if (cnt >= 2) {
          double cost;
          taken += lm_round(X, sc.steps, accumulate, cost);
        }
        int c1 = 0;
        bool same = true;
        for (int k = lane; k < m; k += 64) {
          double e;
          const bool inl = row_inlier(sc, srow[k], X, e);
          same = same && (inl ? 1 : 0) == sflag[k];
          sflag[k] = inl ? 1 : 0;
          ebuf[k] = e;
          c1 += inl ? 1 : 0;
        }
        cnt = nin = wave_add(c1);
        const bool all_same = __ballot(!same) == 0ull;
        if (nin < 2) {
          status = 2;
          break;
        }
        if (all_same) {
          converged = 1;
          break;
        }
      }
      __syncthreads();  // sflag and ebuf are read across lanes from here
      if (status == 0) {
        bool found = false;
        for (int i = 0; i < m; ++i) {
          if (!sflag[i]) continue;
          double Ci[3];
          row_centre(sc, srow[i], Ci);
          for (int j = i + 1 + lane; j < m; j += 64) {
            if (!sflag[j]) continue;
            double Cj[3];
            row_centre(sc, srow[j], Cj);
            found = found || pftri::angle_ok(X, Ci, Cj, sc.cosmin);
          }
          if (__ballot(found) != 0ull) break;
        }
        status = __ballot(found) != 0ull ? 0 : 3;
      }
      bool changed = false;
      for (int k = lane; k < m; k += 64) {
        changed = changed || (in.flags[off + k] != 0) != (sflag[k] != 0);
        const bool inl = status == 0 && sflag[k];
        flags[k] = inl ? 1 : 0;
        if (inl) o.point_of_row[srow[k]] = t;
      }
      const int any_changed = __ballot(changed) != 0ull ? 1 : 0;
      if (lane == 0) {
        double sum = 0.0;
        for (int k = 0; k < m; ++k)  // member order
          if (sflag[k]) sum = sum + ebuf[k];
        write_track(in, o, t, status, X, sum / (double)(nin > 0 ? nin : 1), nin, used, taken,
                    converged, any_changed);
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

extern "C" int posfeat_refine_point(const double* obs, int n, const double* X0, int steps, double* X,
                                    double* cost) {
  if (!obs || !X0 || !X || !cost || n < 2 || steps < MIN_STEPS || steps > MAX_STEPS)
    return POSFEAT_E_INVALID;
  double x[3] = {X0[0], X0[1], X0[2]}, c;
  const int taken = pfrefine::lm_round(
      x, steps,
      [&](const double (&Y)[3], double (&acc)[ACC]) { return accumulate_rows(obs, n, Y, acc); }, c);
  X[0] = x[0], X[1] = x[1], X[2] = x[2];
  *cost = c;
  return taken;
}

extern "C" size_t posfeat_refine_points_workspace(const int32_t* set_off, int nsets, long long tmax,
                                                  long long mmax) {
  pfrefine::Layout L;
  if (pfrefine::layout(set_off, nsets, tmax, mmax, L) != 0) return 0;
  return L.total;
}

extern "C" int posfeat_refine_points(const float* kp, const int32_t* set_off, int nsets,
                                     const double* cams, const double* poses,
                                     const double* points_in, const int32_t* tinfo_in,
                                     const int32_t* track_off, const int32_t* track_rows,
                                     const uint8_t* inlier_in, const int32_t* counts_in,
                                     long long tmax, long long mmax, double thr,
                                     double min_angle_deg, int rounds, int steps, double* points,
                                     double* err, int32_t* tinfo, uint8_t* obs_inlier,
                                     int32_t* point_of_row, int32_t* rinfo, int32_t* counts, void* ws,
                                     size_t ws_bytes, void* stream) {
  pfrefine::Layout L;
  if (pfrefine::layout(set_off, nsets, tmax, mmax, L) != 0) return POSFEAT_E_INVALID;
  if ((!kp && L.n > 0) || ((!cams || !poses) && nsets > 0) || !points_in || !tinfo_in || !track_off ||
      !track_rows || !inlier_in || !counts_in || !points || !err || !tinfo || !obs_inlier ||
      !point_of_row || !rinfo || !counts || !ws)
    return POSFEAT_E_INVALID;
  if (!pfrefine::params_ok(thr, min_angle_deg, rounds, steps)) return POSFEAT_E_INVALID;
  const uintptr_t a8 = reinterpret_cast<uintptr_t>(points_in) | reinterpret_cast<uintptr_t>(points) |
                       reinterpret_cast<uintptr_t>(err) | reinterpret_cast<uintptr_t>(cams) |
                       reinterpret_cast<uintptr_t>(poses);
  const uintptr_t a4 = reinterpret_cast<uintptr_t>(tinfo_in) | reinterpret_cast<uintptr_t>(track_off) |
                       reinterpret_cast<uintptr_t>(track_rows) |
                       reinterpret_cast<uintptr_t>(counts_in) | reinterpret_cast<uintptr_t>(tinfo) |
                       reinterpret_cast<uintptr_t>(point_of_row) | reinterpret_cast<uintptr_t>(rinfo) |
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
  Scene sc{kp,          setid,  cams,  poses,     L.n,
           mmax,        (int)tmax, rounds, steps, thr * thr,
           cos(min_angle_deg * 3.14159265358979323846 / 180.0)};
  TrackIn in{points_in, tinfo_in, track_off, track_rows, inlier_in, counts_in};
  TrackOut o{points, err, tinfo, obs_inlier, point_of_row, rinfo, counts};
  hipLaunchKernelGGL(ref_init_kernel, dim3(grid_for(L.n, 256, 0x7fffffffu)), dim3(256), 0, st,
                     set_tab, nsets, sc, in, setid, point_of_row, counts);
  PF_CHECK_LAUNCH();
  hipLaunchKernelGGL(ref_lane_kernel, dim3(grid_for(tmax, 64, 8192)), dim3(64), 0, st, sc, in, o);
  PF_CHECK_LAUNCH();
  // a workgroup per 64 consecutive tracks, which is how the kernel deals them
  hipLaunchKernelGGL(ref_wave_kernel, dim3(grid_for(tmax, 64, 1u << 16)), dim3(64), 0, st, sc, in, o);
  PF_CHECK_LAUNCH();
  return POSFEAT_OK;
}
