// matchpairs.hip -- the evaluation matchers over a whole pair list, and the
// HPatches reprojection check, on gfx950.
//
// Replaces the per-pair loops of evaluations/hpatches/evaluation.py:49-90
// (mnn_matcher of image 1 against images 2..6 of every sequence, then the
// homography check of lines 69-90) and of
// evaluations/aachen/reconstruct_pipeline.py match_features (one matcher call
// per listed pair).  posfeat_match (match.hip) costs five launches, three
// allocations and a blocking read of the count per pair; here a pair list of
// any length is one plan upload and four launches:
//
//   mp_top2_kernel    a flat grid of tiles (match_plan.h): each names a side of
//                     a pair, a 128-column block and an A-row range and runs
//                     match_tile_top2 -- the tile loop of match_top2_kernel
//                     (match_tile.h: B fragments resident in VGPRs, A streamed
//                     through double-buffered LDS by global_load_lds with the
//                     XOR swizzle, v_mfma_f32_32x32x2_f32 in the same k order,
//                     strict '>' fold in increasing row order).  Each
//                     similarity is one full K = 128 chain whatever the range,
//                     so the bits equal posfeat_match's.
//   mp_merge_kernel   folds the partials of the sides that were split, in
//                     split order (skipped when no side is split).
//   mp_select_kernel  one workgroup per pair: match_select_pair.
//
// The A-row split is chosen for the whole grid (match_plan.h), not per pair:
// with hundreds of pairs no side is split.
//
// posfeat_match_pairs_guided is the same plan and the same launches with the
// candidates of each pair restricted by its 3x3 model (guided_solve.h):
// gd_record_kernel builds one fp32x4 record per keypoint per pair side in
// fp64, gd_top2_kernel<GUIDE> is mp_top2_kernel on match_tile_top2_g<GUIDE>
// (the step's records beside its descriptors in LDS, the fp32 predicate in the
// fold), mp_merge_kernel as is, gd_select_kernel = match_select_pair<true>.
//
// posfeat_reproj_hist: one workgroup per pair; per match the fp64 projection
// and distance of evaluation.py:71-78, binned by ceil(dist) with LDS integer
// atomics and prefix-summed into the cumulative counts of lines 86-90.
#include <vector>

#include "match_plan.h"
#include "match_tile.h"

namespace {

using namespace pfmatch;
using pfmatch_plan::Plan;
using pfmatch_plan::Side;
using pfmatch_plan::Tile;

static_assert(pfmatch_plan::PCOLS == MCOLS && pfmatch_plan::PSTEP == MSTEP,
              "match_plan.h tiles are match_tile.h tiles");
static_assert(sizeof(Side) == 48 && sizeof(Tile) == 16, "device table layout");

struct SideOut {
  int* nn;
  float* v1;
  float* v2;
};
__device__ __forceinline__ SideOut side_out(char* merged, const Side& s) {
  char* b = merged + s.out_off * 12;
  return SideOut{reinterpret_cast<int*>(b), reinterpret_cast<float*>(b + (size_t)s.nb * 4),
                 reinterpret_cast<float*>(b + (size_t)s.nb * 8)};
}

__global__ __launch_bounds__(256) void mp_top2_kernel(const float* __restrict__ desc,
                                                      const Side* __restrict__ sides,
                                                      const Tile* __restrict__ tiles,
                                                      char* __restrict__ merged,
                                                      char* __restrict__ parts) {
  __shared__ __attribute__((aligned(16))) float As[2 * MSTEP * MD];  // 2 x 32 KB
  const Tile t = tiles[blockIdx.x];
  const Side s = sides[t.side];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = t.cb * MCOLS + wave * 32 + (lane & 31);
  const int r0 = t.split * s.rps;
  const int r1 = s.na - r0 > s.rps ? r0 + s.rps : s.na;
  const Top2 best = match_tile_top2(desc + (long long)s.a_off * MD, r0, r1,
                                    desc + (long long)s.b_off * MD, s.nb, col, As);
  if ((lane >> 5) == 0 && col < s.nb) {
    if (s.nsplit == 1) {  // the only range of this side: its final statistics
      const SideOut o = side_out(merged, s);
      o.nn[col] = best.i1;
      o.v1[col] = best.v1;
      o.v2[col] = best.v2;
    } else {
      char* b = parts + s.part_off * 12;
      const size_t plane = (size_t)s.nsplit * s.nb * 4;
      const size_t p = (size_t)t.split * s.nb + col;
      reinterpret_cast<float*>(b)[p] = best.v1;
      reinterpret_cast<int*>(b + plane)[p] = best.i1;
      reinterpret_cast<float*>(b + 2 * plane)[p] = best.v2;
    }
  }
}

// one thread per merged entry: find its side, fold the partials in split order
__global__ void mp_merge_kernel(const Side* __restrict__ sides, int nsides, long long entries,
                                char* __restrict__ merged, const char* __restrict__ parts) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= entries) return;
  int lo = 0, hi = nsides - 1;  // the last side with out_off <= e (empty sides precede it)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (sides[mid].out_off <= e) lo = mid; else hi = mid - 1;
  }
  const Side s = sides[lo];
  const int c = (int)(e - s.out_off);
  if (s.nsplit <= 1 || c >= s.nb) return;
  const char* b = parts + s.part_off * 12;
  const size_t plane = (size_t)s.nsplit * s.nb * 4;
  const float* pv1 = reinterpret_cast<const float*>(b);
  const int* pi1 = reinterpret_cast<const int*>(b + plane);
  const float* pv2 = reinterpret_cast<const float*>(b + 2 * plane);
  Top2 t{pv1[c], pi1[c], pv2[c]};
  for (int k = 1; k < s.nsplit; ++k) {
    const size_t p = (size_t)k * s.nb + c;
    t = top2_merge(t, Top2{pv1[p], pi1[p], pv2[p]});
  }
  const SideOut o = side_out(merged, s);
  o.nn[c] = t.i1;
  o.v1[c] = t.v1;
  o.v2[c] = t.v2;
}

__global__ __launch_bounds__(1024) void mp_select_kernel(const Side* __restrict__ sides,
                                                         char* __restrict__ merged, int mode,
                                                         float ratio, int* __restrict__ matches,
                                                         int* __restrict__ counts) {
  __shared__ int off[1024];
  const int p = blockIdx.x;
  const Side r = sides[2 * p], c = sides[2 * p + 1];
  if (r.nb <= 0 || c.nb <= 0) {  // an empty side: no matches
    if (threadIdx.x == 0) counts[p] = 0;
    return;
  }
  const SideOut ro = side_out(merged, r), co = side_out(merged, c);
  match_select_pair(ro.nn, ro.v1, ro.v2, co.nn, co.v1, co.v2, r.nb, c.nb, mode, ratio,
                    matches + 2 * (long long)r.moff, counts + p, off);
}

// ---- guided matching (posfeat_match_pairs_guided) ---------------------------
// The records of pair p lie at rec_off entries of the record plane: rec1[n1]
// (image 1 = set s1) then rec2[n2]; a pair with an empty side has none.
struct GuidePair {  // 32 bytes
  int64_t rec_off;
  int32_t off1, n1, off2, n2, pad[2];
};
static_assert(sizeof(GuidePair) == 32, "device table layout");

// one thread per record: find its pair, build it in fp64 (guided_solve.h)
__global__ void gd_record_kernel(const float* __restrict__ kp, const double* __restrict__ M,
                                 const GuidePair* __restrict__ gp, int npairs, long long total,
                                 int model, f32x4* __restrict__ rec) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  int lo = 0, hi = npairs - 1;  // the last pair with rec_off <= e (empty pairs precede it)
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (gp[mid].rec_off <= e) lo = mid; else hi = mid - 1;
  }
  const GuidePair g = gp[lo];
  const int k = (int)(e - g.rec_off);
  if (k >= g.n1 + g.n2) return;
  const int side = k < g.n1 ? 0 : 1;
  const float* pt = kp + 2 * ((long long)(side ? g.off2 : g.off1) + (side ? k - g.n1 : k));
  double m[9];
#pragma unroll
  for (int i = 0; i < 9; ++i) m[i] = M[(long long)lo * 9 + i];
  float r[4];
  pfguided::record(model, side, m, pt[0], pt[1], r);
  rec[e] = f32x4{r[0], r[1], r[2], r[3]};
}

template <int GUIDE>
__global__ __launch_bounds__(256) void gd_top2_kernel(
    const float* __restrict__ desc, const float* __restrict__ kp, const Side* __restrict__ sides,
    const Tile* __restrict__ tiles, const GuidePair* __restrict__ gp,
    const f32x4* __restrict__ rec, float t2, char* __restrict__ merged, char* __restrict__ parts) {
  __shared__ __attribute__((aligned(16))) float As[2 * MSTEP * MD];  // 2 x 32 KB
  __shared__ __attribute__((aligned(16))) float Rs[2 * MSTEP * 4];   // 2 x 1 KB
  const Tile t = tiles[blockIdx.x];
  const Side s = sides[t.side];
  const GuidePair g = gp[t.side >> 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int col = t.cb * MCOLS + wave * 32 + (lane & 31);
  const int r0 = t.split * s.rps;
  const int r1 = s.na - r0 > s.rps ? r0 + s.rps : s.na;
  // side 2p streams image 2 against the columns of image 1, side 2p + 1 the reverse
  const bool rows = (t.side & 1) == 0;
  const f32x4* arec = rec + g.rec_off + (rows ? g.n1 : 0);
  const f32x4* brec = rec + g.rec_off + (rows ? 0 : g.n1);
  const int cc = min(col, s.nb - 1);
  const f32x4 rc = brec[cc];
  GuideCol gc;
  if constexpr (GUIDE == GUIDE_F) {
    const float* pt = kp + 2 * ((long long)s.b_off + cc);
    gc = GuideCol{pt[0], pt[1], rc[3], t2};
  } else {
    gc = GuideCol{rc[0], rc[1], 0.f, t2};
  }
  const Top2 best = match_tile_top2_g<GUIDE>(desc + (long long)s.a_off * MD, r0, r1,
                                             desc + (long long)s.b_off * MD, s.nb, col, As, arec,
                                             Rs, gc);
  if ((lane >> 5) == 0 && col < s.nb) {
    if (s.nsplit == 1) {
      const SideOut o = side_out(merged, s);
      o.nn[col] = best.i1;
      o.v1[col] = best.v1;
      o.v2[col] = best.v2;
    } else {
      char* b = parts + s.part_off * 12;
      const size_t plane = (size_t)s.nsplit * s.nb * 4;
      const size_t p = (size_t)t.split * s.nb + col;
      reinterpret_cast<float*>(b)[p] = best.v1;
      reinterpret_cast<int*>(b + plane)[p] = best.i1;
      reinterpret_cast<float*>(b + 2 * plane)[p] = best.v2;
    }
  }
}

__global__ __launch_bounds__(1024) void gd_select_kernel(const Side* __restrict__ sides,
                                                         char* __restrict__ merged, int mode,
                                                         float ratio, int* __restrict__ matches,
                                                         int* __restrict__ counts) {
  __shared__ int off[1024];
  const int p = blockIdx.x;
  const Side r = sides[2 * p], c = sides[2 * p + 1];
  if (r.nb <= 0 || c.nb <= 0) {
    if (threadIdx.x == 0) counts[p] = 0;
    return;
  }
  const SideOut ro = side_out(merged, r), co = side_out(merged, c);
  match_select_pair<true>(ro.nn, ro.v1, ro.v2, co.nn, co.v1, co.v2, r.nb, c.nb, mode, ratio,
                          matches + 2 * (long long)r.moff, counts + p, off);
}

// the guided call's workspace: the plan's, then the GuidePair table, then the records
struct GuideLayout {
  size_t gp_off, rec_off, total_bytes;
  long long nrec;
};
GuideLayout guide_layout(const Plan& pl, int npairs) {
  GuideLayout L;
  L.nrec = 0;
  for (int p = 0; p < npairs; ++p) L.nrec += (long long)pl.sides[2 * (size_t)p].nb + pl.sides[2 * (size_t)p].na;
  L.gp_off = pf_align(pl.total_bytes, 256);
  L.rec_off = L.gp_off + pf_align((size_t)npairs * sizeof(GuidePair), 256);
  L.total_bytes = L.rec_off + pf_align((size_t)L.nrec * 16, 256) + 256;
  return L;
}

struct ReprojPair {  // 32 bytes
  int32_t a_off, n1, b_off, n2, moff, pad[3];
};

__global__ __launch_bounds__(256) void reproj_hist_kernel(const float* __restrict__ kp,
                                                          const ReprojPair* __restrict__ tab,
                                                          const int* __restrict__ matches,
                                                          const int* __restrict__ counts,
                                                          const double* __restrict__ H, int nthr,
                                                          int* __restrict__ hist) {
  __shared__ int bins[32];
  const int p = blockIdx.x, tid = threadIdx.x;
  if (tid < 32) bins[tid] = 0;
  __syncthreads();
  const ReprojPair q = tab[p];
  const double* h = H + (long long)p * 9;
  const double h0 = h[0], h1 = h[1], h2 = h[2], h3 = h[3], h4 = h[4], h5 = h[5], h6 = h[6],
               h7 = h[7], h8 = h[8];
  const int cnt = min(counts[p], q.n1);
  const int* mp = matches + 2 * (long long)q.moff;
  for (int m = tid; m < cnt; m += 256) {
    const int ia = mp[2 * m], ib = mp[2 * m + 1];
    if ((unsigned)ia >= (unsigned)q.n1 || (unsigned)ib >= (unsigned)q.n2) continue;
    const float* pa = kp + 2 * ((long long)q.a_off + ia);
    const float* pb = kp + 2 * ((long long)q.b_off + ib);
    const double xa = pa[0], ya = pa[1], xb = pb[0], yb = pb[1];
    const double px = h0 * xa + h1 * ya + h2, py = h3 * xa + h4 * ya + h5,
                 pz = h6 * xa + h7 * ya + h8;
    const double dx = xb - px / pz, dy = yb - py / pz;
    const double d = sqrt(dx * dx + dy * dy);
    // dist <= t for the integers t >= ceil(dist); NaN / inf fail the test
    if (d <= (double)nthr) atomicAdd(&bins[max(1, (int)ceil(d)) - 1], 1);
  }
  __syncthreads();
  if (tid < nthr) {
    int c = 0;
    for (int t = 0; t <= tid; ++t) c += bins[t];
    hist[(long long)p * nthr + tid] = c;
  }
}

}  // namespace

extern "C" size_t posfeat_match_pairs_workspace(const int32_t* set_off, int nsets,
                                                const int32_t* pairs, int npairs) {
  Plan pl;
  if (pfmatch_plan::build_plan(set_off, nsets, pairs, npairs, false, pl) != 0) return 0;
  return pl.total_bytes;
}

extern "C" int posfeat_match_pairs_splits(const int32_t* set_off, int nsets, const int32_t* pairs,
                                          int npairs, int32_t* nsplit) {
  Plan pl;
  if (!nsplit || pfmatch_plan::build_plan(set_off, nsets, pairs, npairs, false, pl) != 0)
    return POSFEAT_E_INVALID;
  for (size_t i = 0; i < pl.sides.size(); ++i) nsplit[i] = pl.sides[i].nsplit;
  return POSFEAT_OK;
}

extern "C" int posfeat_match_pairs(const float* desc, const int32_t* set_off, int nsets,
                                   const int32_t* pairs, int npairs, int dim, int mode, float ratio,
                                   int32_t* matches, int32_t* counts, void* ws, size_t ws_bytes,
                                   void* stream) {
  if (!desc || !set_off || !pairs || !matches || !counts || !ws || nsets <= 0 || npairs <= 0)
    return POSFEAT_E_INVALID;
  if (dim != MD || mode < 0 || mode > 2) return POSFEAT_E_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(desc) & 15) || (reinterpret_cast<uintptr_t>(ws) & 255))
    return POSFEAT_E_INVALID;
  Plan pl;
  if (pfmatch_plan::build_plan(set_off, nsets, pairs, npairs, true, pl) != 0)
    return POSFEAT_E_INVALID;
  if (ws_bytes < pl.total_bytes) return POSFEAT_E_WORKSPACE;
  hipStream_t st = pf_stream(stream);
  char* w = static_cast<char*>(ws);
  // the runtime has read a pageable source when the copy call returns (as
  // posfeat_detect's threshold table relies on), so the plan may die with us
  if (hipMemcpyAsync(w, pl.sides.data(), pl.sides.size() * sizeof(Side), hipMemcpyHostToDevice,
                     st) != hipSuccess)
    return POSFEAT_E_HIP;
  if (pl.ntiles > 0 &&
      hipMemcpyAsync(w + pl.tiles_off, pl.tiles.data(), pl.tiles.size() * sizeof(Tile),
                     hipMemcpyHostToDevice, st) != hipSuccess)
    return POSFEAT_E_HIP;
  const Side* sides = reinterpret_cast<const Side*>(w);
  const Tile* tiles = reinterpret_cast<const Tile*>(w + pl.tiles_off);
  char* merged = w + pl.merged_off;
  char* parts = w + pl.part_off;
  if (pl.ntiles > 0) {
    hipLaunchKernelGGL(mp_top2_kernel, dim3((unsigned)pl.ntiles), dim3(256), 0, st, desc, sides,
                       tiles, merged, parts);
    PF_CHECK_LAUNCH();
  }
  if (pl.part_entries > 0) {
    const long long blocks = (pl.merged_entries + 255) / 256;
    if (blocks > INT32_MAX) return POSFEAT_E_INVALID;
    hipLaunchKernelGGL(mp_merge_kernel, dim3((unsigned)blocks), dim3(256), 0, st, sides,
                       (int)pl.sides.size(), (long long)pl.merged_entries, merged, parts);
    PF_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(mp_select_kernel, dim3(npairs), dim3(1024), 0, st, sides, merged, mode, ratio,
                     matches, counts);
  PF_CHECK_LAUNCH();
  return POSFEAT_OK;
}

extern "C" size_t posfeat_match_pairs_guided_workspace(const int32_t* set_off, int nsets,
                                                       const int32_t* pairs, int npairs) {
  Plan pl;
  if (pfmatch_plan::build_plan(set_off, nsets, pairs, npairs, false, pl) != 0) return 0;
  return guide_layout(pl, npairs).total_bytes;
}

extern "C" int posfeat_guided_record(int model, int side, const double* M, const float* pt,
                                     float* rec) {
  if (!M || !pt || !rec || side < 0 || side > 1) return POSFEAT_E_INVALID;
  if (model < 0 || model > 1) return POSFEAT_E_UNSUPPORTED;
  float r[4];
  pfguided::record(model, side, M, pt[0], pt[1], r);
  for (int i = 0; i < 4; ++i) rec[i] = r[i];
  return POSFEAT_OK;
}

extern "C" int posfeat_guided_admissible(int model, const float* ra, const float* col,
                                         double thr) {
  if (!ra || !col || !(thr > 0.0) || !(thr < (double)INFINITY)) return POSFEAT_E_INVALID;
  if (model < 0 || model > 1) return POSFEAT_E_UNSUPPORTED;
  const float t2 = (float)(thr * thr);
  return model == pfguided::FUNDAMENTAL
             ? pfguided::admissible<pfguided::FUNDAMENTAL>(ra[0], ra[1], ra[2], ra[3], col[0],
                                                           col[1], col[2], t2)
             : pfguided::admissible<pfguided::HOMOGRAPHY>(ra[0], ra[1], ra[2], ra[3], col[0],
                                                          col[1], col[2], t2);
}

extern "C" int posfeat_match_pairs_guided(const float* desc, const float* kp,
                                          const int32_t* set_off, int nsets, const int32_t* pairs,
                                          int npairs, int dim, int mode, float ratio, int model,
                                          const double* M, double thr, int32_t* matches,
                                          int32_t* counts, void* ws, size_t ws_bytes,
                                          void* stream) {
  if (!desc || !kp || !M || !set_off || !pairs || !matches || !counts || !ws || nsets <= 0 ||
      npairs <= 0)
    return POSFEAT_E_INVALID;
  if (dim != MD || mode < 0 || mode > 2 || model < 0 || model > 1) return POSFEAT_E_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(desc) & 15) || (reinterpret_cast<uintptr_t>(ws) & 255) ||
      (reinterpret_cast<uintptr_t>(M) & 7))
    return POSFEAT_E_INVALID;
  if (!(thr > 0.0) || !(thr < (double)INFINITY)) return POSFEAT_E_INVALID;
  Plan pl;
  if (pfmatch_plan::build_plan(set_off, nsets, pairs, npairs, true, pl) != 0)
    return POSFEAT_E_INVALID;
  const GuideLayout L = guide_layout(pl, npairs);
  if (ws_bytes < L.total_bytes) return POSFEAT_E_WORKSPACE;
  std::vector<GuidePair> gtab((size_t)npairs);
  long long nrec = 0;
  for (int p = 0; p < npairs; ++p) {
    const Side& r = pl.sides[2 * (size_t)p];  // B = set s1, A = set s2
    gtab[p] = GuidePair{nrec, r.b_off, r.nb, r.a_off, r.na, {0, 0}};
    nrec += (long long)r.nb + r.na;
  }
  hipStream_t st = pf_stream(stream);
  char* w = static_cast<char*>(ws);
  // pageable sources, read by the runtime before the copy calls return (as in
  // posfeat_match_pairs), so the tables may die with us
  if (hipMemcpyAsync(w, pl.sides.data(), pl.sides.size() * sizeof(Side), hipMemcpyHostToDevice,
                     st) != hipSuccess)
    return POSFEAT_E_HIP;
  if (pl.ntiles > 0 &&
      hipMemcpyAsync(w + pl.tiles_off, pl.tiles.data(), pl.tiles.size() * sizeof(Tile),
                     hipMemcpyHostToDevice, st) != hipSuccess)
    return POSFEAT_E_HIP;
  if (hipMemcpyAsync(w + L.gp_off, gtab.data(), gtab.size() * sizeof(GuidePair),
                     hipMemcpyHostToDevice, st) != hipSuccess)
    return POSFEAT_E_HIP;
  const Side* sides = reinterpret_cast<const Side*>(w);
  const Tile* tiles = reinterpret_cast<const Tile*>(w + pl.tiles_off);
  const GuidePair* gp = reinterpret_cast<const GuidePair*>(w + L.gp_off);
  f32x4* rec = reinterpret_cast<f32x4*>(w + L.rec_off);
  char* merged = w + pl.merged_off;
  char* parts = w + pl.part_off;
  const float t2 = (float)(thr * thr);
  if (nrec > 0) {
    const long long blocks = (nrec + 255) / 256;
    if (blocks > INT32_MAX) return POSFEAT_E_INVALID;
    hipLaunchKernelGGL(gd_record_kernel, dim3((unsigned)blocks), dim3(256), 0, st, kp, M, gp,
                       npairs, nrec, model, rec);
    PF_CHECK_LAUNCH();
  }
  if (pl.ntiles > 0) {
    if (model == pfguided::FUNDAMENTAL)
      hipLaunchKernelGGL(gd_top2_kernel<GUIDE_F>, dim3((unsigned)pl.ntiles), dim3(256), 0, st, desc,
                         kp, sides, tiles, gp, rec, t2, merged, parts);
    else
      hipLaunchKernelGGL(gd_top2_kernel<GUIDE_H>, dim3((unsigned)pl.ntiles), dim3(256), 0, st, desc,
                         kp, sides, tiles, gp, rec, t2, merged, parts);
    PF_CHECK_LAUNCH();
  }
  if (pl.part_entries > 0) {
    const long long blocks = (pl.merged_entries + 255) / 256;
    if (blocks > INT32_MAX) return POSFEAT_E_INVALID;
    hipLaunchKernelGGL(mp_merge_kernel, dim3((unsigned)blocks), dim3(256), 0, st, sides,
                       (int)pl.sides.size(), (long long)pl.merged_entries, merged, parts);
    PF_CHECK_LAUNCH();
  }
  hipLaunchKernelGGL(gd_select_kernel, dim3(npairs), dim3(1024), 0, st, sides, merged, mode, ratio,
                     matches, counts);
  PF_CHECK_LAUNCH();
  return POSFEAT_OK;
}

extern "C" size_t posfeat_reproj_hist_workspace(int npairs) {
  return npairs > 0 ? pf_align((size_t)npairs * sizeof(ReprojPair), 256) : 0;
}

extern "C" int posfeat_reproj_hist(const float* kp, const int32_t* set_off, int nsets,
                                   const int32_t* pairs, int npairs, const int32_t* matches,
                                   const int32_t* counts, const double* H, int nthr, int32_t* hist,
                                   void* ws, size_t ws_bytes, void* stream) {
  if (!kp || !set_off || !pairs || !matches || !counts || !H || !hist || !ws || nsets <= 0 ||
      npairs <= 0 || nthr < 1 || nthr > 32)
    return POSFEAT_E_INVALID;
  if ((reinterpret_cast<uintptr_t>(ws) & 255) || (reinterpret_cast<uintptr_t>(H) & 7))
    return POSFEAT_E_INVALID;
  Plan pl;
  if (pfmatch_plan::build_plan(set_off, nsets, pairs, npairs, false, pl) != 0)
    return POSFEAT_E_INVALID;
  if (ws_bytes < posfeat_reproj_hist_workspace(npairs)) return POSFEAT_E_WORKSPACE;
  std::vector<ReprojPair> tab((size_t)npairs);
  for (int p = 0; p < npairs; ++p) {
    const Side& r = pl.sides[2 * (size_t)p];  // B = set s1, A = set s2
    tab[p] = ReprojPair{r.b_off, r.nb, r.a_off, r.na, r.moff, {0, 0, 0}};
  }
  hipStream_t st = pf_stream(stream);
  if (hipMemcpyAsync(ws, tab.data(), tab.size() * sizeof(ReprojPair), hipMemcpyHostToDevice, st) !=
      hipSuccess)
    return POSFEAT_E_HIP;
  hipLaunchKernelGGL(reproj_hist_kernel, dim3(npairs), dim3(256), 0, st, kp,
                     reinterpret_cast<const ReprojPair*>(ws), matches, counts, H, nthr, hist);
  PF_CHECK_LAUNCH();
  return POSFEAT_OK;
}
