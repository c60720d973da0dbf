// ransac_plan.h -- what the host and the kernels of posfeat_ransac_homography
// (ransac.hip) and posfeat_ransac_fundamental (fundamental.hip) share: the
// counter-based sampler, the validation of the set / pair tables and the
// workspace layout.  Plain C++ with no HIP call, so a
// stand-alone host program can check it (tests/host/ransac_plan_check.cpp);
// the sampler is also what posfeat_ransac_sample calls.
//
// Workspace (byte offsets, each 256-B aligned):
//   [0, pts_off)               Pair table (uploaded per call)
//   [pts_off, +16 * M)         per match row of the list (M = sum n1, pair p at
//                              moff[p]): x1 y1 x2 y2 fp32
//   [norm_off, +64 * npairs)   per pair 8 doubles: cx1 cy1 s1 cx2 cy2 s2 - -
//   [slot_off, +8 * npairs * nblk)  per (pair, hypothesis block) the packed
//                              (count, iteration) key of the block's best
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

#if defined(__HIPCC__)
#define PFR_HD __host__ __device__
#else
#define PFR_HD
#endif

namespace pfransac_plan {

constexpr int RBLOCK = 256;         // hypotheses per workgroup (one per lane)
constexpr int RTILE = 256;          // matches staged through LDS per tile (8 KB as doubles)
constexpr int RMAXITERS = 65536;    // so a pair has at most 256 block slots

PFR_HD inline uint64_t mix(uint64_t z) {  // splitmix64's finaliser
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the four distinct match indices in [0, n) of iteration `it` of pair `pair`
// (n >= 4): draw k is uniform over the n - k indices not drawn yet
PFR_HD inline void sample4(uint64_t seed, int pair, int it, int n, int32_t out[4]) {
  const uint64_t base = mix(mix(seed ^ mix((uint64_t)pair)) ^ (uint64_t)it);
  int32_t s0 = 0, s1 = 0, s2 = 0;  // the earlier draws, ascending
  for (int k = 0; k < 4; ++k) {
    const uint64_t r = mix(base ^ (uint64_t)k);
    int32_t j = (int32_t)(((r >> 32) * (uint64_t)(n - k)) >> 32);
    if (k > 0 && j >= s0) ++j;
    if (k > 1 && j >= s1) ++j;
    if (k > 2 && j >= s2) ++j;
    out[k] = j;
    // insert j into the ascending (s0, s1, s2)
    if (k == 0) {
      s0 = j;
    } else if (k == 1) {
      if (j < s0) { s1 = s0; s0 = j; } else { s1 = j; }
    } else if (k == 2) {
      if (j < s0) { s2 = s1; s1 = s0; s0 = j; }
      else if (j < s1) { s2 = s1; s1 = j; }
      else { s2 = j; }
    }
  }
}

// The sampler continued to K draws (4 <= K <= 8): the same base, the same mix,
// draw k uniform over the n - k indices not drawn yet (n >= K).  The first four
// draws are sample4's.  The earlier draws are kept ascending in s[]; every
// index is a compile-time constant once the loops are unrolled.
template <int K>
PFR_HD inline void sample_k(uint64_t seed, int pair, int it, int n, int32_t (&out)[K]) {
  static_assert(K >= 4 && K <= 8, "sample_k draws 4..8 indices");
  const uint64_t base = mix(mix(seed ^ mix((uint64_t)pair)) ^ (uint64_t)it);
  int32_t s[K];
#pragma unroll
  for (int k = 0; k < K; ++k) s[k] = 0;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    const uint64_t r = mix(base ^ (uint64_t)k);
    int32_t j = (int32_t)(((r >> 32) * (uint64_t)(n - k)) >> 32);
#pragma unroll
    for (int q = 0; q < k; ++q)
      if (j >= s[q]) ++j;
    out[k] = j;
    int pos = 0;  // the earlier draws below j
#pragma unroll
    for (int q = 0; q < k; ++q) pos += s[q] < j ? 1 : 0;
#pragma unroll
    for (int q = k; q > 0; --q) s[q] = q < pos ? s[q] : (q == pos ? j : s[q - 1]);
    s[0] = 0 < pos ? s[0] : j;
  }
}

// The slot key of a scored candidate when a sample yields several models
// (posfeat_ransac_fundamental: the up to three real roots of the 7-point
// cubic; two bits hold the root index): more
// inliers first, then the lower iteration, then the lower root index; 0 stays
// the key of "nothing scored".  it < RMAXITERS, so it * 4 + root fits easily.
PFR_HD inline unsigned long long slot_key_root(int cnt, int it, int root) {
  return ((unsigned long long)(unsigned)(cnt + 1) << 32) |
         (0xffffffffu - (((unsigned)it << 2) | (unsigned)root));
}
PFR_HD inline int slot_key_iter(unsigned long long key) {
  return (int)((0xffffffffu - (unsigned)key) >> 2);
}
PFR_HD inline int slot_key_rootidx(unsigned long long key) {
  return (int)((0xffffffffu - (unsigned)key) & 3u);
}

struct Pair {  // 32 bytes, read by the device as is
  int32_t a_off, n1;  // pool rows of set s1 (image 1)
  int32_t b_off, n2;  // pool rows of set s2
  int32_t moff;       // first matches / inlier row of the pair
  int32_t pad[3];
};

struct Plan {
  std::vector<Pair> tab;
  int nblk = 0;  // hypothesis blocks per pair
  int64_t total_matches = 0;
  size_t pts_off = 0, norm_off = 0, slot_off = 0, total_bytes = 0;
};

inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }

// 0, or -1 (POSFEAT_E_INVALID) for a bad table or iteration count: a null
// table, a negative or decreasing set_off, a set index out of range, sum n1
// past INT32_MAX, iters outside 1..RMAXITERS.
inline int build_plan(const int32_t* set_off, int nsets, const int32_t* pairs, int npairs,
                      int iters, Plan& pl) {
  pl = Plan();
  if (!set_off || nsets < 0 || npairs < 0 || (npairs > 0 && !pairs)) return -1;
  if (iters < 1 || iters > RMAXITERS) return -1;
  if (set_off[0] < 0) return -1;
  for (int s = 0; s < nsets; ++s)
    if (set_off[s + 1] < set_off[s]) return -1;
  pl.tab.resize((size_t)npairs);
  int64_t moff = 0;
  for (int p = 0; p < npairs; ++p) {
    const int s1 = pairs[2 * p], s2 = pairs[2 * p + 1];
    if (s1 < 0 || s1 >= nsets || s2 < 0 || s2 >= nsets) return -1;
    if (moff > INT32_MAX) return -1;
    const int n1 = set_off[s1 + 1] - set_off[s1], n2 = set_off[s2 + 1] - set_off[s2];
    pl.tab[p] = Pair{set_off[s1], n1, set_off[s2], n2, (int32_t)moff, {0, 0, 0}};
    moff += n1;
  }
  if (moff > INT32_MAX) return -1;
  pl.total_matches = moff;
  pl.nblk = (iters + RBLOCK - 1) / RBLOCK;
  pl.pts_off = align256((size_t)npairs * sizeof(Pair));
  pl.norm_off = pl.pts_off + align256((size_t)moff * 16);
  pl.slot_off = pl.norm_off + align256((size_t)npairs * 64);
  pl.total_bytes = pl.slot_off + align256((size_t)npairs * pl.nblk * 8) + 256;
  return 0;
}

// The plan of posfeat_ransac_fundamental: the same tables and the same
// workspace regions (the slots hold slot_key_root keys); FMINSET is the sample
// size, below which a pair has no model.
constexpr int FMINSET = 7;
inline int build_plan_fundamental(const int32_t* set_off, int nsets, const int32_t* pairs,
                                  int npairs, int iters, Plan& pl) {
  return build_plan(set_off, nsets, pairs, npairs, iters, pl);
}

// The slot key of posfeat_ransac_essential (essential.hip): a sample yields up
// to ten models, so four bits hold the root index.  The order is
// slot_key_root's: more inliers, then the lower iteration, then the lower root.
PFR_HD inline unsigned long long slot_key_root4(int cnt, int it, int root) {
  return ((unsigned long long)(unsigned)(cnt + 1) << 32) |
         (0xffffffffu - (((unsigned)it << 4) | (unsigned)root));
}
PFR_HD inline int slot_key_iter4(unsigned long long key) {
  return (int)((0xffffffffu - (unsigned)key) >> 4);
}
PFR_HD inline int slot_key_rootidx4(unsigned long long key) {
  return (int)((0xffffffffu - (unsigned)key) & 15u);
}

// The plan of posfeat_ransac_essential: the same Pair table (pad[0], pad[1]
// carry the two set indices, for the cameras) and hypothesis blocks; its own
// workspace, each region 256-B aligned:
//   [0, pts_off)                   Pair table (uploaded per call)
//   [pts_off, +32 * M)             per match row x y u v fp64, undistorted
//   [cnt_off, +4 * npairs * nblk)  candidate records of each hypothesis block
//   [rec_off, +EREC_BYTES * EBLOCK_RECS * npairs * nblk)  the records: per
//                                  block EBLOCK_RECS of 10 doubles (key, E)
//   [slot_off, +8 * npairs * nblk * ESUB)  per (pair, block, 256 records) the
//                                  best slot_key_root4 key
constexpr int EMINSET = 5;
constexpr int ESUB = 10;                      // candidates per sample at the most
constexpr int EBLOCK_RECS = RBLOCK * ESUB;    // records per hypothesis block at the most
constexpr int EREC_DOUBLES = 10;              // (it << 4 | root) as a double's bits, E[9]
struct EssPlan {
  Plan base;
  size_t cnt_off = 0, rec_off = 0, slot_off = 0, total_bytes = 0;
};
inline int build_plan_essential(const int32_t* set_off, int nsets, const int32_t* pairs,
                                int npairs, int iters, EssPlan& pl) {
  pl = EssPlan();
  if (build_plan(set_off, nsets, pairs, npairs, iters, pl.base) != 0) return -1;
  for (int p = 0; p < npairs; ++p) {
    pl.base.tab[p].pad[0] = pairs[2 * p];
    pl.base.tab[p].pad[1] = pairs[2 * p + 1];
  }
  const int64_t blocks = (int64_t)npairs * pl.base.nblk;
  if (blocks * ESUB > INT32_MAX) return -1;
  pl.cnt_off = pl.base.pts_off + align256((size_t)pl.base.total_matches * 32);
  pl.rec_off = pl.cnt_off + align256((size_t)blocks * 4);
  pl.slot_off = pl.rec_off + align256((size_t)blocks * EBLOCK_RECS * EREC_DOUBLES * 8);
  pl.total_bytes = pl.slot_off + align256((size_t)blocks * ESUB * 8) + 256;
  return 0;
}

}  // namespace pfransac_plan
