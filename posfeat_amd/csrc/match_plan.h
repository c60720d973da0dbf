// match_plan.h -- host-side plan of posfeat_match_pairs (matchpairs.hip): the
// validation of the set / pair tables, the A-row split, the flat tile list and
// the workspace layout.  Plain C++ with no HIP call, so a stand-alone host
// program can check it (tests/host/match_plan_check.cpp).
//
// Side 2p of pair p = (s1, s2) is "rows of sim": for every d1 row (B = set s1)
// the top-2 over the d2 rows (A = set s2); side 2p + 1 is "columns" (B = s2,
// A = s1).  A tile is (side, 128-column block of B, A-row range).  A side whose
// A rows are not split writes its result directly; a split side writes one
// partial per range and the merge launch folds them.
//
// Workspace (byte offsets, each 256-B aligned):
//   [0, tab_bytes)             Side table then Tile table (uploaded per call)
//   [merged_off, +12 * E)      per side at out_off entries: nn[nb] v1[nb] v2[nb]
//   [part_off, +12 * P)        per split side at part_off entries:
//                              pv1[nsplit][nb] pi1[nsplit][nb] pv2[nsplit][nb]
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

namespace pfmatch_plan {

constexpr int PCOLS = 128;      // B rows per tile (match_tile.h MCOLS)
constexpr int PSTEP = 64;       // A-row granularity (match_tile.h MSTEP)
constexpr int PRESIDENT = 512;  // resident workgroups of the tile kernel (2 per CU)
constexpr int PMAXSPLIT = 32;   // at most this many row ranges per side

struct Side {            // 48 bytes, read by the device as is
  int32_t a_off, na;     // A rows: pool rows [a_off, a_off + na)
  int32_t b_off, nb;     // B rows
  int32_t rps, nsplit;   // rows per range (multiple of PSTEP), ranges
  int32_t moff, pad;     // first matches row of the pair
  int64_t part_off;      // entries; used when nsplit > 1
  int64_t out_off;       // entries
};

struct Tile {  // 16 bytes
  int32_t side, cb, split, pad;
};

struct Plan {
  std::vector<Side> sides;  // 2 * npairs (na = nb = 0 for a pair with an empty side)
  std::vector<Tile> tiles;
  int64_t ntiles = 0, merged_entries = 0, part_entries = 0, total_matches = 0;
  size_t tab_bytes = 0, tiles_off = 0, merged_off = 0, part_off = 0, total_bytes = 0;
};

inline size_t align256(size_t x) { return (x + 255) / 256 * 256; }
inline int cblocks(int n) { return (int)(((int64_t)n + PCOLS - 1) / PCOLS); }

// 0, or -1 (POSFEAT_E_INVALID) for a bad table.  want_tiles = false sizes the
// workspace without materialising the tile list.
inline int build_plan(const int32_t* set_off, int nsets, const int32_t* pairs, int npairs,
                      bool want_tiles, Plan& pl) {
  pl = Plan();
  if (!set_off || nsets < 0 || npairs < 0 || (npairs > 0 && !pairs)) return -1;
  if (set_off[0] < 0) return -1;
  for (int s = 0; s < nsets; ++s)
    if (set_off[s + 1] < set_off[s]) return -1;
  pl.sides.resize((size_t)2 * npairs);
  int64_t moff = 0, base_tiles = 0;
  int maxna = 0;
  for (int p = 0; p < npairs; ++p) {
    const int s1 = pairs[2 * p], s2 = pairs[2 * p + 1];
    if (s1 < 0 || s1 >= nsets || s2 < 0 || s2 >= nsets) return -1;
    const int n1 = set_off[s1 + 1] - set_off[s1], n2 = set_off[s2 + 1] - set_off[s2];
    if (moff > INT32_MAX) return -1;
    const bool live = n1 > 0 && n2 > 0;
    Side& r = pl.sides[2 * p];
    Side& c = pl.sides[2 * p + 1];
    r = Side{set_off[s2], live ? n2 : 0, set_off[s1], live ? n1 : 0, 0, 0, (int32_t)moff, 0, 0, 0};
    c = Side{set_off[s1], live ? n1 : 0, set_off[s2], live ? n2 : 0, 0, 0, (int32_t)moff, 0, 0, 0};
    moff += n1;
    if (live) {
      base_tiles += cblocks(n1) + cblocks(n2);
      maxna = std::max(maxna, std::max(n1, n2));
    }
  }
  if (moff > INT32_MAX) return -1;
  pl.total_matches = moff;
  // One row-range length R for the whole list, so tiles take about the same
  // time whichever pair they belong to: the longest R (fewest ranges) at which
  // the grid holds two rounds of resident workgroups; a long enough list is
  // not split at all.
  auto ranges = [](int na, int R) {
    return (int)std::min<int64_t>(PMAXSPLIT, ((int64_t)na + R - 1) / R);
  };
  int R = std::max(maxna, PSTEP);
  if (base_tiles < 2 * PRESIDENT) {
    for (int k = 2; k <= PMAXSPLIT; ++k) {
      const int Rk =
          (int)std::max<int64_t>(PSTEP, (((int64_t)maxna + k - 1) / k + PSTEP - 1) / PSTEP * PSTEP);
      R = Rk;
      int64_t t = 0;
      for (const Side& s : pl.sides)
        if (s.na > 0) t += (int64_t)(cblocks(s.nb)) * ranges(s.na, Rk);
      if (t >= 2 * PRESIDENT || Rk == PSTEP) break;
    }
  }
  int64_t out = 0, part = 0, ntiles = 0;
  for (Side& s : pl.sides) {
    s.out_off = out;
    s.part_off = part;
    if (s.na <= 0) continue;
    const int ns = ranges(s.na, R);
    s.rps = (int32_t)((((int64_t)s.na + ns - 1) / ns + PSTEP - 1) / PSTEP * PSTEP);
    s.nsplit = (int32_t)(((int64_t)s.na + s.rps - 1) / s.rps);
    out += s.nb;
    if (s.nsplit > 1) part += (int64_t)s.nsplit * s.nb;
    ntiles += (int64_t)(cblocks(s.nb)) * s.nsplit;
  }
  if (ntiles > INT32_MAX) return -1;
  pl.ntiles = ntiles;
  pl.merged_entries = out;
  pl.part_entries = part;
  pl.tiles_off = align256(pl.sides.size() * sizeof(Side));
  pl.tab_bytes = pl.tiles_off + align256((size_t)ntiles * sizeof(Tile));
  pl.merged_off = pl.tab_bytes;
  pl.part_off = pl.merged_off + align256((size_t)out * 12);
  pl.total_bytes = pl.part_off + align256((size_t)part * 12) + 256;
  if (want_tiles) {
    pl.tiles.reserve((size_t)ntiles);
    for (size_t i = 0; i < pl.sides.size(); ++i) {
      const Side& s = pl.sides[i];
      if (s.na <= 0) continue;
      const int ncb = cblocks(s.nb);
      for (int sp = 0; sp < s.nsplit; ++sp)
        for (int cb = 0; cb < ncb; ++cb) pl.tiles.push_back(Tile{(int32_t)i, cb, sp, 0});
    }
    // longest tiles first: the short ones fill the tail of the grid
    auto rows = [&](const Tile& t) {
      const Side& s = pl.sides[t.side];
      return std::min(s.na - t.split * s.rps, s.rps);
    };
    std::stable_sort(pl.tiles.begin(), pl.tiles.end(),
                     [&](const Tile& a, const Tile& b) { return rows(a) > rows(b); });
  }
  return 0;
}

}  // namespace pfmatch_plan
