// Stand-alone check of posfeat_amd/csrc/match_plan.h (the host plan of
// posfeat_match_pairs), built with -fsanitize=address,undefined and run
// directly by tests/test_match_plan_host.py.  For every case it asserts that
// the tiles cover each (pair, side, column, A row) exactly once, that every
// offset a kernel derives from the plan lies inside the reported workspace and
// that no two sides' regions overlap.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <utility>
#include <vector>

#include "../../posfeat_amd/csrc/match_plan.h"

using namespace pfmatch_plan;

#define CHECK(c)                                                    \
  do {                                                              \
    if (!(c)) {                                                     \
      std::fprintf(stderr, "%s:%d: %s failed (case %s)\n", __FILE__, __LINE__, #c, g_case); \
      std::exit(1);                                                 \
    }                                                               \
  } while (0)

static const char* g_case = "";

static void check_case(const char* name, const std::vector<int>& sizes,
                       const std::vector<std::pair<int, int>>& pr, bool expect_split) {
  g_case = name;
  std::vector<int32_t> set_off(sizes.size() + 1, 0), pairs;
  for (size_t i = 0; i < sizes.size(); ++i) set_off[i + 1] = set_off[i] + sizes[i];
  for (auto& p : pr) {
    pairs.push_back(p.first);
    pairs.push_back(p.second);
  }
  const int nsets = (int)sizes.size(), npairs = (int)pr.size();
  Plan pl, sz;
  CHECK(build_plan(set_off.data(), nsets, pairs.data(), npairs, true, pl) == 0);
  CHECK(build_plan(set_off.data(), nsets, pairs.data(), npairs, false, sz) == 0);
  CHECK(sz.total_bytes == pl.total_bytes && sz.ntiles == pl.ntiles && sz.tiles.empty());
  CHECK((int64_t)pl.tiles.size() == pl.ntiles);
  CHECK(pl.sides.size() == (size_t)2 * npairs);
  // table, merged and partial regions: ordered, aligned, inside the workspace
  CHECK(pl.sides.size() * sizeof(Side) <= pl.tiles_off);
  CHECK(pl.tiles_off + pl.tiles.size() * sizeof(Tile) <= pl.tab_bytes);
  CHECK(pl.tab_bytes <= pl.merged_off && pl.merged_off % 256 == 0 && pl.part_off % 256 == 0);
  CHECK(pl.merged_off + (size_t)pl.merged_entries * 12 <= pl.part_off);
  CHECK(pl.part_off + (size_t)pl.part_entries * 12 <= pl.total_bytes);
  int64_t moff = 0, out = 0, part = 0;
  bool any_split = false;
  for (int p = 0; p < npairs; ++p) {
    const int n1 = sizes[pr[p].first], n2 = sizes[pr[p].second];
    const bool live = n1 > 0 && n2 > 0;
    for (int sd = 0; sd < 2; ++sd) {
      const Side& s = pl.sides[2 * p + sd];
      CHECK(s.moff == moff);
      CHECK(s.nb == (live ? (sd == 0 ? n1 : n2) : 0) && s.na == (live ? (sd == 0 ? n2 : n1) : 0));
      if (!live) {
        CHECK(s.nsplit == 0);
        continue;
      }
      CHECK(s.b_off == set_off[sd == 0 ? pr[p].first : pr[p].second]);
      CHECK(s.a_off == set_off[sd == 0 ? pr[p].second : pr[p].first]);
      CHECK(s.a_off + s.na <= set_off[nsets] && s.b_off + s.nb <= set_off[nsets]);
      CHECK(s.nsplit >= 1 && s.nsplit <= PMAXSPLIT && s.rps > 0 && s.rps % PSTEP == 0);
      CHECK((int64_t)s.nsplit * s.rps >= s.na && (int64_t)(s.nsplit - 1) * s.rps < s.na);
      // consecutive, non-overlapping regions
      CHECK(s.out_off == out);
      out += s.nb;
      if (s.nsplit > 1) {
        CHECK(s.part_off == part);
        part += (int64_t)s.nsplit * s.nb;
        any_split = true;
      }
    }
    moff += n1;
  }
  CHECK(out == pl.merged_entries && part == pl.part_entries && moff == pl.total_matches);
  CHECK(any_split == expect_split);
  // coverage: every (side, column block, range) exactly once; rows of a side
  // partitioned by its ranges; tiles sorted by length, longest first
  std::map<std::pair<int, std::pair<int, int>>, int> seen;
  int prev_rows = INT32_MAX;
  for (const Tile& t : pl.tiles) {
    CHECK(t.side >= 0 && t.side < 2 * npairs);
    const Side& s = pl.sides[t.side];
    CHECK(s.na > 0 && t.cb >= 0 && t.cb * PCOLS < s.nb && t.split >= 0 && t.split < s.nsplit);
    const int r0 = t.split * s.rps, r1 = s.na - r0 > s.rps ? r0 + s.rps : s.na;
    CHECK(r0 < r1 && r1 <= s.na);
    CHECK(r1 - r0 <= prev_rows);
    prev_rows = r1 - r0;
    const int times = ++seen[std::make_pair(t.side, std::make_pair(t.cb, t.split))];
    CHECK(times == 1);
  }
  int64_t want = 0;
  for (const Side& s : pl.sides)
    if (s.na > 0) want += (int64_t)((s.nb + PCOLS - 1) / PCOLS) * s.nsplit;
  CHECK((int64_t)seen.size() == want);
  // brute force on the small cases: each (side, column, row) hit exactly once
  if (set_off[nsets] <= 8192 && npairs <= 64) {
    for (int sd = 0; sd < 2 * npairs; ++sd) {
      const Side& s = pl.sides[sd];
      std::vector<unsigned char> hit((size_t)s.na * s.nb, 0);
      for (const Tile& t : pl.tiles) {
        if (t.side != sd) continue;
        const int r0 = t.split * s.rps, r1 = s.na - r0 > s.rps ? r0 + s.rps : s.na;
        for (int c = t.cb * PCOLS; c < t.cb * PCOLS + PCOLS && c < s.nb; ++c)
          for (int r = r0; r < r1; ++r) ++hit[(size_t)c * s.na + r];
      }
      for (unsigned char h : hit) CHECK(h == 1);
    }
  }
  std::printf("%-14s pairs %5d tiles %6lld split %d bytes %zu\n", name, npairs,
              (long long)pl.ntiles, (int)any_split, pl.total_bytes);
}

int main() {
  const std::vector<int> sizes = {1, 2, 31, 64, 129, 300, 1000, 2049};
  std::vector<std::pair<int, int>> all;
  for (int i = 0; i < 8; ++i) {
    all.push_back({i, (i + 1) % 8});
    all.push_back({(i + 3) % 8, i});
  }
  for (int j = 0; j < 5; ++j) all.push_back({5, j});  // one set against five others
  all.push_back({6, 6});
  all.push_back({7, 4});
  all.push_back({4, 7});
  check_case("ragged", sizes, all, true);
  check_case("single", sizes, {{7, 6}}, true);
  check_case("single-small", sizes, {{2, 3}}, false);
  check_case("empty-set", {0, 300, 0, 70}, {{0, 1}, {1, 0}, {1, 3}, {2, 2}, {3, 1}}, true);
  check_case("all-empty", {0, 0}, {{0, 1}}, false);
  {
    std::vector<int> one(2000, 1);
    std::vector<std::pair<int, int>> pr;
    for (int p = 0; p < 1000; ++p) pr.push_back({2 * p, 2 * p + 1});
    check_case("1000x1", one, pr, false);
  }
  {  // a long list of full-size pairs is not split
    std::vector<int> big(12, 8192);
    std::vector<std::pair<int, int>> pr;
    for (int s = 0; s < 2; ++s)
      for (int k = 1; k < 6; ++k) pr.push_back({6 * s, 6 * s + k});
    check_case("hpatches", big, pr, false);
  }
  // invalid tables
  g_case = "invalid";
  Plan pl;
  const int32_t off_ok[3] = {0, 4, 9}, off_dec[3] = {0, 5, 4}, off_neg[3] = {-1, 4, 9};
  const int32_t p_ok[2] = {0, 1}, p_hi[2] = {0, 2}, p_lo[2] = {-1, 1};
  CHECK(build_plan(off_ok, 2, p_ok, 1, true, pl) == 0);
  CHECK(build_plan(off_dec, 2, p_ok, 1, true, pl) == -1);
  CHECK(build_plan(off_neg, 2, p_ok, 1, true, pl) == -1);
  CHECK(build_plan(off_ok, 2, p_hi, 1, true, pl) == -1);
  CHECK(build_plan(off_ok, 2, p_lo, 1, true, pl) == -1);
  CHECK(build_plan(nullptr, 2, p_ok, 1, true, pl) == -1);
  {  // sum n1 past INT32_MAX: three pairs of a 2^30-row set
    const int32_t off_big[2] = {0, 1 << 30};
    const int32_t p_big[6] = {0, 0, 0, 0, 0, 0};
    CHECK(build_plan(off_big, 1, p_big, 1, false, pl) == 0);
    CHECK(build_plan(off_big, 1, p_big, 3, false, pl) == -1);
  }
  std::printf("match_plan ok\n");
  return 0;
}
