// Stand-alone check of posfeat_amd/csrc/ransac_plan.h (the sampler, the table
// checks and the workspace layout of posfeat_ransac_homography), built with
// -fsanitize=address,undefined and run directly by tests/test_ransac_host.py.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <utility>
#include <vector>

#include "../../posfeat_amd/csrc/ransac_plan.h"

using namespace pfransac_plan;

#define CHECK(c)                                                                            \
  do {                                                                                      \
    if (!(c)) {                                                                             \
      std::fprintf(stderr, "%s:%d: %s failed (case %s)\n", __FILE__, __LINE__, #c, g_case); \
      std::exit(1);                                                                         \
    }                                                                                       \
  } while (0)

static const char* g_case = "";

// the definition, written the long way round: a list of the earlier draws,
// sorted before each use
static void sample_slow(uint64_t seed, int pair, int it, int n, int32_t out[4]) {
  const uint64_t base = mix(mix(seed ^ mix((uint64_t)pair)) ^ (uint64_t)it);
  std::set<int32_t> prev;
  for (int k = 0; k < 4; ++k) {
    const uint64_t r = mix(base ^ (uint64_t)k);
    int32_t j = (int32_t)(((r >> 32) * (uint64_t)(n - k)) >> 32);
    for (int32_t q : prev)
      if (j >= q) ++j;
    out[k] = j;
    prev.insert(j);
  }
}

static void check_sampler() {
  g_case = "sampler";
  const int sizes[] = {4, 5, 63, 64, 65, 8192, 60000, INT32_MAX};
  const uint64_t seeds[] = {0ull, 1ull, 0x123456789abcdef0ull, ~0ull};
  for (int n : sizes)
    for (uint64_t seed : seeds)
      for (int pair : {0, 99, INT32_MAX})
        for (int it = 0; it < 256; ++it) {
          int32_t a[4], b[4];
          sample4(seed, pair, it, n, a);
          sample_slow(seed, pair, it, n, b);
          for (int k = 0; k < 4; ++k) {
            CHECK(a[k] == b[k] && a[k] >= 0 && a[k] < n);
            for (int l = 0; l < k; ++l) CHECK(a[k] != a[l]);
          }
        }
  // every index of a 64-match pair is drawn within 4096 iterations
  std::vector<int> hit(64, 0);
  for (int it = 0; it < 4096; ++it) {
    int32_t a[4];
    sample4(7, 3, it, 64, a);
    for (int k = 0; k < 4; ++k) ++hit[a[k]];
  }
  for (int h : hit) CHECK(h > 0);
  CHECK(mix(0) == 0xE220A8397B1DCDAFull);  // splitmix64's first output for seed 0
}

static void check_case(const char* name, const std::vector<int>& sizes,
                       const std::vector<std::pair<int, int>>& pr, int iters) {
  g_case = name;
  std::vector<int32_t> set_off(sizes.size() + 1, 0), pairs;
  for (size_t i = 0; i < sizes.size(); ++i) set_off[i + 1] = set_off[i] + sizes[i];
  for (auto& p : pr) {
    pairs.push_back(p.first);
    pairs.push_back(p.second);
  }
  const int nsets = (int)sizes.size(), npairs = (int)pr.size();
  Plan pl;
  CHECK(build_plan(set_off.data(), nsets, pairs.data(), npairs, iters, pl) == 0);
  CHECK(pl.tab.size() == (size_t)npairs);
  CHECK(pl.nblk >= 1 && pl.nblk <= RMAXITERS / RBLOCK);
  CHECK((int64_t)pl.nblk * RBLOCK >= iters && (int64_t)(pl.nblk - 1) * RBLOCK < iters);
  int64_t moff = 0;
  for (int p = 0; p < npairs; ++p) {
    const Pair& q = pl.tab[p];
    CHECK(q.moff == moff && q.n1 == sizes[pr[p].first] && q.n2 == sizes[pr[p].second]);
    CHECK(q.a_off == set_off[pr[p].first] && q.b_off == set_off[pr[p].second]);
    CHECK(q.a_off + q.n1 <= set_off[nsets] && q.b_off + q.n2 <= set_off[nsets]);
    moff += q.n1;
  }
  CHECK(moff == pl.total_matches);
  // regions: ordered, aligned, disjoint, inside the workspace
  CHECK(pl.pts_off % 256 == 0 && pl.norm_off % 256 == 0 && pl.slot_off % 256 == 0);
  CHECK((size_t)npairs * sizeof(Pair) <= pl.pts_off);
  CHECK(pl.pts_off + (size_t)moff * 16 <= pl.norm_off);
  CHECK(pl.norm_off + (size_t)npairs * 64 <= pl.slot_off);
  CHECK(pl.slot_off + (size_t)npairs * pl.nblk * 8 <= pl.total_bytes);
  std::printf("%-12s pairs %5d iters %6d blocks %3d bytes %zu\n", name, npairs, iters, pl.nblk,
              pl.total_bytes);
}

int main() {
  check_sampler();
  const std::vector<int> sizes = {0, 3, 4, 5, 63, 64, 65, 300, 2049, 8192};
  std::vector<std::pair<int, int>> all;
  for (int i = 0; i < 10; ++i) {
    all.push_back({i, (i + 1) % 10});
    all.push_back({(i + 3) % 10, i});
  }
  all.push_back({7, 7});
  for (int iters : {1, 100, 255, 256, 257, 1024, 65536}) check_case("ragged", sizes, all, iters);
  check_case("single", sizes, {{8, 7}}, 256);
  check_case("all-empty", {0, 0}, {{0, 1}}, 256);
  {
    std::vector<int> big(120, 8192);
    std::vector<std::pair<int, int>> pr;
    for (int s = 0; s < 20; ++s)
      for (int k = 1; k < 6; ++k) pr.push_back({6 * s, 6 * s + k});
    check_case("hpatches", big, pr, 1024);
  }
  // invalid tables and iteration counts
  g_case = "invalid";
  Plan pl;
  const int32_t off_ok[3] = {0, 4, 9}, off_dec[3] = {0, 5, 4}, off_neg[3] = {-1, 4, 9};
  const int32_t p_ok[2] = {0, 1}, p_hi[2] = {0, 2}, p_lo[2] = {-1, 1};
  CHECK(build_plan(off_ok, 2, p_ok, 1, 256, pl) == 0);
  CHECK(build_plan(off_dec, 2, p_ok, 1, 256, pl) == -1);
  CHECK(build_plan(off_neg, 2, p_ok, 1, 256, pl) == -1);
  CHECK(build_plan(off_ok, 2, p_hi, 1, 256, pl) == -1);
  CHECK(build_plan(off_ok, 2, p_lo, 1, 256, pl) == -1);
  CHECK(build_plan(nullptr, 2, p_ok, 1, 256, pl) == -1);
  CHECK(build_plan(off_ok, 2, nullptr, 1, 256, pl) == -1);
  CHECK(build_plan(off_ok, 2, p_ok, 1, 0, pl) == -1);
  CHECK(build_plan(off_ok, 2, p_ok, 1, -5, pl) == -1);
  CHECK(build_plan(off_ok, 2, p_ok, 1, 65537, pl) == -1);
  CHECK(build_plan(off_ok, 2, p_ok, 1, 65536, pl) == 0);
  {  // sum n1 past INT32_MAX: three pairs of a 2^30-row set
    const int32_t off_big[2] = {0, 1 << 30};
    const int32_t p_big[6] = {0, 0, 0, 0, 0, 0};
    CHECK(build_plan(off_big, 1, p_big, 1, 256, pl) == 0);
    CHECK(build_plan(off_big, 1, p_big, 3, 256, pl) == -1);
  }
  std::printf("ransac_plan ok\n");
  return 0;
}
