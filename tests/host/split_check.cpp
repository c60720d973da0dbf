// Stand-alone check of posfeat_amd/csrc/split_plan.h (the closed form of the
// output numbering under a capacity against a walk in output order, the
// parameter check and the workspace layout), built with
// -fsanitize=address,undefined and run directly by tests/test_split_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../posfeat_amd/csrc/split_plan.h"

using namespace pfsplit;

#define CHECK(c)                                                                            \
  do {                                                                                      \
    if (!(c)) {                                                                             \
      std::fprintf(stderr, "%s:%d: %s failed (case %s)\n", __FILE__, __LINE__, #c, g_case); \
      std::exit(1);                                                                         \
    }                                                                                       \
  } while (0)

static const char* g_case = "";

static uint64_t g_state = 77;
static int below(int n) {
  g_state = pfransac_plan::mix(g_state);
  return (int)((g_state >> 33) % (uint64_t)n);
}

// the rule as the header states it: in output order a child is created iff its
// number plus the parents still to come stays below tmax_out
static void walk(const std::vector<int>& c, long long tmax_out, std::vector<long long>& id,
                 std::vector<int>& made) {
  const long long T = (long long)c.size();
  long long next = 0;
  id.assign(c.size(), 0), made.assign(c.size(), 0);
  for (long long t = 0; t < T; ++t) {
    id[t] = next++;
    for (int g = 1; g <= c[t]; ++g)
      if (next + (T - 1 - t) < tmax_out) ++next, ++made[t];
  }
}

static void check_numbering() {
  g_case = "numbering";
  for (int trial = 0; trial < 4000; ++trial) {
    const int T = below(40);
    std::vector<int> c(T);
    long long all = T;
    for (int t = 0; t < T; ++t) c[t] = below(3) == 0 ? below(MAX_ROUNDS + 1) : 0, all += c[t];
    for (long long tmax_out = T; tmax_out <= all + 2; ++tmax_out) {
      std::vector<long long> id;
      std::vector<int> made;
      walk(c, tmax_out, id, made);
      long long u = 0, last = -1, total = 0;
      for (int t = 0; t < T; ++t) {
        const long long pid = parent_id(u, t, T, tmax_out);
        const int cr = children_created(u, c[t], t, T, tmax_out);
        CHECK(pid == id[t] && cr == made[t]);
        CHECK(pid == last + 1 && cr >= 0 && cr <= c[t]);  // dense, ascending
        last = pid + cr, total += 1 + cr;
        u += 1 + c[t];
      }
      CHECK(total == (all < tmax_out ? all : tmax_out) && last + 1 == total);
    }
  }
}

static void check_plan() {
  g_case = "params";
  CHECK(params_ok(64, 4.0, 1.5, 2) && params_ok(8, 1e-3, 0.0, 1) && params_ok(1024, 1e9, 89.9, 4));
  CHECK(!params_ok(7, 4.0, 1.5, 2) && !params_ok(1025, 4.0, 1.5, 2));
  CHECK(!params_ok(64, 0.0, 1.5, 2) && !params_ok(64, (double)INFINITY, 1.5, 2) &&
        !params_ok(64, (double)NAN, 1.5, 2));
  CHECK(!params_ok(64, 4.0, -0.1, 2) && !params_ok(64, 4.0, 90.0, 2) &&
        !params_ok(64, 4.0, (double)NAN, 2));
  CHECK(!params_ok(64, 4.0, 1.5, 0) && !params_ok(64, 4.0, 1.5, 5));
  g_case = "layout";
  const int32_t so[4] = {0, 300, 300, 2400};
  Layout L;
  CHECK(layout(so, 3, 1000, 2000, 1000, L) == 0 && L.n == 2400 && L.nblk == 1);
  const size_t at[] = {L.set_off, L.setid,    L.und,    L.list, L.mark, L.nleft, L.nchild,
                       L.ids,     L.ncreated, L.cpoint, L.cerr, L.cinfo, L.bsum, L.total};
  const size_t need[] = {16,   9600, 38400, 8000,  2000,  4000, 4000,
                         4000, 4000, 96000, 32000, 64000, 8};
  for (int i = 0; i < 13; ++i) CHECK(at[i] % 256 == 0 && at[i + 1] >= at[i] + need[i]);
  CHECK(layout(so, 3, 2049, 5000, 2500, L) == 0 && L.nblk == 2);
  CHECK(layout(so, 3, 0, 0, 0, L) == 0 && L.nblk == 1 && L.total > 0);
  CHECK(layout(so, 3, 1000, 2000, 999, L) != 0);  // tmax_out below tmax
  CHECK(layout(so, 3, -1, 2000, 1000, L) != 0 && layout(so, 3, 1000, -1, 1000, L) != 0);
  CHECK(layout(so, 3, 2147483647LL, 2000, 2147483647LL, L) != 0);
  CHECK(layout(so, 3, 1000, 2147483648LL, 1000, L) != 0);
  CHECK(layout(so, 3, 1000, 2000, 2147483647LL, L) != 0);
  CHECK(layout(nullptr, 3, 1000, 2000, 1000, L) != 0 && layout(so, -1, 1000, 2000, 1000, L) != 0);
  const int32_t dec[4] = {0, 300, 299, 2400};
  CHECK(layout(dec, 3, 1000, 2000, 1000, L) != 0);
}

int main() {
  check_numbering();
  check_plan();
  std::printf("split_plan ok\n");
  return 0;
}
