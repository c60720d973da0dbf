// Stand-alone check of posfeat_amd/csrc/guided_solve.h (the record and the
// admissibility predicate of posfeat_match_pairs_guided), built with
// -fsanitize=address,undefined and run directly by tests/test_guided_host.py
// on a file of cases the test writes: the inputs and the values its numpy
// restatement (tests/guided_ref.py) expects, compared bit for bit.
//
//   int32 nrec, nadm
//   nrec x { int32 model, side; double M[9]; float pt[2]; float expect[4] }
//   nadm x { int32 model; float ra[4]; float col[3]; float t2; int32 expect }
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../posfeat_amd/csrc/guided_solve.h"

#pragma pack(push, 1)
struct RecCase {
  int32_t model, side;
  double M[9];
  float pt[2];
  float expect[4];
};
struct AdmCase {
  int32_t model;
  float ra[4];
  float col[3];
  float t2;
  int32_t expect;
};
#pragma pack(pop)
static_assert(sizeof(RecCase) == 104 && sizeof(AdmCase) == 40, "file layout");

static bool same(float a, float b) {
  if (a != a || b != b) return a != a && b != b;
  return std::memcmp(&a, &b, 4) == 0;
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: guided_check CASES\n");
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f) {
    std::perror(argv[1]);
    return 2;
  }
  int32_t n[2];
  if (std::fread(n, 4, 2, f) != 2 || n[0] < 0 || n[1] < 0) return 2;
  std::vector<RecCase> rc((size_t)n[0]);
  std::vector<AdmCase> ac((size_t)n[1]);
  if (std::fread(rc.data(), sizeof(RecCase), rc.size(), f) != rc.size()) return 2;
  if (std::fread(ac.data(), sizeof(AdmCase), ac.size(), f) != ac.size()) return 2;
  std::fclose(f);
  long bad = 0;
  for (size_t i = 0; i < rc.size(); ++i) {
    const RecCase& c = rc[i];
    double M[9];
    std::memcpy(M, c.M, sizeof M);
    float r[4];
    pfguided::record(c.model, c.side, M, c.pt[0], c.pt[1], r);
    for (int k = 0; k < 4; ++k)
      if (!same(r[k], c.expect[k])) {
        if (bad++ < 10)
          std::fprintf(stderr, "record %zu (model %d side %d) component %d: %.9g, expected %.9g\n",
                       i, c.model, c.side, k, r[k], c.expect[k]);
      }
  }
  for (size_t i = 0; i < ac.size(); ++i) {
    const AdmCase c = ac[i];
    const bool got =
        c.model == pfguided::FUNDAMENTAL
            ? pfguided::admissible<pfguided::FUNDAMENTAL>(c.ra[0], c.ra[1], c.ra[2], c.ra[3],
                                                          c.col[0], c.col[1], c.col[2], c.t2)
            : pfguided::admissible<pfguided::HOMOGRAPHY>(c.ra[0], c.ra[1], c.ra[2], c.ra[3],
                                                         c.col[0], c.col[1], c.col[2], c.t2);
    if ((int)got != c.expect) {
      if (bad++ < 10)
        std::fprintf(stderr, "admissible %zu (model %d): %d, expected %d\n", i, c.model, (int)got,
                     c.expect);
    }
  }
  if (bad) {
    std::fprintf(stderr, "%ld mismatches\n", bad);
    return 1;
  }
  std::printf("guided ok: %zu records, %zu predicates\n", rc.size(), ac.size());
  return 0;
}
