// Stand-alone check of posfeat_amd/csrc/essential_solve.h and of the slot key
// and plan ransac_plan.h gained for posfeat_ransac_essential, built with
// -fsanitize=address,undefined and run directly by tests/test_essential_host.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>

#include "../../posfeat_amd/csrc/essential_solve.h"
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

static double urand(uint64_t& s) {
  s = mix(s);
  return (double)(s >> 11) / 9007199254740992.0;
}

// matches of a random scene in normalised camera coordinates under a planted
// motion: kind 0 general (rotation about y), 1 pure forward, 2 pure sideways, 3
// a tilted plane under the general motion.  P = [R | t / |t|].
static void scene(uint64_t& s, int kind, int n, double (*m)[4], double (&P)[12]) {
  const double th = (kind == 0 || kind == 3) ? 0.2 * (urand(s) - 0.5) + 0.02 : 0.0;
  double t[3] = {kind == 1 ? 0.0 : 0.5 + urand(s), kind == 1 ? 0.0 : urand(s) - 0.5,
                 kind == 2 ? 0.0 : 0.5 + urand(s)};
  const double tn = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
  const double R[9] = {std::cos(th), 0.0, std::sin(th), 0.0, 1.0, 0.0, -std::sin(th), 0.0, std::cos(th)};
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) P[4 * r + c] = R[3 * r + c];
    P[4 * r + 3] = t[r] / tn;
  }
  for (int i = 0; i < n; ++i) {
    const double X = 4.0 * (urand(s) - 0.5), Y = 3.0 * (urand(s) - 0.5);
    const double Z = kind == 3 ? 6.0 + 0.5 * X - 0.3 * Y : 4.0 + 5.0 * urand(s);
    const double X2 = R[0] * X + R[2] * Z + t[0], Y2 = Y + t[1], Z2 = R[6] * X + R[8] * Z + t[2];
    m[i][0] = X / Z, m[i][1] = Y / Z, m[i][2] = X2 / Z2, m[i][3] = Y2 / Z2;
  }
}

static void essential_of(const double (&P)[12], double (&E)[9]) {  // [t]x R
  const double t[3] = {P[3], P[7], P[11]};
  for (int c = 0; c < 3; ++c) {
    E[c] = t[1] * P[8 + c] - t[2] * P[4 + c];
    E[3 + c] = t[2] * P[c] - t[0] * P[8 + c];
    E[6 + c] = t[0] * P[4 + c] - t[1] * P[c];
  }
}

static void check_keys_and_plan() {
  g_case = "slot key";
  CHECK(slot_key_root4(0, 0, 0) > 0ull);
  CHECK(slot_key_root4(5, 9, 2) > slot_key_root4(4, 0, 0));
  CHECK(slot_key_root4(5, 3, 9) > slot_key_root4(5, 4, 0));
  CHECK(slot_key_root4(5, 3, 8) > slot_key_root4(5, 3, 9));
  for (int it : {0, 1, 255, 256, RMAXITERS - 1})
    for (int r = 0; r < 10; ++r) {
      const unsigned long long k = slot_key_root4(INT32_MAX - 1, it, r);
      CHECK(slot_key_iter4(k) == it && slot_key_rootidx4(k) == r && (k >> 32) == (unsigned)INT32_MAX);
    }
  g_case = "plan";
  const int32_t set_off[] = {0, 300, 300, 1300, 3349}, pairs[] = {0, 2, 2, 3, 1, 0, 3, 3};
  EssPlan pl;
  CHECK(build_plan_essential(set_off, 4, pairs, 4, 300, pl) == 0);
  CHECK(pl.base.nblk == 2 && pl.base.total_matches == 300 + 1000 + 0 + 2049);
  CHECK(pl.base.tab[1].pad[0] == 2 && pl.base.tab[1].pad[1] == 3 && pl.base.tab[1].moff == 300);
  CHECK(pl.cnt_off >= pl.base.pts_off + 32u * 3349 && pl.rec_off >= pl.cnt_off + 4u * 8);
  CHECK(pl.slot_off >= pl.rec_off + 80ull * EBLOCK_RECS * 8);
  CHECK(pl.total_bytes >= pl.slot_off + 8u * 8 * ESUB && pl.total_bytes % 256 == 0);
  CHECK(build_plan_essential(set_off, 4, pairs, 4, 0, pl) == -1);
  CHECK(build_plan_essential(set_off, 4, pairs, 4, RMAXITERS + 1, pl) == -1);
  const int32_t bad[] = {0, 4};
  CHECK(build_plan_essential(set_off, 4, bad, 1, 256, pl) == -1);
}

static void check_roots() {
  g_case = "roots10";
  // (z - 1)(z - 2)(z + 3)(z^2 + 1)(z^2 + 4)(z^2 - 2 z + 5)(z - 0.5): four real roots
  double co[11] = {1.0}, zr[10];
  int deg = 0;
  auto times = [&](double c0, double c1, double c2) {  // by c0 + c1 z + c2 z^2
    double o[11] = {};
    for (int i = 0; i <= deg; ++i) {
      o[i] += co[i] * c0;
      if (i + 1 < 11) o[i + 1] += co[i] * c1;
      if (i + 2 < 11) o[i + 2] += co[i] * c2;
    }
    deg += c2 != 0.0 ? 2 : 1;
    for (int i = 0; i < 11; ++i) co[i] = o[i];
  };
  times(-1, 1, 0), times(-2, 1, 0), times(3, 1, 0), times(1, 0, 1), times(4, 0, 1), times(5, -2, 1);
  times(-0.5, 1, 0);
  CHECK(deg == 10);
  CHECK(pfess::roots10(co, zr) == 4);
  CHECK(std::fabs(zr[0] + 3) < 1e-12 && std::fabs(zr[1] - 0.5) < 1e-12 && std::fabs(zr[2] - 1) < 1e-12 &&
        std::fabs(zr[3] - 2) < 1e-12 && zr[4] > 1e300);
  double low[11] = {1.0, 2.0, 3.0};  // the leading coefficient is zero
  CHECK(pfess::roots10(low, zr) == 0);
  double bad[11] = {1.0, NAN, 0, 0, 0, 0, 0, 0, 0, 0, 1.0};
  CHECK(pfess::roots10(bad, zr) == 0);
  double none[11] = {1.0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1.0};  // z^10 + 1
  CHECK(pfess::roots10(none, zr) == 0);
}

static double dist_up_to_sign(const double* a, const double* b) {
  double dp = 0.0, dm = 0.0;
  for (int k = 0; k < 9; ++k) dp = std::fmax(dp, std::fabs(a[k] - b[k])), dm = std::fmax(dm, std::fabs(a[k] + b[k]));
  return std::fmin(dp, dm);
}

static void check_solver() {
  g_case = "solve5";
  uint64_t s = 12345;
  long total = 0, rejected = 0, found = 0;
  for (int trial = 0; trial < 400; ++trial) {
    double m[5][4], P[12], E[pfess::MAXCAND][9], Et[9];
    scene(s, trial % 4, 5, m, P);
    essential_of(P, Et);
    CHECK(pffund::unit_sign(Et));
    if (trial % 50 == 49)
      for (int k = 0; k < 4; ++k) m[4][k] = m[1][k];  // a repeated match: rejected
    const int nc = pfess::solve5(m, E);
    CHECK(nc >= 0 && nc <= pfess::MAXCAND);
    if (trial % 50 == 49) CHECK(nc == 0);
    rejected += nc == 0;
    double best = 1e9;
    for (int r = 0; r < nc; ++r) {
      ++total;
      double ss = 0.0;
      for (int k = 0; k < 9; ++k) ss += E[r][k] * E[r][k];
      CHECK(std::fabs(std::sqrt(ss) - 1.0) <= 1e-14);
      best = std::fmin(best, dist_up_to_sign(E[r], Et));
      for (int i = 0; i < 5; ++i) {
        double row[9], e = 0.0;
        pffund::epi_row(m[i][0], m[i][1], m[i][2], m[i][3], row);
        for (int k = 0; k < 9; ++k) e += row[k] * E[r][k];
        CHECK(std::fabs(e) <= 1e-7);
      }
    }
    if (trial % 50 != 49 && best <= 1e-5) ++found;
  }
  CHECK(total >= 800 && rejected >= 8 && found >= 380);
  std::printf("solve5: %ld candidates, %ld samples rejected, planted E found in %ld\n", total,
              rejected, found);
  double z[5][4] = {}, E[pfess::MAXCAND][9];
  CHECK(pfess::solve5(z, E) == 0);
  z[3][1] = NAN;
  CHECK(pfess::solve5(z, E) == 0);
}

static void check_refit_and_pose() {
  g_case = "refit";
  uint64_t s = 777;
  int reached[4] = {0, 0, 0, 0};
  for (int trial = 0; trial < 80; ++trial) {
    double m[40][4], P[12], nmat[9][9] = {}, E[9], Et[9];
    scene(s, trial % 4, 40, m, P);
    if (trial % 2)  // the mirrored scene: another valid motion, compared by its counts only
      for (int i = 0; i < 40; ++i) {
        m[i][0] = -m[i][0], m[i][2] = -m[i][2];
      }
    essential_of(P, Et);
    for (int i = 0; i < 40; ++i) {
      double row[9];
      pffund::epi_row(m[i][0], m[i][1], m[i][2], m[i][3], row);
      for (int r = 0; r < 9; ++r)
        for (int c = r; c < 9; ++c) nmat[r][c] += row[r] * row[c];
    }
    CHECK(pfess::refit_from_normal(nmat, E));
    double U[9], V[9];
    pfess::frames(E, U, V);
    double Pd[4][12];
    pfess::decompositions(E, Pd);
    int best = 0, nf = -1;
    for (int k = 0; k < 4; ++k) {
      // R orthonormal, |t| = 1
      for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) {
          double d = 0.0;
          for (int j = 0; j < 3; ++j) d += Pd[k][4 * r + j] * Pd[k][4 * c + j];
          CHECK(std::fabs(d - (r == c ? 1.0 : 0.0)) <= 1e-12);
        }
      int f = 0;
      for (int i = 0; i < 40; ++i) f += pfess::in_front(Pd[k], m[i][0], m[i][1], m[i][2], m[i][3]);
      if (f > nf) best = k, nf = f;
    }
    ++reached[best];
    if (trial % 2 == 0) {
      CHECK(nf == 40);
      for (int i = 0; i < 40; ++i)
        CHECK(pffund::sampson_inlier(E, m[i][0], m[i][1], m[i][2], m[i][3], 1e-16));
      for (int k = 0; k < 12; ++k) CHECK(std::fabs(Pd[best][k] - P[k]) <= 1e-6);
    }
  }
  std::printf("decompositions chosen: %d %d %d %d\n", reached[0], reached[1], reached[2], reached[3]);
  double zero[9] = {}, Pd[4][12];
  pfess::decompositions(zero, Pd);  // no fault on a zero matrix; the entries are NaN
  CHECK(Pd[0][0] != Pd[0][0]);
  const double cam1[8] = {400, 420, 0, 0, 0, 0, 0, 0}, cam2[8] = {900, 900, 0, 0, 0, 0, 0, 0};
  const double t = (3.0 / 410.0 + 3.0 / 900.0) / 2.0;
  CHECK(std::fabs(pfess::thr_norm2(cam1, cam2, 3.0) - t * t) <= 1e-18);
}

int main() {
  check_keys_and_plan();
  check_roots();
  check_solver();
  check_refit_and_pose();
  std::printf("essential_solve ok\n");
  return 0;
}
