// Host check of posfeat_amd/csrc/conv_plan.h (plain C++, built with
// -fsanitize=address,undefined by tests/test_conv_plan_host.py):
//  1. tests/golden/conv_plans.txt -- the plans, launched kernels and grids
//     recorded at the commit before the planner became a table, for every
//     shape x mode x allow_split x forced tile of its sweep -- recomputed and
//     required equal, field by field;
//  2. shapes whose M or grid sits just below / above 2^31: an error or the
//     exact 64-bit result, never wrap-around.
// usage: conv_plan_check [fixture]; prints "conv_plan ok".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <map>
#include <utility>
#include <sstream>
#include <string>
#include <vector>

#include "../../posfeat_amd/csrc/conv_plan.h"

namespace {

long long g_checked = 0;
int g_fail = 0;

void fail(const std::string& what) {
  if (++g_fail <= 20) fprintf(stderr, "MISMATCH %s\n", what.c_str());
}

// one recorded result: the R line's fields and the shape's T entry for it
struct Result {
  int kern, tile, bm, bn, ppi, ksplit;
  std::string kernel;
  int block, arith;
};
struct Grid {
  long long tiles_m, grid;
};

std::string describe(const Plan& p) {
  std::ostringstream o;
  o << p.kern << ' ' << p.tile << ' ' << p.bm << ' ' << p.bn << ' ' << p.ppi << ' ' << p.tiles_m
    << ' ' << p.ksplit << ' ' << variant_name(p.variant) << ' ' << (long long)p.nwg * p.ksplit
    << ' ' << p.threads << ' ' << p.arith;
  return o.str();
}

bool same(const Plan& p, const Result& r, const Grid& g) {
  return p.kern == r.kern && p.tile == r.tile && p.bm == r.bm && p.bn == r.bn && p.ppi == r.ppi &&
         p.tiles_m == g.tiles_m && p.ksplit == r.ksplit && r.kernel == variant_name(p.variant) &&
         (long long)p.nwg * p.ksplit == g.grid && p.threads == r.block && p.arith == r.arith;
}

std::vector<std::string> split(const std::string& s, char c) {
  std::vector<std::string> out;
  std::istringstream ss(s);
  for (std::string t; std::getline(ss, t, c);) out.push_back(t);
  return out;
}

struct Fixture {
  std::map<int, ConvShape> shapes;
  std::map<int, ConvMode> modes;
  std::map<int, Result> results;
  std::map<int, std::map<int, Grid>> grids;  // [shape][R]
  std::vector<long long> gm;
  std::vector<int> gn;
  // the open B block: its shapes and C lines (who, plan per forced + 1)
  std::vector<int> bshapes;
  std::vector<std::pair<std::string, std::vector<int>>> blines;
  std::map<int, int> covered;  // shape -> blocks it was in
  long long ncase = 0, ncand = 0, ngemm = 0;

  // every mode x allow_split x forced tile of every shape of the block
  bool flush() {
    if (bshapes.empty()) return true;
    std::map<std::pair<int, int>, const std::vector<int>*> named;
    const std::vector<int>* rest = nullptr;
    for (const auto& bl : blines) {
      if (bl.first == "*") {
        if (rest) return false;
        rest = &bl.second;
        continue;
      }
      for (const std::string& w : split(bl.first, ',')) {
        int m = -1, sp = -1;
        const int n = sscanf(w.c_str(), "%d.%d", &m, &sp);
        if (n < 1 || !modes.count(m) || (n == 2 && sp != 0 && sp != 1)) return false;
        for (int k = 0; k < 2; ++k)
          if (n == 1 || sp == k)
            if (!named.emplace(std::make_pair(m, k), &bl.second).second) return false;
      }
    }
    if (!rest) return false;
    for (int sid : bshapes) {
      ++covered[sid];
      for (const auto& mo : modes)
        for (int sp = 0; sp < 2; ++sp) {
          const auto it = named.find({mo.first, sp});
          const std::vector<int>& want = it != named.end() ? *it->second : *rest;
          for (int forced = -1; forced <= 35; ++forced) {
            const Plan p = conv_plan(shapes[sid], mo.second, sp != 0, forced);
            const int rid = want[forced + 1];
            ++g_checked;
            if (!grids[sid].count(rid) || !same(p, results[rid], grids[sid][rid]))
              fail("shape " + std::to_string(sid) + " mode " + std::to_string(mo.first) + " split " +
                   std::to_string(sp) + " forced " + std::to_string(forced) + ": want R " +
                   std::to_string(rid) + ", got " + describe(p));
          }
          ++ncase;
        }
    }
    bshapes.clear();
    blines.clear();
    return true;
  }
};

int check_fixture(const char* path) {
  std::ifstream in(path);
  if (!in) {
    fprintf(stderr, "cannot open %s\n", path);
    return 1;
  }
  Fixture fx;
  std::string line;
  const auto bad = [&] { return fprintf(stderr, "bad line: %s\n", line.c_str()), 1; };
  while (std::getline(in, line)) {
    if (line.empty() || line[0] == '#') continue;
    std::istringstream ss(line.substr(0, line.find('#')));
    std::string kind;
    ss >> kind;
    if (kind != "C" && !fx.flush()) return bad();
    if (kind == "S") {
      int id, wb, xb, x2, am;
      ConvShape s{};
      ss >> id >> s.M >> s.hw >> s.OH >> s.OW >> s.Cin >> s.xcs >> s.Cout >> s.KH >> s.KW >>
          s.stride >> s.pad >> s.Kpad >> wb >> xb >> x2 >> am;
      s.has_wb = wb, s.has_xb = xb, s.has_x2 = x2, s.has_amean = am;
      if (!ss) return bad();
      fx.shapes[id] = s;
    } else if (kind == "M") {
      int id, b[18];
      ss >> id;
      for (int& v : b) ss >> v;
      if (!ss) return bad();
      ConvMode m;
      m.precision = b[0], m.halo_fp32 = b[1], m.dense32 = b[2], m.stem32 = b[3];
      m.bf6_halo = b[4], m.bf6d = b[5], m.bf6x = b[6], m.bf6_stem = b[7], m.maxsplit = b[8];
      m.kmax = b[9], m.tile = b[10], m.bm192 = b[11], m.rb4n64 = b[12], m.gemm_b256 = b[13];
      m.rb4 = b[14], m.n256 = b[15], m.train_wino_bf6x = b[16], m.wsb = b[17];
      fx.modes[id] = m;
    } else if (kind == "GM" || kind == "GN") {
      for (long long v; ss >> v;) kind == "GM" ? fx.gm.push_back(v) : fx.gn.push_back((int)v);
    } else if (kind == "R") {
      int id;
      Result r;
      ss >> id >> r.kern >> r.tile >> r.bm >> r.bn >> r.ppi >> r.ksplit;
      const size_t k0 = line.find('('), k1 = line.rfind(')');
      if (!ss || k0 == std::string::npos || k1 < k0) return bad();
      r.kernel = line.substr(k0, k1 - k0 + 1);
      std::istringstream tail(line.substr(k1 + 1));
      tail >> r.block >> r.arith;
      if (!tail) return bad();
      fx.results[id] = r;
    } else if (kind == "T") {
      std::string sids;
      ss >> sids;
      for (const std::string& t : split(sids, ','))
        if (!fx.shapes.count(atoi(t.c_str()))) return bad();
      for (std::string tok; ss >> tok;) {
        Grid g;
        int used = 0;
        if (sscanf(tok.c_str(), "%lld:%lld=%n", &g.tiles_m, &g.grid, &used) != 2 ||
            !used) {
          if (sscanf(tok.c_str(), "%lld=%n", &g.tiles_m, &used) != 1 || !used) return bad();
          g.grid = g.tiles_m;  // one number: both
        }
        for (const std::string& r : split(tok.substr(used), ',')) {
          if (!fx.results.count(atoi(r.c_str()))) return bad();
          for (const std::string& t : split(sids, ','))
            fx.grids[atoi(t.c_str())][atoi(r.c_str())] = g;
        }
      }
    } else if (kind == "B") {
      std::string list;
      ss >> list;
      for (const std::string& t : split(list, ',')) {
        if (!fx.shapes.count(atoi(t.c_str()))) return bad();
        fx.bshapes.push_back(atoi(t.c_str()));
      }
      if (fx.bshapes.empty()) return bad();
    } else if (kind == "C") {
      std::string who;
      int r0;
      ss >> who >> r0;
      if (!ss || fx.bshapes.empty() || !fx.results.count(r0)) return bad();
      std::vector<int> want(37, r0);  // [forced + 1]
      for (std::string tok; ss >> tok;) {
        int f, r;
        if (tok[0] == '=') {  // what the forced tiles not listed gave
          r = atoi(tok.c_str() + 1);
          if (!fx.results.count(r)) return bad();
          std::fill(want.begin() + 1, want.end(), r);
          continue;
        }
        if (sscanf(tok.c_str(), "%d:%d", &f, &r) != 2 || f < 0 || f > 35 || !fx.results.count(r))
          return bad();
        want[f + 1] = r;
      }
      fx.blines.emplace_back(who, want);
    } else if (kind == "K") {
      int mid;
      std::string list, colon, sids;
      ss >> mid >> list >> colon >> sids;
      if (!ss || colon != ":" || !fx.modes.count(mid)) return bad();
      for (const std::string& t : split(sids, ',')) {
        const int sid = atoi(t.c_str());
        if (!fx.shapes.count(sid)) return bad();
        std::string got;
        for (const TileRow& r : kTileTable)
          if (!r.not_candidate && plan_for_tile(fx.shapes[sid], fx.modes[mid], r.id).kern >= 0)
            got += (got.empty() ? "" : ",") + std::to_string(r.id);
        if (got.empty()) got = "-";
        ++g_checked;
        if (got != list) fail(line.substr(0, 60) + " shape " + t + ": got " + got);
        ++fx.ncand;
      }
    } else if (kind == "G") {
      std::string mids, bar;
      int bb, K, nb;
      ss >> mids >> bb >> K >> nb >> bar;
      if (!ss || bar != "|" || fx.gm.empty() || fx.gn.empty()) return bad();
      std::vector<std::pair<int, int>> cells;
      for (std::string tok; ss >> tok;) {
        int want, wsf;
        if (sscanf(tok.c_str(), "%d/%d", &want, &wsf) != 2) return bad();
        cells.emplace_back(want, wsf);
      }
      if (cells.size() != fx.gm.size() * fx.gn.size()) return bad();
      for (const std::string& t : split(mids, ',')) {
        if (!fx.modes.count(atoi(t.c_str()))) return bad();
        ConvMode m = fx.modes[atoi(t.c_str())];
        const bool ws = gemm_batched_ws_first(K, bb != 0, m);
        if (m.train_wino_bf6x && bb) m.halo_fp32 = false;  // as pf_gemm_batched
        for (size_t i = 0; i < cells.size(); ++i) {
          const int tile = gemm_batched_tile(fx.gm[i / fx.gn.size()], fx.gn[i % fx.gn.size()], nb,
                                             bb != 0, m);
          ++g_checked;
          if (tile != cells[i].first || ws != (cells[i].second != 0))
            fail(line.substr(0, 60) + " mode " + t + " cell " + std::to_string(i) + ": got " +
                 std::to_string(tile) + "/" + std::to_string(ws));
          ++fx.ngemm;
        }
      }
    } else {
      return bad();
    }
  }
  if (!fx.flush()) return fprintf(stderr, "bad last block\n"), 1;
  for (const auto& s : fx.shapes)
    if (fx.covered[s.first] != 1)
      return fprintf(stderr, "shape %d is in %d blocks\n", s.first, fx.covered[s.first]), 1;
  printf("fixture: %zu shapes x %zu modes x 2 x 37 forced tiles, %lld candidate lists, %lld "
         "batched GEMMs\n", fx.shapes.size(), fx.modes.size(), fx.ncand, fx.ngemm);
  // the sweep the fixture promises (a truncated file must not pass)
  if (fx.shapes.size() < 340 || fx.modes.size() < 41 || fx.ncand < 1000 || fx.ngemm < 9000)
    return fprintf(stderr, "fixture too short\n"), 1;
  return 0;
}

// Exact expectation, formed without any sum that could pass 2^63.
long long ceil_div(long long a, long long b) { return a / b + (a % b != 0); }

void check_wide() {
  const long long two31 = 1LL << 31;
  const long long Ms[] = {two31 - 200, two31 - 127, two31 - 1, two31, two31 + 5, 1LL << 33};
  const int couts[] = {64, 128, 8192, 65536, 1 << 24, INT_MAX - 3};
  std::vector<ConvShape> shapes;
  for (long long M : Ms)
    for (int co : couts)
      for (int wb = 0; wb < 2; ++wb) {
        // a 1x1 GEMM of M rows, one image
        shapes.push_back(ConvShape{M, INT_MAX, 1, INT_MAX, 32, 32, co, 1, 1, 1, 0, 32, wb != 0,
                                   false, false, false});
        // a deep-K one (split-K multiplies the grid)
        shapes.push_back(ConvShape{M, INT_MAX, 1, INT_MAX, 4096, 4096, co, 1, 1, 1, 0, 4096,
                                   wb != 0, false, false, false});
        // 3x3 stride 1 on 32 x 64 images: hw = 2048, M / hw images
        shapes.push_back(ConvShape{M / 2048 * 2048, 2048, 32, 64, 64, 64, co, 3, 3, 1, 1, 576,
                                   wb != 0, false, false, false});
      }
  ConvMode modes[3];
  modes[0].precision = 0;
  modes[2].bm192 = modes[2].rb4n64 = true;
  for (const ConvShape& s : shapes)
    for (const ConvMode& m : modes)
      for (int split = 0; split < 2; ++split)
        for (int forced = -1; forced <= 35; ++forced) {
          const Plan p = conv_plan(s, m, split != 0, forced);
          ++g_checked;
          const std::string tag = "wide M " + std::to_string(s.M) + " Cout " +
                                  std::to_string(s.Cout) + " KH " + std::to_string(s.KH) +
                                  " forced " + std::to_string(forced);
          if (p.kern < 0) {
            fail(tag + ": conv_plan returned an illegal plan");
            continue;
          }
          const long long tm = p.ppi ? s.M / s.hw * p.ppi : ceil_div(s.M, p.bm);
          if (p.tiles_m != tm || p.ksplit < 1) fail(tag + ": tiles_m " + describe(p));
          const TileRow* r = tile_row(p.run_tile);
          const long long rtm = p.ppi ? tm : ceil_div(s.M, r->bm);
          const unsigned __int128 grid =
              (unsigned __int128)rtm * ceil_div(s.Cout, r->bn) * p.ksplit;
          if (grid > INT_MAX) {
            if (p.variant != V_NONE) fail(tag + ": a grid past INT_MAX planned " + describe(p));
          } else if (p.variant == V_NONE || (long long)p.nwg * p.ksplit != (long long)grid ||
                     p.nwg <= 0 || p.tiles_n != ceil_div(s.Cout, r->bn)) {
            fail(tag + ": grid " + describe(p));
          }
        }
}

}  // namespace

int main(int argc, char** argv) {
  if (check_fixture(argc > 1 ? argv[1] : "tests/golden/conv_plans.txt")) return 1;
  check_wide();
  // the table itself: unique ids, every id resolvable, sane rows
  for (const TileRow& r : kTileTable) {
    if (tile_row(r.id) != &r || r.bm <= 0 || r.bn <= 0 || r.threads % 64 ||
        (r.family == FAM_HALO) != (r.ph > 0) || (r.ph && r.bm != r.ph * 16))
      fail(std::string("tile table row ") + r.name);
  }
  if (g_fail) {
    fprintf(stderr, "%d mismatches in %lld checks\n", g_fail, g_checked);
    return 1;
  }
  printf("conv_plan ok (%lld checks)\n", g_checked);
  return 0;
}
