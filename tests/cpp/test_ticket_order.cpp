// Ticket orders of the joined-pass launch (lp_mp_amd/csrc/order.cpp) on synthetic block relations, host only:
//   g++ -std=c++17 -O2 -I lp_mp_amd/csrc tests/cpp/test_ticket_order.cpp lp_mp_amd/csrc/order.cpp -lpthread
// Prints "ticket orders ok" and exits 0, or names the first failed check and exits 1.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <string>
#include <tuple>
#include <vector>

#include "plan.hpp"

using namespace lpmp;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d: %s — ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); if (++failures > 20) std::exit(1); } } while (0)

// All four steps of nb blocks; a block's predecessors in the step before lie at the offsets `offs` (a 2-D grid in a 2-colour
// order: -row, -1, 0, +1, +row), the one two steps before (where the kind has one) is the same block.
static RotationInfo synthetic(int64_t nb, const std::vector<int64_t>& offs) {
  RotationInfo ri;
  ri.valid = true; ri.kclass = KC_DENSE_32; ri.gpb = 4; ri.hist_ok = true;
  for (int i = 0; i < 4; ++i) {
    ri.t[i].sched = i == 2 ? 1 : 0;
    ri.t[i].lr = LevelRange{KC_DENSE_32, 0, nb * 4};
    ri.t[i].nb = (int32_t)nb; ri.t[i].factors = nb * 4; ri.t[i].recv = nb * 8; ri.t[i].bytes = nb * 160000;
  }
  int64_t r = 0;
  for (int64_t o : offs) r = std::max(r, o);
  ri.reach = (double)r / (double)nb;
  for (int kind = 0; kind < 6; ++kind) {
    ri.off[kind].assign(1, 0);
    for (int64_t j = 0; j < nb; ++j) {
      std::vector<std::pair<int8_t, int32_t>> p;
      for (int64_t o : offs) if (j + o >= 0 && j + o < nb) p.emplace_back((int8_t)1, (int32_t)(j + o));
      if (kind != 0) p.emplace_back((int8_t)2, (int32_t)j);
      std::sort(p.begin(), p.end());
      p.erase(std::unique(p.begin(), p.end()), p.end());
      for (const auto& d : p) { ri.delta[kind].push_back(d.first); ri.block[kind].push_back(d.second); }
      ri.off[kind].push_back((int64_t)ri.block[kind].size());
    }
  }
  return ri;
}
static std::vector<int64_t> grid_offsets(int64_t row) { return {-row, -1, 0, 1, row}; }
static std::vector<int64_t> grid3d_offsets(int64_t row) { return {-row * row, -row, -1, 0, 1, row, row * row}; }

// the steps of n joined passes, stated independently of order.cpp: H, W, (K, W)^(n-1), T and their predecessor kinds
static void steps(int n, std::vector<int>& tmpl, std::vector<int>& kind) {
  const int ns = 2 * n + 1;
  tmpl.assign(ns, 0); kind.assign(ns, -1);
  for (int s = 1; s < ns; ++s) {
    tmpl[s] = s == ns - 1 ? 3 : s % 2 == 1 ? 1 : 2;
    kind[s] = s == ns - 1 ? (n == 1 ? 5 : 4) : s == 1 ? 0 : s == 2 ? 1 : s % 2 == 1 ? 2 : 3;
  }
}

// explicit tables of n passes: every block once, every dependency the one of RotationInfo, every one earlier, the rows of the bounds
static bool check_tables(const RotationInfo& ri, int n, const JoinedTables& jt, const char* what) {
  const int before = failures;
  std::vector<int> tmpl, kind;
  steps(n, tmpl, kind);
  const int ns = 2 * n + 1;
  CHECK(jt.step_tmpl == tmpl, "%s: step templates", what);
  for (int s = 0; s < ns && (int)jt.step_row.size() == ns; ++s) {
    const int want = tmpl[s] == 1 && (s - 1) / 2 < n - 1 ? (s - 1) / 2 : tmpl[s] == 2 ? (s - 2) / 2 : -1;
    CHECK(jt.step_row[s] == want, "%s: bound row of step %d", what, s);
  }
  std::vector<std::vector<int32_t>> ticket(ns);
  for (int s = 0; s < ns; ++s) ticket[s].assign((size_t)ri.t[tmpl[s]].nb, -1);
  const int64_t N = (int64_t)jt.tk_launch.size();
  CHECK((int64_t)jt.tk_block.size() == N && (int64_t)jt.dep_off.size() == N + 1, "%s: table sizes", what);
  if (failures > before) return false;
  for (int64_t t = 0; t < N; ++t) {
    const int s = jt.tk_launch[t];
    const int32_t j = jt.tk_block[t];
    CHECK(s >= 0 && s < ns && j >= 0 && j < ri.t[tmpl[s]].nb && ticket[s][j] < 0, "%s: ticket %lld is not a new block", what, (long long)t);
    if (failures > before) return false;
    ticket[s][j] = (int32_t)t;
  }
  for (int s = 0; s < ns; ++s) for (int32_t t : ticket[s]) CHECK(t >= 0, "%s: a block of step %d has no ticket", what, s);
  for (int64_t t = 0; t < N && failures == before; ++t) {
    const int s = jt.tk_launch[t], kd = kind[s];
    const int32_t j = jt.tk_block[t];
    std::vector<int32_t> want, got(jt.dep.begin() + jt.dep_off[t], jt.dep.begin() + jt.dep_off[t + 1]);
    if (kd >= 0)
      for (int64_t q = ri.off[kd][j]; q < ri.off[kd][j + 1]; ++q) want.push_back(ticket[s - ri.delta[kd][q]][ri.block[kd][q]]);
    std::sort(want.begin(), want.end()); std::sort(got.begin(), got.end());
    CHECK(got == want, "%s: dependencies of ticket %lld", what, (long long)t);
    for (int32_t d : got) CHECK(d < t, "%s: ticket %lld depends on the later ticket %d", what, (long long)t, d);
  }
  return failures == before;
}

// the periodic template expanded to n passes as the kernel expands it (kernels.hip chain_ticket_ref: tickets past the prologue map
// onto the period, shifted by whole copies; a copy is depth steps further) must be the explicit tables of n passes
static void check_periodic(const RotationInfo& ri, const JoinedOrder& ord, int n) {
  const int depth = ord.depth, tail = (2 * n + 1) % depth, n_tmpl = (3 * depth + tail - 1) / 2;
  if (n < n_tmpl) return;
  JoinedTables tp, ex;
  std::string why = joined_pass_tables(ri, ord, n_tmpl, true, tp, nullptr);
  CHECK(why.empty(), "template of %d passes, depth %d: %s", n, depth, why.c_str());
  why = joined_pass_tables(ri, ord, n, false, ex, nullptr);
  CHECK(why.empty(), "%d passes, depth %d: %s", n, depth, why.c_str());
  if (failures) return;
  const int extra = (n - n_tmpl) / (depth / 2);
  CHECK(n_tmpl + extra * (depth / 2) == n, "pass count %d does not fit the template of %d (depth %d)", n, n_tmpl, depth);
  CHECK(tp.ring == 3 * tp.per_len && tp.per_len > 0, "ring of the template (depth %d)", depth);
  const int64_t N = (int64_t)tp.tk_launch.size() + (int64_t)extra * tp.per_len;
  CHECK(N == (int64_t)ex.tk_launch.size(), "%d passes: %lld tickets expanded, %zu explicit", n, (long long)N, ex.tk_launch.size());
  for (int64_t t = 0; t < N && !failures; ++t) {
    const int64_t q = t < tp.per_begin ? 0 : std::min<int64_t>((t - tp.per_begin) / tp.per_len, extra);
    const int64_t i = t - q * tp.per_len;
    CHECK(tp.tk_launch[i] + q * depth == ex.tk_launch[t] && tp.tk_block[i] == ex.tk_block[t], "%d passes, depth %d: ticket %lld", n, depth, (long long)t);
    std::vector<int64_t> a, b;
    for (int32_t k = tp.dep_off[i]; k < tp.dep_off[i + 1]; ++k) a.push_back(tp.dep[k] + q * tp.per_len);
    for (int32_t k = ex.dep_off[t]; k < ex.dep_off[t + 1]; ++k) b.push_back(ex.dep[k]);
    CHECK(a == b, "%d passes, depth %d: dependencies of ticket %lld", n, depth, (long long)t);
    // a dependency reaches at most one group back: the ring of three groups never hands out a slot still in use
    for (int64_t d : a) CHECK(t - d < tp.ring, "%d passes: ticket %lld waits on %lld, a ring or more back", n, (long long)t, (long long)d);
  }
}

int main() {
  std::mt19937 rng(7);
  // ---- band order: a permutation; inside a group the sort statement (band + lag * d, d, block), band = floor(j * bands / nb)
  int64_t cases = 0;
  for (int it = 0; it < 400; ++it) {
    const int n_steps = 1 + (int)(rng() % 9), bands = 1 + (int)(rng() % 64), lag = 1 + (int)(rng() % 16), depth = 1 + (int)(rng() % 10);
    std::vector<int64_t> nb(n_steps), base(n_steps + 1, 0);
    for (int s = 0; s < n_steps; ++s) { nb[s] = 1 + rng() % 300; base[s + 1] = base[s] + nb[s]; }
    TicketOrder o;
    band_order(nb, bands, lag, depth, o);
    std::vector<std::tuple<int64_t, int, int64_t, int64_t>> want;     // (group, band + lag * d, d, block) per (step, block) in step order
    for (int s = 0; s < n_steps; ++s)
      for (int64_t j = 0; j < nb[s]; ++j) want.emplace_back(s / depth, j * bands / nb[s] + (int64_t)lag * (s % depth), s % depth, j);
    std::vector<int64_t> idx(want.size());
    for (size_t i = 0; i < idx.size(); ++i) idx[i] = (int64_t)i;
    std::sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) { return want[a] < want[b]; });
    CHECK((int64_t)o.tk_step.size() == base[n_steps] && o.group_begin.back() == base[n_steps], "band order: ticket count");
    for (size_t t = 0; t < idx.size() && !failures; ++t) {
      const int s = (int)(std::upper_bound(base.begin(), base.end(), idx[t]) - base.begin()) - 1;
      CHECK(o.tk_step[t] == s && o.tk_block[t] == idx[t] - base[s] && o.new_of[idx[t]] == (int32_t)t,
            "band order (%d steps, %d bands, lag %d, depth %d): ticket %zu", n_steps, bands, lag, depth, t);
    }
    CHECK((int)o.group_begin.size() == (n_steps + depth - 1) / depth + 1, "band order: groups");
    for (size_t g = 0; g + 1 < o.group_begin.size(); ++g)
      CHECK(o.group_begin[g] == base[std::min<int64_t>(n_steps, (int64_t)g * depth)], "band order: start of group %zu", g);
    ++cases;
  }

  // ---- lag: with one block per band, predecessors r blocks ahead need lag >= r; the search of the builder goes up to max(16, 2 lag)
  for (int64_t r : {2, 5, 12, 20}) {
    const RotationInfo ri = synthetic(24 * r, grid_offsets(r));
    for (int n : {1, 2, 3}) {
      JoinedTables jt;
      JoinedOrder ord{(int)(24 * r), (int)r - 1, 4, nullptr};
      TicketOrder o;
      std::vector<int64_t> nb(2 * n + 1, 24 * r);
      band_order(nb, ord.bands, (int)r - 1, 4, o);
      bool forward = false;                                 // the order of lag r - 1 itself puts a predecessor behind its dependant
      for (int64_t j = 0; j + r < 24 * r; ++j) forward = forward || o.new_of[1 * 24 * r + j + r] > o.new_of[2 * 24 * r + j];
      CHECK(forward, "lag %lld below the reach %lld keeps the dependencies", (long long)(r - 1), (long long)r);
      std::string why = joined_pass_tables(ri, ord, n, false, jt, nullptr);
      CHECK(why.empty() && jt.lag == r, "reach %lld from lag %lld: '%s', lag %d", (long long)r, (long long)(r - 1), why.c_str(), jt.lag);
      if (why.empty()) check_tables(ri, n, jt, "band order");
      if (r > 16) {                                         // a search from 3 to 16 finds nothing
        ord.lag = 3;
        why = joined_pass_tables(ri, ord, n, false, jt, nullptr);
        CHECK(why == "no band order keeps the dependencies backwards", "reach %lld refused from lag 3: '%s'", (long long)r, why.c_str());
      }
      ++cases;
    }
  }

  // ---- band orders of the builder on fewer bands than blocks, every depth and pass count
  for (int64_t row : {4, 16}) {
    const RotationInfo ri = synthetic(row * 12, grid_offsets(row));
    for (int bands : {1, 3, 12, 48}) for (int depth = 1; depth <= 8; ++depth) for (int n : {1, 2, 3, 6}) {
      JoinedTables jt;
      const std::string why = joined_pass_tables(ri, JoinedOrder{bands, 1, depth, nullptr}, n, false, jt, nullptr);
      CHECK(why.empty(), "band order, %d bands, depth %d, %d passes: %s", bands, depth, n, why.c_str());
      if (why.empty()) check_tables(ri, n, jt, "band order");
      ++cases;
    }
  }

  // ---- tiled order: valid by construction, for every tile size and depth
  for (const auto& g : {std::make_pair(synthetic(24 * 16, grid_offsets(24)), "2-D"), std::make_pair(synthetic(8 * 8 * 8, grid3d_offsets(8)), "3-D")}) {
    for (int T : {1, 3, 8, 20, 1024}) {
      const TileSet ts = make_tiles(g.first, T);
      CHECK(ts.T == T && ts.n > 0 && ts.depth >= 2 && ts.depth <= 8 && ts.depth % 2 == 0, "%s tiles of %d: %d tiles, depth %d", g.second, T, ts.n, ts.depth);
      for (int32_t x : ts.w) CHECK(x >= 0 && x < ts.n, "%s: a W block without a tile", g.second);
      for (int32_t x : ts.k) CHECK(x >= 0 && x < ts.n, "%s: a K block without a tile", g.second);
      for (int depth = 2; depth <= 8; ++depth) for (int n : {1, 2, 4, 7}) {
        JoinedTables jt;
        const std::string why = joined_pass_tables(g.first, JoinedOrder{1, 3, depth, &ts}, n, false, jt, nullptr);
        CHECK(why.empty() && jt.lag == 3, "%s tiles of %d, depth %d, %d passes: %s", g.second, T, depth, n, why.c_str());
        if (why.empty()) check_tables(g.first, n, jt, "tiled order");
        ++cases;
      }
    }
  }

  // ---- periodic templates: n = 8 ... 40 of both parities, band and tiled order, even depths
  {
    const RotationInfo ri = synthetic(16 * 10, grid_offsets(16));
    const TileSet ts = make_tiles(ri, 20);
    for (int depth = 2; depth <= 8; depth += 2)
      for (int n = 8; n <= 40; ++n) {
        check_periodic(ri, JoinedOrder{10, 16, depth, nullptr}, n);
        check_periodic(ri, JoinedOrder{1, 3, depth, &ts}, n);
        cases += 2;
      }
  }

  // ---- the window: no step to measure keeps the defaults (no division by a zero step size)
  {
    RotationInfo ri = synthetic(64, grid_offsets(8));
    ri.t[1].bytes = 0;
    const RotGeometry g = rot_geometry(RotSettings(), ri);
    CHECK(g.bands == 1 && g.lag == 3 && g.depth == 4 && g.fits, "zero step bytes: %d bands, lag %d, depth %d", g.bands, g.lag, g.depth);
    ri.t[1].bytes = (int64_t)1 << 30; ri.t[1].nb = 0;
    const RotGeometry h = rot_geometry(RotSettings(), ri);
    CHECK(h.bands == 1 && h.lag == 3 && h.depth == 4 && h.fits, "no blocks: %d bands, lag %d, depth %d", h.bands, h.lag, h.depth);
  }

  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("ticket orders ok (%lld cases)\n", (long long)cases);
  return 0;
}
