// Wide consume blocks of the joined passes (lp_mp_amd/csrc/order.cpp plan_rotation_chain with consume_gpb; kernels.hip
// dense_pq_consume_body on 32-lane groups), host only:
//   g++ -std=c++17 -O2 -I lp_mp_amd/csrc tests/cpp/wide_consume_probe.cpp lp_mp_amd/csrc/order.cpp -lpthread
// The step records of 2-colour grids (H, W, K, T as plan.cpp emits them: the fields order.cpp reads) go through the real
// plan_rotation_chain with H / K / T blocks of 8 records beside W blocks of 4, and then through joined_pass_tables: band order and
// tiled order, forced windows, 1 to 32 passes, the periodic template expanded as the kernel expands it.  Checked on every launch:
//   * every block of every step has exactly one ticket;
//   * every dependency points to a lower ticket;
//   * the slot hazards of peer_minima_probe.cpp, the K / T blocks computed with the consume block size;
//   * for EVERY factor, unary and pairwise: any two consecutive touches in step order (a record that updates it or reaches it
//     through an op) by different tickets are ordered by ancestry in the dependency graph.  Blocks of neighbouring steps no longer
//     have the same size, so this is checked on what was emitted, not argued.
// And: with the parameter left out, 0, or the class's own block size the function returns the same value field for field, and
// that value's block counts and predecessor lists are those of an independent statement of their definition.
// Prints "wide consume ok" and exits 0, or names the first failed checks and exits 1.
// With arguments, `wide_consume_probe GRAPH bands:lag:depth ...`, the same launch checks run on the bipartite graph of the file GRAPH
// instead of the grids ("n0 n1", then an edge "a b" per line, a < n0 of colour 0 and b < n1 of colour 1, in the order the model's
// builder adds them: tests/peer_minima_cases.py), in the given windows, with consume blocks of 4 and of 8 records.  The tiled order
// needs equal block counts of H, K and T (engine.cpp offers it only then); where they differ it is skipped, and the output says so.
// make_steps emits a record's ops in edge order and the records in vertex order.  plan.cpp lists a factor's messages type by type,
// so on a graph whose records sit on either side of their tables its receives come side 0 first; the blocks, and with them every
// check here, depend on which factors a record reaches, not on the order of its ops.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>
#include <vector>

#include "plan.hpp"

using namespace lpmp;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d: %s — ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); if (++failures > 20) std::exit(1); } } while (0)

struct Graph { int n = 0; std::vector<int> side; std::vector<std::pair<int, int>> edges; };   // edges (a of colour 0, b of colour 1)
static Graph grid(int H, int W) {
  Graph g; g.n = H * W; g.side.resize((size_t)g.n);
  for (int r = 0; r < H; ++r) for (int c = 0; c < W; ++c) g.side[r * W + c] = (r + c) & 1;
  auto add = [&](int a, int b) { if (g.side[a]) std::swap(a, b); g.edges.emplace_back(a, b); };
  for (int r = 0; r < H; ++r) for (int c = 0; c < W; ++c) { if (c + 1 < W) add(r * W + c, r * W + c + 1); if (r + 1 < H) add(r * W + c, (r + 1) * W + c); }
  return g;
}

static bool read_graph(const char* path, Graph& g) {
  std::ifstream in(path);
  long long n0 = 0, n1 = 0, a = 0, b = 0;
  if (!(in >> n0 >> n1) || n0 < 0 || n1 < 0 || n0 + n1 > (1 << 24)) return false;
  g.n = (int)(n0 + n1); g.side.assign((size_t)g.n, 0);
  for (long long v = n0; v < n0 + n1; ++v) g.side[(size_t)v] = 1;
  while (in >> a >> b) { if (a < 0 || a >= n0 || b < 0 || b >= n1) return false; g.edges.emplace_back((int)a, (int)(n0 + b)); }
  return in.eof();
}

// forward+backward (levels H, W, T) and backward+forward (level K) of that graph: unary v = factor v, edge e = factor n + e
struct Steps { Schedule fb, bf; LevelRange h, w, k, t; int64_t nf = 0; };
static Steps make_steps(const Graph& g) {
  Steps s; s.nf = g.n + (int64_t)g.edges.size();
  std::vector<std::vector<int>> inc((size_t)g.n);
  for (size_t e = 0; e < g.edges.size(); ++e) { inc[g.edges[e].first].push_back((int)e); inc[g.edges[e].second].push_back((int)e); }
  auto level = [&](Schedule& sc, int lvl, int colour, bool recv, bool send) {
    LevelRange lr{KC_DENSE_32, (int64_t)sc.recs.size(), 0};
    lr.level = lvl; lr.stride = 1 + PK_MAX_OPS;
    for (int v = 0; v < g.n; ++v) {
      if (g.side[v] != colour || inc[v].empty()) continue;
      UpdRec r{}; r.factor = v; r.op_begin = (int32_t)sc.ops.size(); r.d0 = 32;
      const int deg = (int)inc[v].size();
      if (recv) for (int j = 0; j < deg; ++j) { Op o{}; o.peer = g.n + inc[v][j]; o.pad = send ? j + 1 : 0; sc.ops.push_back(o); ++lr.n_recv; }
      if (send) for (int j = 0; j < deg; ++j) { Op o{}; o.peer = g.n + inc[v][j]; o.pad = recv ? j + 1 : 0; sc.ops.push_back(o); ++lr.n_send; }
      r.n_recv = (int16_t)(recv ? deg : 0); r.n_send = (int16_t)(send ? deg : 0);
      sc.recs.push_back(r);
    }
    lr.end = (int64_t)sc.recs.size(); lr.bytes = (lr.end - lr.begin) * 40000;
    sc.launches.push_back(lr);
    return lr;
  };
  s.h = level(s.fb, 1, 0, false, true);
  s.w = level(s.fb, 2, 1, true, true);
  s.t = level(s.fb, 3, 0, true, false);
  level(s.bf, 1, 1, false, true);
  s.k = level(s.bf, 2, 0, true, true);
  level(s.bf, 3, 1, true, false);
  s.fb.n_levels = s.bf.n_levels = 3;
  return s;
}

// the tickets of a launch of n passes as the kernel sees them: explicit tables, or a periodic template expanded (chain_ticket_ref)
struct Launch { int64_t N = 0; std::vector<int32_t> step, block; std::vector<std::vector<int32_t>> dep; };
static Launch expand(const JoinedTables& jt, int depth, int extra) {
  Launch l;
  l.N = (int64_t)jt.tk_launch.size() + (int64_t)extra * jt.per_len;
  l.step.resize((size_t)l.N); l.block.resize((size_t)l.N); l.dep.resize((size_t)l.N);
  for (int64_t t = 0; t < l.N; ++t) {
    const int64_t q = jt.per_len == 0 || t < jt.per_begin ? 0 : std::min<int64_t>((t - jt.per_begin) / jt.per_len, extra);
    const int64_t i = t - q * jt.per_len;
    l.step[t] = jt.tk_launch[i] + (int32_t)(q * depth); l.block[t] = jt.tk_block[i];
    for (int32_t k = jt.dep_off[i]; k < jt.dep_off[i + 1]; ++k) l.dep[t].push_back((int32_t)(jt.dep[k] + q * jt.per_len));
  }
  return l;
}

static int tmpl_of(int st, int ns) { return st == 0 ? 0 : st == ns - 1 ? 3 : (st & 1) ? 1 : 2; }
static int gpb_of(const RotationInfo& ri, int tmpl) { return tmpl == 1 ? ri.gpb : ri.consume_gpb; }

static int64_t pairs_checked = 0, launches_checked = 0;
static void check_launch(const Steps& s, const RotationInfo& ri, const Launch& l, int n, const char* what) {
  ++launches_checked;
  const int ns = 2 * n + 1;
  // ---- every block exactly one ticket, every dependency backwards
  std::vector<std::vector<int32_t>> ticket((size_t)ns);
  int64_t blocks = 0;
  for (int st = 0; st < ns; ++st) { ticket[st].assign((size_t)ri.t[tmpl_of(st, ns)].nb, -1); blocks += ri.t[tmpl_of(st, ns)].nb; }
  CHECK(l.N == blocks, "%s, %d passes: %lld tickets for %lld blocks", what, n, (long long)l.N, (long long)blocks);
  for (int64_t t = 0; t < l.N; ++t) {
    CHECK(l.step[t] >= 0 && l.step[t] < ns && l.block[t] >= 0 && l.block[t] < (int32_t)ticket[l.step[t]].size() && ticket[l.step[t]][l.block[t]] < 0,
          "%s, %d passes: ticket %lld is no block or a block's second ticket", what, n, (long long)t);
    if (failures) return;
    ticket[l.step[t]][l.block[t]] = (int32_t)t;
    for (int32_t d : l.dep[t]) CHECK(d >= 0 && d < t, "%s, %d passes: ticket %lld depends on ticket %d", what, n, (long long)t, d);
  }
  for (int st = 0; st < ns; ++st) for (int32_t t : ticket[st]) CHECK(t >= 0, "%s, %d passes: a block of step %d has no ticket", what, n, st);
  if (failures) return;
  // a before b: a is an ancestor of b (dependencies point to lower tickets)
  std::vector<int32_t> mark((size_t)l.N, -1); int32_t stamp = 0;
  std::vector<int32_t> todo;
  auto before = [&](int32_t a, int32_t b) {
    if (a >= b) return false;
    ++stamp;
    todo.assign(1, b);
    while (!todo.empty()) {
      const int32_t x = todo.back(); todo.pop_back();
      for (int32_t d : l.dep[x]) { if (d == a) return true; if (d > a && mark[d] != stamp) { mark[d] = stamp; todo.push_back(d); } }
    }
    return false;
  };
  // ---- who touches a factor in a step of each template: the block of the record that updates it or reaches it through an op
  const LevelRange* lrs[4] = {&s.h, &s.w, &s.k, &s.t};
  const Schedule* sch[4] = {&s.fb, &s.fb, &s.bf, &s.fb};
  std::vector<int32_t> touch[4], recv_of[4];
  for (int i = 0; i < 4; ++i) {
    touch[i].assign((size_t)s.nf, -1); recv_of[i].assign((size_t)s.nf, -1);
    const int g = gpb_of(ri, i);
    for (int64_t r = lrs[i]->begin; r < lrs[i]->end; ++r) {
      const UpdRec& rec = sch[i]->recs[r];
      const int32_t b = (int32_t)((r - lrs[i]->begin) / g);
      CHECK(touch[i][rec.factor] < 0, "two records of one step update factor %d", rec.factor);
      touch[i][rec.factor] = b;
      for (int q = 0; q < rec.n_recv + rec.n_send; ++q) {
        const int32_t f = sch[i]->ops[rec.op_begin + q].peer;
        CHECK(touch[i][f] < 0 || touch[i][f] == b, "two blocks of one step reach factor %d", f);
        touch[i][f] = b;
        if (q < rec.n_recv) recv_of[i][f] = b;
      }
    }
  }
  // ---- slot hazards: the published minima of f, written by the W block that receives f, read by the K / T block that receives f
  for (int64_t f = 0; f < s.nf; ++f) {
    if (recv_of[1][f] < 0) continue;
    CHECK(recv_of[2][f] >= 0 && recv_of[3][f] >= 0, "%s: slot %lld has a writer and no reader", what, (long long)f);
    for (int st = 1; st < ns - 1 && !failures; st += 2) {
      const bool last = st + 1 == ns - 1;
      const int32_t w = ticket[st][recv_of[1][f]], r = ticket[st + 1][recv_of[last ? 3 : 2][f]];
      CHECK(before(w, r), "%s, %d passes: the reader of slot %lld at step %d (ticket %d) is not ordered after its writer (ticket %d)", what, n, (long long)f, st + 1, r, w);
      ++pairs_checked;
      if (!last) {
        const int32_t w2 = ticket[st + 2][recv_of[1][f]];
        CHECK(before(r, w2), "%s, %d passes: the next writer of slot %lld at step %d (ticket %d) is not ordered after the reader (ticket %d)", what, n, (long long)f, st + 2, w2, r);
        ++pairs_checked;
      }
    }
  }
  // ---- every factor: consecutive touches by different tickets
  for (int64_t f = 0; f < s.nf && !failures; ++f) {
    int32_t prev = -1; int prev_st = -1;
    for (int st = 0; st < ns; ++st) {
      const int32_t b = touch[tmpl_of(st, ns)][f];
      if (b < 0) continue;
      const int32_t t = ticket[st][b];
      if (prev >= 0 && prev != t) {
        CHECK(before(prev, t), "%s, %d passes: factor %lld is touched at step %d (ticket %d) and at step %d (ticket %d), and the two are not ordered", what, n,
              (long long)f, prev_st, prev, st, t);
        ++pairs_checked;
      }
      prev = t; prev_st = st;
    }
  }
}

static bool same(const RotationInfo& a, const RotationInfo& b) {
  bool eq = a.valid == b.valid && a.kclass == b.kclass && a.gpb == b.gpb && a.consume_gpb == b.consume_gpb && a.hist_ok == b.hist_ok && a.reach == b.reach &&
            a.peer_minima == b.peer_minima && a.peer_minima_why == b.peer_minima_why;
  for (int i = 0; i < 4; ++i)
    eq = eq && a.t[i].sched == b.t[i].sched && a.t[i].nb == b.t[i].nb && a.t[i].factors == b.t[i].factors && a.t[i].recv == b.t[i].recv && a.t[i].bytes == b.t[i].bytes &&
         a.t[i].lr.begin == b.t[i].lr.begin && a.t[i].lr.end == b.t[i].lr.end && a.t[i].lr.kclass == b.t[i].lr.kclass && a.t[i].lr.level == b.t[i].lr.level &&
         a.t[i].lr.stride == b.t[i].lr.stride;
  for (int k = 0; k < 6; ++k) eq = eq && a.off[k] == b.off[k] && a.delta[k] == b.delta[k] && a.block[k] == b.block[k];
  return eq;
}

// block counts and predecessor lists from their definition (plan.hpp RotationInfo), every template in blocks of g[tmpl] records
static void check_definition(const Steps& s, const RotationInfo& ri, const int (&g)[4], const char* what) {
  const LevelRange* lrs[4] = {&s.h, &s.w, &s.k, &s.t};
  const Schedule* sch[4] = {&s.fb, &s.fb, &s.bf, &s.fb};
  std::vector<int32_t> touch[4];
  for (int i = 0; i < 4; ++i) {
    const int64_t cnt = lrs[i]->end - lrs[i]->begin;
    CHECK(ri.t[i].nb == (cnt + g[i] - 1) / g[i] && ri.t[i].factors == cnt, "%s: template %d has %d blocks for %lld records", what, i, ri.t[i].nb, (long long)cnt);
    touch[i].assign((size_t)s.nf, -1);
    for (int64_t r = lrs[i]->begin; r < lrs[i]->end; ++r) {
      const UpdRec& rec = sch[i]->recs[r];
      touch[i][rec.factor] = (int32_t)((r - lrs[i]->begin) / g[i]);
      for (int q = 0; q < rec.n_recv + rec.n_send; ++q) touch[i][sch[i]->ops[rec.op_begin + q].peer] = (int32_t)((r - lrs[i]->begin) / g[i]);
    }
  }
  const int X[6] = {1, 2, 1, 2, 3, 3}, Y1[6] = {0, 1, 2, 1, 1, 1}, Y2[6] = {-1, 0, 1, 2, 2, 0};
  for (int kind = 0; kind < 6; ++kind) {
    const int x = X[kind];
    CHECK((int64_t)ri.off[kind].size() == ri.t[x].nb + 1, "%s: kind %d", what, kind);
    if (failures) return;
    for (int32_t b = 0; b < ri.t[x].nb; ++b) {
      std::vector<std::pair<int, int32_t>> want, got;
      for (int64_t r = lrs[x]->begin + (int64_t)b * g[x]; r < std::min<int64_t>(lrs[x]->end, lrs[x]->begin + (int64_t)(b + 1) * g[x]); ++r) {
        const UpdRec& rec = sch[x]->recs[r];
        std::vector<int32_t> fs{rec.factor};
        for (int q = 0; q < rec.n_recv + rec.n_send; ++q) fs.push_back(sch[x]->ops[rec.op_begin + q].peer);
        for (int32_t f : fs) {
          if (touch[Y1[kind]][f] >= 0) want.emplace_back(1, touch[Y1[kind]][f]);
          else if (Y2[kind] >= 0 && touch[Y2[kind]][f] >= 0) want.emplace_back(2, touch[Y2[kind]][f]);
        }
      }
      std::sort(want.begin(), want.end()); want.erase(std::unique(want.begin(), want.end()), want.end());
      for (int64_t q = ri.off[kind][b]; q < ri.off[kind][b + 1]; ++q) got.emplace_back((int)ri.delta[kind][q], ri.block[kind][q]);
      CHECK(want == got, "%s: predecessors of block %d, kind %d", what, b, kind);
    }
  }
}

struct Window { int bands, lag, depth; };
// every window, band order and tiled order, 1 to 32 passes, explicit tables and the periodic template
static void check_launches(const Steps& s, const RotationInfo& ri, const std::vector<Window>& windows, const char* name) {
  const bool tiles_ok = ri.t[0].nb == ri.t[2].nb && ri.t[3].nb == ri.t[2].nb;
  if (!tiles_ok) std::printf("%s: H, K, T have %d, %d, %d blocks: the tiled order is not offered, skipped\n", name, ri.t[0].nb, ri.t[2].nb, ri.t[3].nb);
  const TileSet ts = tiles_ok ? make_tiles(ri, 3) : TileSet();
  for (const Window& wnd : windows) for (int tiled = 0; tiled < (tiles_ok ? 2 : 1); ++tiled) {
    const JoinedOrder ord{wnd.bands, wnd.lag, tiled ? std::max(2, wnd.depth & ~1) : wnd.depth, tiled ? &ts : nullptr};
    for (int n : {1, 2, 3, 5, 7, 9, 12, 20, 32}) {
      JoinedTables jt;
      std::string why = joined_pass_tables(ri, ord, n, false, jt, nullptr);
      CHECK(why.empty(), "%s, %d passes: %s", name, n, why.c_str());
      if (why.empty()) check_launch(s, ri, expand(jt, ord.depth, 0), n, tiled ? "tiled order" : "band order");
      // the periodic template of this pass count's parity, expanded to n passes
      const int depth = ord.depth, tail = (2 * n + 1) % depth, n_tmpl = (3 * depth + tail - 1) / 2;
      if (depth % 2 || n < n_tmpl || n <= 7) continue;
      JoinedTables tp;
      why = joined_pass_tables(ri, ord, n_tmpl, true, tp, nullptr);
      CHECK(why.empty(), "%s, template of %d passes: %s", name, n_tmpl, why.c_str());
      const int extra = (n - n_tmpl) / (depth / 2);
      if (why.empty() && n_tmpl + extra * (depth / 2) == n) check_launch(s, ri, expand(tp, depth, extra), n, tiled ? "periodic, tiled order" : "periodic, band order");
    }
  }
}

// the launch checks on a graph read from a file, in the caller's windows, consume blocks of 4 and of 8 records
static int graph_mode(int argc, char** argv) {
  Graph g;
  if (!read_graph(argv[1], g)) { std::printf("%s: not a graph file\n", argv[1]); return 2; }
  std::vector<Window> windows;
  for (int i = 2; i < argc; ++i) {
    Window w{};
    if (std::sscanf(argv[i], "%d:%d:%d", &w.bands, &w.lag, &w.depth) != 3 || w.bands < 1 || w.lag < 1 || w.depth < 1) { std::printf("%s: not bands:lag:depth\n", argv[i]); return 2; }
    windows.push_back(w);
  }
  if (windows.empty()) { std::printf("no window given\n"); return 2; }
  const Steps s = make_steps(g);
  for (int consume : {0, PQ_WIDE_RECORDS}) {
    const RotationInfo ri = plan_rotation_chain(s.fb, s.bf, s.nf, consume);
    const std::string name = std::string(argv[1]) + (consume ? ", consume blocks of 8" : ", consume blocks of 4");
    CHECK(ri.valid && ri.peer_minima && ri.peer_minima_why.empty(), "%s: '%s'", name.c_str(), ri.peer_minima_why.c_str());
    if (!ri.valid) continue;
    CHECK(ri.gpb == 4 && ri.consume_gpb == (consume ? PQ_WIDE_RECORDS : 4), "%s: blocks of %d and %d records", name.c_str(), ri.gpb, ri.consume_gpb);
    const int g4[4] = {4, 4, 4, 4}, g8[4] = {8, 4, 8, 8};
    check_definition(s, ri, consume ? g8 : g4, name.c_str());
    check_launches(s, ri, windows, name.c_str());
  }
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("wide consume ok (%lld launches, %lld ordered pairs)\n", (long long)launches_checked, (long long)pairs_checked);
  return 0;
}

int main(int argc, char** argv) {
  if (argc > 1) return graph_mode(argc, argv);
  // ---- the default is what it was
  for (const auto& hw : {std::pair<int, int>{13, 11}, std::pair<int, int>{40, 36}}) {
    const Steps s = make_steps(grid(hw.first, hw.second));
    const RotationInfo a = plan_rotation_chain(s.fb, s.bf, s.nf), b = plan_rotation_chain(s.fb, s.bf, s.nf, 0),
                       c = plan_rotation_chain(s.fb, s.bf, s.nf, kc_block_records(KC_DENSE_32));
    CHECK(a.valid && a.gpb == 4 && a.consume_gpb == 4, "%d x %d: blocks of %d and %d records", hw.first, hw.second, a.gpb, a.consume_gpb);
    CHECK(same(a, b) && same(a, c), "%d x %d: the default differs from consume blocks of the class's own size", hw.first, hw.second);
    check_definition(s, a, {4, 4, 4, 4}, "default");
    const RotationInfo w = plan_rotation_chain(s.fb, s.bf, s.nf, PQ_WIDE_RECORDS);
    CHECK(w.valid && w.gpb == 4 && w.consume_gpb == 8 && w.peer_minima == a.peer_minima && w.hist_ok == a.hist_ok, "%d x %d: wide", hw.first, hw.second);
    check_definition(s, w, {8, 4, 8, 8}, "wide");
  }
  // ---- the launches
  const std::pair<int, int> grids[] = {{2, 2}, {1, 7}, {3, 3}, {13, 11}, {14, 10}, {40, 36}, {37, 41}};
  const std::vector<Window> windows = {{8, 2, 4}, {5, 1, 2}, {16, 2, 3}, {3, 4, 7}};
  for (const auto& hw : grids) {
    const Steps s = make_steps(grid(hw.first, hw.second));
    const RotationInfo ri = plan_rotation_chain(s.fb, s.bf, s.nf, PQ_WIDE_RECORDS);
    const std::string name = std::to_string(hw.first) + " x " + std::to_string(hw.second);
    CHECK(ri.valid && ri.peer_minima, "%s grid: '%s'", name.c_str(), ri.peer_minima_why.c_str());
    if (!ri.valid) continue;
    CHECK(ri.t[0].nb == ri.t[2].nb && ri.t[3].nb == ri.t[2].nb, "%s: H, K, T block counts %d, %d, %d", name.c_str(), ri.t[0].nb, ri.t[2].nb, ri.t[3].nb);
    check_launches(s, ri, windows, name.c_str());
  }
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("wide consume ok (%lld launches, %lld ordered pairs)\n", (long long)launches_checked, (long long)pairs_checked);
  return 0;
}
