// Peer minima of the joined passes (lp_mp_amd/csrc/order.cpp, kernels.hip dense_pq_*_body), host only:
//   g++ -std=c++17 -O2 -I lp_mp_amd/csrc tests/cpp/peer_minima_probe.cpp lp_mp_amd/csrc/order.cpp -lpthread
// The step records of a 2-colour grid (H, W, K, T as plan.cpp emits them: the fields order.cpp reads) go through the real
// plan_rotation_chain and joined_pass_tables.  Checked: the eligibility rule, and — the hazard proof — that with one more location
// per pairwise factor f, "the published minima of f" (written by the W record that receives-and-sends f, read by the K / T record
// that receives over f), every read-after-write and write-after-read pair is ordered by the emitted dependencies, i.e. the earlier
// ticket is an ancestor of the later one in the dependency graph (then every linear extension, however adversarial, keeps them in
// order).  Band order, tiled order and the periodic template expanded as the kernel expands it; several pass counts.
// Prints "peer minima ok" and exits 0, or names the first failed check and exits 1.
// With arguments, `peer_minima_probe GRAPH bands:lag:depth ...`, the eligibility rule and the hazard proof run on the bipartite
// graph of the file GRAPH instead of the grids ("n0 n1", then an edge "a b" per line, a < n0 of colour 0 and b < n1 of colour 1, in
// the order the model's builder adds them: tests/peer_minima_cases.py), in the given windows.  The tiled order needs equal block
// counts of H, K and T (engine.cpp offers it only then); where they differ it is skipped, and the output says so.
// make_steps emits a record's ops in edge order and the records in vertex order.  plan.cpp lists a factor's messages type by type,
// so on a graph whose records sit on either side of their tables its receives come side 0 first; the slots' writer and reader
// blocks, and with them every check here, depend on which factors a record receives over, not on the order of its ops.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <functional>
#include <string>
#include <vector>

#include "plan.hpp"

using namespace lpmp;

static int failures = 0;
#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d: %s — ", __FILE__, __LINE__, #cond); std::printf(__VA_ARGS__); std::printf("\n"); if (++failures > 20) std::exit(1); } } while (0)

struct Graph {                       // a bipartite graph in a 2-colour order: side[v] = colour, edges (a of colour 0, b of colour 1)
  int n = 0; std::vector<int> side; std::vector<std::pair<int, int>> edges;
};
static Graph grid(int H, int W) {
  Graph g; g.n = H * W; g.side.resize((size_t)g.n);
  for (int r = 0; r < H; ++r) for (int c = 0; c < W; ++c) g.side[r * W + c] = (r + c) & 1;
  auto add = [&](int a, int b) { if (g.side[a]) std::swap(a, b); g.edges.emplace_back(a, b); };
  for (int r = 0; r < H; ++r) for (int c = 0; c < W; ++c) { if (c + 1 < W) add(r * W + c, r * W + c + 1); if (r + 1 < H) add(r * W + c, (r + 1) * W + c); }
  return g;
}
static Graph stars(int arms, int leaves) {
  Graph g; g.n = arms * (leaves + 1); g.side.assign((size_t)g.n, 0);
  for (int a = 0; a < arms; ++a) { const int c = a * (leaves + 1); g.side[c] = 1; for (int i = 1; i <= leaves; ++i) g.edges.emplace_back(c + i, c); }
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
enum Defect { NONE, W_KEEPS_ONE, W_STORES_FIRST };
static Steps make_steps(const Graph& g, int kclass = KC_DENSE_32, Defect defect = NONE) {
  Steps s; s.nf = g.n + (int64_t)g.edges.size();
  std::vector<std::vector<int>> inc((size_t)g.n);
  for (size_t e = 0; e < g.edges.size(); ++e) { inc[g.edges[e].first].push_back((int)e); inc[g.edges[e].second].push_back((int)e); }
  int max_ops = 0;
  for (const auto& v : inc) max_ops = std::max(max_ops, 2 * (int)v.size());
  auto level = [&](Schedule& sc, int lvl, int colour, bool recv, bool send) {
    LevelRange lr{kclass, (int64_t)sc.recs.size(), 0};
    lr.level = lvl; lr.stride = max_ops <= PK_MAX_OPS ? 1 + PK_MAX_OPS : -1;
    bool first = true;
    for (int v = 0; v < g.n; ++v) {
      if (g.side[v] != colour || inc[v].empty()) continue;
      UpdRec r{}; r.factor = v; r.op_begin = (int32_t)sc.ops.size(); r.d0 = 32;
      const int deg = (int)inc[v].size();
      const bool short_send = defect == W_KEEPS_ONE && recv && send && colour == 1 && first && deg > 1;
      if (recv) for (int j = 0; j < deg; ++j) { Op o{}; o.peer = g.n + inc[v][j]; o.pad = send && !(defect == W_STORES_FIRST && colour == 1 && first && j == 0) ? j + 1 : 0; sc.ops.push_back(o); ++lr.n_recv; }
      if (send) for (int j = 0; j < deg - (short_send ? 1 : 0); ++j) { Op o{}; o.peer = g.n + inc[v][j]; o.pad = recv ? j + 1 : 0; sc.ops.push_back(o); ++lr.n_send; }
      r.n_recv = (int16_t)(recv ? deg : 0); r.n_send = (int16_t)(send ? deg - (short_send ? 1 : 0) : 0);
      sc.recs.push_back(r);
      first = false;
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
struct Launch {
  int64_t N = 0; std::vector<int32_t> step, block; std::vector<std::vector<int32_t>> dep;
};
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

static int64_t pairs_checked = 0;
// RAW and WAR pairs on the slot of every pairwise factor, over the 2 n + 1 steps H, W, (K, W)^(n-1), T
static void check_slots(const Steps& s, const RotationInfo& ri, const Launch& l, int n, const char* what) {
  const int ns = 2 * n + 1;
  std::vector<std::vector<int32_t>> ticket((size_t)ns);
  for (int st = 0; st < ns; ++st) ticket[st].assign((size_t)ri.t[st == 0 ? 0 : st == ns - 1 ? 3 : (st & 1) ? 1 : 2].nb, -1);
  for (int64_t t = 0; t < l.N; ++t) {
    CHECK(l.step[t] >= 0 && l.step[t] < ns && l.block[t] >= 0 && l.block[t] < (int32_t)ticket[l.step[t]].size() && ticket[l.step[t]][l.block[t]] < 0, "%s: ticket %lld", what, (long long)t);
    if (failures) return;
    ticket[l.step[t]][l.block[t]] = (int32_t)t;
  }
  // writer / reader blocks of every slot
  std::vector<int32_t> wb((size_t)s.nf, -1), kb((size_t)s.nf, -1), tb((size_t)s.nf, -1);
  auto blocks = [&](const Schedule& sc, const LevelRange& lr, std::vector<int32_t>& out) {
    for (int64_t i = lr.begin; i < lr.end; ++i) for (int q = 0; q < sc.recs[i].n_recv; ++q) out[sc.ops[sc.recs[i].op_begin + q].peer] = (int32_t)((i - lr.begin) / ri.gpb);
  };
  blocks(s.fb, s.w, wb); blocks(s.bf, s.k, kb); blocks(s.fb, s.t, tb);
  // a before b: a is an ancestor of b (dependencies point to lower tickets)
  std::vector<int32_t> mark((size_t)l.N, -1); int32_t stamp = 0;
  auto before = [&](int32_t a, int32_t b) {
    if (a >= b) return false;
    ++stamp;
    std::vector<int32_t> todo{b};
    while (!todo.empty()) {
      const int32_t x = todo.back(); todo.pop_back();
      for (int32_t d : l.dep[x]) { if (d == a) return true; if (d > a && mark[d] != stamp) { mark[d] = stamp; todo.push_back(d); } }
    }
    return false;
  };
  for (int64_t f = 0; f < s.nf; ++f) {
    if (wb[f] < 0) continue;
    CHECK(kb[f] >= 0 && tb[f] >= 0, "%s: slot %lld has a writer and no reader", what, (long long)f);
    for (int st = 1; st < ns - 1 && !failures; st += 2) {
      const bool last = st + 1 == ns - 1;
      const int32_t w = ticket[st][wb[f]], r = ticket[st + 1][last ? tb[f] : kb[f]];
      CHECK(before(w, r), "%s, %d passes: the reader of slot %lld at step %d (ticket %d) is not ordered after its writer (ticket %d)", what, n, (long long)f, st + 1, r, w);
      ++pairs_checked;
      if (!last) {
        const int32_t w2 = ticket[st + 2][wb[f]];
        CHECK(before(r, w2), "%s, %d passes: the next writer of slot %lld at step %d (ticket %d) is not ordered after the reader (ticket %d)", what, n, (long long)f, st + 2, w2, r);
        ++pairs_checked;
      }
    }
  }
}

struct Window { int bands, lag, depth; };
// every window, band order and tiled order, 1 to 32 passes, explicit tables and the periodic template
static void check_windows(const Steps& s, const RotationInfo& ri, const std::vector<Window>& windows, const char* name) {
  const bool tiles_ok = ri.t[0].nb == ri.t[2].nb && ri.t[3].nb == ri.t[2].nb;
  if (!tiles_ok) std::printf("%s: H, K, T have %d, %d, %d blocks: the tiled order is not offered, skipped\n", name, ri.t[0].nb, ri.t[2].nb, ri.t[3].nb);
  const TileSet ts = tiles_ok ? make_tiles(ri, 3) : TileSet();
  for (const Window& wnd : windows) for (int tiled = 0; tiled < (tiles_ok ? 2 : 1); ++tiled) {
    const JoinedOrder ord{wnd.bands, wnd.lag, tiled ? std::max(2, wnd.depth & ~1) : wnd.depth, tiled ? &ts : nullptr};
    for (int n : {1, 2, 3, 5, 7, 9, 12, 20, 32}) {
      JoinedTables jt;
      std::string why = joined_pass_tables(ri, ord, n, false, jt, nullptr);
      CHECK(why.empty(), "%s, %d passes: %s", name, n, why.c_str());
      if (why.empty()) check_slots(s, ri, expand(jt, ord.depth, 0), n, tiled ? "tiled order" : "band order");
      // the periodic template of this pass count's parity, expanded to n passes
      const int depth = ord.depth, tail = (2 * n + 1) % depth, n_tmpl = (3 * depth + tail - 1) / 2;
      if (depth % 2 || n < n_tmpl || n <= 7) continue;
      JoinedTables tp;
      why = joined_pass_tables(ri, ord, n_tmpl, true, tp, nullptr);
      CHECK(why.empty(), "%s, template of %d passes: %s", name, n_tmpl, why.c_str());
      const int extra = (n - n_tmpl) / (depth / 2);
      if (why.empty() && n_tmpl + extra * (depth / 2) == n) check_slots(s, ri, expand(tp, depth, extra), n, tiled ? "periodic, tiled order" : "periodic, band order");
    }
  }
}

// the eligibility rule and the hazard proof on a graph read from a file, in the caller's windows
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
  const RotationInfo ri = plan_rotation_chain(s.fb, s.bf, s.nf);
  CHECK(ri.valid && ri.peer_minima && ri.peer_minima_why.empty(), "%s: '%s'", argv[1], ri.peer_minima_why.c_str());
  if (ri.valid) check_windows(s, ri, windows, argv[1]);
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("peer minima ok (%lld ordered pairs)\n", (long long)pairs_checked);
  return 0;
}

int main(int argc, char** argv) {
  // ---- eligibility
  const std::pair<int, int> grids[] = {{2, 2}, {1, 7}, {3, 3}, {13, 11}, {14, 10}, {40, 36}};
  if (argc > 1 && std::string(argv[1]) != "why") return graph_mode(argc, argv);
  if (argc > 1) {   // the obstacle strings, for the record
    for (int leaves : {4, 5}) { const Steps s = make_steps(stars(3, leaves)); std::printf("stars of %d: '%s'\n", leaves, plan_rotation_chain(s.fb, s.bf, s.nf).peer_minima_why.c_str()); }
    return 0;
  }
  for (const auto& hw : grids) {
    const Steps s = make_steps(grid(hw.first, hw.second));
    const RotationInfo ri = plan_rotation_chain(s.fb, s.bf, s.nf);
    CHECK(ri.valid && ri.peer_minima && ri.peer_minima_why.empty(), "%d x %d grid: '%s'", hw.first, hw.second, ri.peer_minima_why.c_str());
  }
  {
    Steps s = make_steps(stars(3, 4));
    CHECK(plan_rotation_chain(s.fb, s.bf, s.nf).peer_minima, "stars of 4 leaves");
    s = make_steps(stars(3, 5));                                   // a colour-1 node of degree 5: indirect records, more than 4 receives
    RotationInfo ri = plan_rotation_chain(s.fb, s.bf, s.nf);
    CHECK(ri.valid && !ri.peer_minima && !ri.peer_minima_why.empty(), "stars of 5 leaves");
    s = make_steps(grid(6, 5), KC_DENSE_16);
    ri = plan_rotation_chain(s.fb, s.bf, s.nf);
    CHECK(ri.valid && !ri.peer_minima, "16 labels");
    s = make_steps(grid(6, 5), KC_DENSE_V32);
    CHECK(!plan_rotation_chain(s.fb, s.bf, s.nf).peer_minima, "run-time dims");
    s = make_steps(grid(6, 5), KC_DENSE_32, W_KEEPS_ONE);
    CHECK(!plan_rotation_chain(s.fb, s.bf, s.nf).peer_minima, "a W record that does not send over an edge it receives from");
    s = make_steps(grid(6, 5), KC_DENSE_32, W_STORES_FIRST);
    CHECK(!plan_rotation_chain(s.fb, s.bf, s.nf).peer_minima, "a W receive that is stored, not forwarded");
  }
  // ---- hazards of the slots
  const std::vector<Window> windows = {{8, 2, 4}, {5, 1, 2}, {16, 2, 3}, {3, 4, 7}};
  for (const auto& hw : grids) {
    const Steps s = make_steps(grid(hw.first, hw.second));
    const RotationInfo ri = plan_rotation_chain(s.fb, s.bf, s.nf);
    if (!ri.valid) continue;
    check_windows(s, ri, windows, (std::to_string(hw.first) + " x " + std::to_string(hw.second)).c_str());
  }
  if (failures) { std::printf("%d checks failed\n", failures); return 1; }
  std::printf("peer minima ok (%lld ordered pairs)\n", (long long)pairs_checked);
  return 0;
}
