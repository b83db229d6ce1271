// tests/cpp/move_plans_sanitize.cpp — the planners of the prepared sets (Plan::path_plan, Plan::forest_plan, Plan::window_plan) as a
// stand-alone host program for sanitizer runs on the CPU.  From lp_mp_amd/csrc:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -I . -o move_plans \
//       ../../tests/cpp/move_plans_sanitize.cpp plan.cpp chain_plan.cpp order.cpp -lpthread && ./move_plans
// Exit status 0 and no sanitizer report is the pass.
//
// The model: a grid of 4 rows of 5 unaries (unary r * 5 + c, 6 labels each) with a DIFF_SHIFT factor on each of its 16 horizontal
// and 15 vertical edges, so 31 pairwise factors and 62 messages; a unary has as many links as grid neighbours.  What is printed,
// and checked against these figures:
//   paths    the rows as paths, groups {row 0, row 2} and {row 1, row 3} (the rows of a group are not adjacent, so no factor joins
//            two paths of a group): 4 paths, a row of 5 has 4 edges: n_path_edges 16, longest 5; every vertical edge is a cost
//            line at both of its ends: n_off_path_links 2 * 15 = 30
//   forests  group 0, a comb: row 0 as the spine, rooted at unary 0, with teeth down the columns 0, 2 and 4 (14 members that induce
//            a tree: 4 + 3 * 3 = 13 edges; the deepest member, unary 19, is 4 + 3 = 7 below the root).  Its members have 13 (row
//            0) + 8 + 11 + 8 (the teeth) = 40 links, 26 of them along the 13 tree edges: 14 off the tree.
//            group 1, two trees: the rows 1 and 3, each a chain rooted in column 0 (8 edges, height 4; 18 + 13 = 31 links, 16 of
//            them along tree edges: 15 off the trees).
//            Together: n_trees 3, n_tree_edges 21, n_off_tree_links 29, max_height 7
//   windows  every unary: 62 links, 31 pairs.  The list {0, 1, 6}: 2 + 3 + 4 = 9 links; unary 0 meets 2 factors, unary 1 two more
//            (it shares one with unary 0), unary 6 three more (it shares one with unary 1): 7 pairs
// Then one refusal of each kind: a unary twice in a group, a cycle of parents, a ring as a path, a factor out of range.
#include "plan.hpp"
#include <cstdio>
#include <functional>
using namespace lpmp;
static int bad = 0;
static void expect(const char* what, int64_t got, int64_t want) {
  std::printf("%s %lld\n", what, (long long)got);
  if (got != want) { std::printf("  ... expected %lld\n", (long long)want); ++bad; }
}
static void refused(const char* what, const std::function<void()>& f) {
  try { f(); std::printf("%s: accepted?\n", what); ++bad; } catch (const std::runtime_error& ex) { std::printf("refused: %s\n", ex.what()); }
}
int main() {
  const int H = 4, W = 5, L = 6, n = H * W;
  std::vector<int32_t> ei, ej;
  for (int r = 0; r < H; ++r) for (int c = 0; c < W; ++c) { if (c + 1 < W) { ei.push_back(r * W + c); ej.push_back(r * W + c + 1); } if (r + 1 < H) { ei.push_back(r * W + c); ej.push_back((r + 1) * W + c); } }
  const int E = (int)ei.size(), nf = n + E;
  std::vector<int32_t> f_type(nf), d0(nf, L), d1(nf, 0), f_table(nf, -1), m_type, m_left, m_right, rel;
  std::vector<uint8_t> kind(nf, LPMP_F_VECTOR), flags(nf, 0);
  std::vector<double> cst;
  for (int e = 0; e < E; ++e) { const int f = n + e; f_type[f] = 1; kind[f] = LPMP_F_PAIRWISE_DIFF_SHIFT; d1[f] = L; f_table[f] = 0;
    cst.push_back(1.5); cst.push_back(L - 1);      // {scale, shift}: the windows of both unaries start at the same label
    m_type.push_back(0); m_left.push_back(ei[e]); m_right.push_back(f); m_type.push_back(1); m_left.push_back(ej[e]); m_right.push_back(f);
    rel.push_back(ei[e]); rel.push_back(f); rel.push_back(f); rel.push_back(ej[e]); }
  std::vector<double> dual((size_t)n * L + (size_t)E * 2 * L, 0.25), pool(2 * L - 1);
  for (int k = 0; k < 2 * L - 1; ++k) pool[k] = std::min(0.05 * std::abs(k - (L - 1)), 0.2);
  lpmp_msg_type mt[2] = {{0, 1, LPMP_SCHED_LEFT, 0, 1, LPMP_M_UNARY_PAIRWISE, 0, 0}, {0, 1, LPMP_SCHED_LEFT, 0, 1, LPMP_M_UNARY_PAIRWISE, 1, 0}};
  const int64_t sh_off[2] = {0, 2 * L - 1}; const int32_t sd0[1] = {1}, sd1[1] = {2 * L - 1};
  lpmp_model m{};
  m.n_ftypes = 2; m.n_mtypes = 2; m.mtypes = mt; m.n_factors = nf; m.f_type = f_type.data(); m.f_kind = kind.data(); m.f_flags = flags.data();
  m.f_dim0 = d0.data(); m.f_dim1 = d1.data(); m.const_data = cst.data(); m.dual_data = dual.data();
  m.n_messages = (int64_t)m_type.size(); m.m_type = m_type.data(); m.m_left = m_left.data(); m.m_right = m_right.data();
  m.n_rel_fwd = (int64_t)rel.size() / 2; m.rel_fwd = rel.data();
  m.n_shared_tables = 1; m.sh_off = sh_off; m.sh_dim0 = sd0; m.sh_dim1 = sd1; m.sh_data = pool.data(); m.f_table = f_table.data();
  Plan p; p.build(m);
  auto row = [&](int r) { std::vector<int32_t> v; for (int c = 0; c < W; ++c) v.push_back(r * W + c); return v; };

  // ---- paths: the rows, groups {0, 2} and {1, 3}
  {
    std::vector<int32_t> un; std::vector<int64_t> go = {0, 2, 4}, po = {0};
    for (int r : {0, 2, 1, 3}) { for (int32_t u : row(r)) un.push_back(u); po.push_back((int64_t)un.size()); }
    const PathPlan pp = p.path_plan(2, go.data(), po.data(), un.data(), "path_plan");
    if (!pp.why.empty()) { std::printf("paths refused: %s\n", pp.why.c_str()); return 1; }
    expect("n_paths", (int64_t)pp.path_off.size() - 1, 4);
    expect("n_path_edges", pp.n_path_edges, 16);
    expect("n_off_path_links", pp.n_off_path_links, 30);
    expect("longest", pp.longest, 5);
  }
  // ---- forests: the comb, then the rows 1 and 3
  {
    std::vector<int32_t> un, par;
    for (int c = 0; c < W; ++c) { un.push_back(c); par.push_back(c ? c - 1 : -1); }
    for (int c : {0, 2, 4}) for (int r = 1; r < H; ++r) { un.push_back(r * W + c); par.push_back((r - 1) * W + c); }
    std::vector<int64_t> go = {0, (int64_t)un.size()};
    for (int r : {1, 3}) for (int c = 0; c < W; ++c) { un.push_back(r * W + c); par.push_back(c ? r * W + c - 1 : -1); }
    go.push_back((int64_t)un.size());
    const ForestPlan fp = p.forest_plan(2, go.data(), un.data(), par.data(), "forest_plan");
    if (!fp.why.empty()) { std::printf("forests refused: %s\n", fp.why.c_str()); return 1; }
    expect("n_trees", fp.n_trees, 3);
    expect("n_tree_edges", fp.n_tree_edges, 21);
    expect("n_off_tree_links", fp.n_off_tree_links, 29);
    expect("max_height", fp.max_height, 7);
  }
  // ---- windows: every unary, then a list of three
  {
    const WindowPlan all = p.window_plan(0, nullptr, "window_plan");
    if (!all.why.empty()) { std::printf("windows refused: %s\n", all.why.c_str()); return 1; }
    expect("window links (all)", (int64_t)all.links.size(), 62);
    expect("window pairs (all)", (int64_t)all.pairs.size(), 31);
    const int32_t three[3] = {0, 1, W + 1};
    const WindowPlan w3 = p.window_plan(3, three, "window_plan");
    if (!w3.why.empty()) { std::printf("windows refused: %s\n", w3.why.c_str()); return 1; }
    expect("window links (three)", (int64_t)w3.links.size(), 9);
    expect("window pairs (three)", (int64_t)w3.pairs.size(), 7);
  }
  // ---- the refusals
  refused("a unary twice in a group", [&] {
    std::vector<int32_t> un = row(0); for (int32_t u : row(0)) un.push_back(u);
    const int64_t go[2] = {0, 2}, po[3] = {0, W, 2 * W};
    p.path_plan(1, go, po, un.data(), "path_plan");
  });
  refused("a cycle of parents", [&] {
    const int32_t un[3] = {0, 1, 2}, par[3] = {1, 2, 0}; const int64_t go[2] = {0, 3};
    p.forest_plan(1, go, un, par, "forest_plan");
  });
  refused("a ring as a path", [&] {
    const int32_t un[4] = {0, 1, W + 1, W}; const int64_t go[2] = {0, 1}, po[2] = {0, 4};
    p.path_plan(1, go, po, un, "path_plan");
  });
  refused("a factor out of range", [&] {
    const int32_t un[2] = {0, nf};
    p.window_plan(2, un, "window_plan");
  });
  return bad ? 1 : 0;
}
