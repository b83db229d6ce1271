// tests/cpp/pool_swap_sanitize.cpp — the planner's pool swap (Plan::set_shared_pool, Plan::refresh_diff_band) as a stand-alone host
// program for sanitizer runs on the CPU: the plan of a 7 x 6 x 40 DIFF grid with two vectors, its pool swapped between banded and
// unbanded vectors a few times, then the two refusals.  From lp_mp_amd/csrc:
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-omit-frame-pointer -I . -o pool_swap \
//       ../../tests/cpp/pool_swap_sanitize.cpp plan.cpp chain_plan.cpp order.cpp -lpthread && ./pool_swap
// Exit status 0 and no sanitizer report is the pass; the launch counts it prints are those tests/test_repool_host.py asserts on.
#include "plan.hpp"
#include <cstdio>
#include <cmath>
using namespace lpmp;
static std::vector<double> tl(int L, double slope, double trunc) {
  std::vector<double> d(2 * L - 1);
  for (int k = 0; k < 2 * L - 1; ++k) d[k] = std::min(slope * std::fabs((double)k - (L - 1)), trunc);
  return d;
}
int main() {
  const int H = 7, W = 6, L = 40, n = H * W;
  std::vector<int32_t> ei, ej;
  for (int r = 0; r < H; ++r) for (int c = 0; c < W; ++c) { if (c + 1 < W) { ei.push_back(r * W + c); ej.push_back(r * W + c + 1); } if (r + 1 < H) { ei.push_back(r * W + c); ej.push_back((r + 1) * W + c); } }
  const int E = (int)ei.size(), nf = n + E;
  std::vector<int32_t> f_type(nf), d0(nf, L), d1(nf, 0), f_table(nf, -1), m_type, m_left, m_right, rel;
  std::vector<uint8_t> kind(nf, LPMP_F_VECTOR), flags(nf, 0);
  for (int e = 0; e < E; ++e) { const int f = n + e; f_type[f] = 1; kind[f] = LPMP_F_PAIRWISE_DIFF; d1[f] = L; f_table[f] = e % 2;
    m_type.push_back(0); m_left.push_back(ei[e]); m_right.push_back(f); m_type.push_back(1); m_left.push_back(ej[e]); m_right.push_back(f);
    rel.push_back(ei[e]); rel.push_back(f); rel.push_back(f); rel.push_back(ej[e]); }
  std::vector<double> cst(E, 1.5), dual((size_t)n * L + (size_t)E * 2 * L, 0.25);
  lpmp_msg_type mt[2] = {{0, 1, LPMP_SCHED_LEFT, 0, 1, LPMP_M_UNARY_PAIRWISE, 0, 0}, {0, 1, LPMP_SCHED_LEFT, 0, 1, LPMP_M_UNARY_PAIRWISE, 1, 0}};
  std::vector<double> pool;
  for (auto v : {tl(L, 0.05, 0.2), tl(L, 0.05, 0.2)}) pool.insert(pool.end(), v.begin(), v.end());
  const int64_t sh_off[3] = {0, 2 * L - 1, 2 * (2 * L - 1)}; const int32_t sd0[2] = {1, 1}, sd1[2] = {2 * L - 1, 2 * L - 1};
  lpmp_model m{};
  m.n_ftypes = 2; m.n_mtypes = 2; m.mtypes = mt; m.n_factors = nf; m.f_type = f_type.data(); m.f_kind = kind.data(); m.f_flags = flags.data();
  m.f_dim0 = d0.data(); m.f_dim1 = d1.data(); m.const_data = cst.data(); m.dual_data = dual.data();
  m.n_messages = (int64_t)m_type.size(); m.m_type = m_type.data(); m.m_left = m_left.data(); m.m_right = m_right.data();
  m.n_rel_fwd = (int64_t)rel.size() / 2; m.rel_fwd = rel.data();
  m.n_shared_tables = 2; m.sh_off = sh_off; m.sh_dim0 = sd0; m.sh_dim1 = sd1; m.sh_data = pool.data(); m.f_table = f_table.data();
  Plan p; p.build(m);
  Schedule s[2];
  for (int d = 0; d < 2; ++d) { p.ensure_weights(0); p.make_schedule(p.upd[d].data(), (int64_t)p.upd[d].size(), p.omega[d][0].off.data(), p.omega[d][0].data.data(), p.mask[d][0].off.data(), p.mask[d][0].data.data(), s[d]); }
  auto count = [&](const char* what) { for (int d = 0; d < 2; ++d) { int nd = 0, nb = 0; for (auto& lr : s[d].launches) if (lr.kclass == KC_DIFF) { ++nd; nb += lr.diff_band; } std::printf("%s: sweep %d: %d launches of class diff, %d banded\n", what, d, nd, nb); } };
  count("built");
  const std::vector<std::vector<double>> pools = {tl(L, 0.01, 0.2), tl(L, 0.1, 0.25), tl(L, 0.05, 0.2)};
  for (int it = 0; it < 6; ++it) {
    std::vector<double> np;
    for (int t = 0; t < 2; ++t) { const auto& v = pools[(size_t)(it + t) % 3]; np.insert(np.end(), v.begin(), v.end()); }
    p.set_shared_pool(np.data());
    for (int d = 0; d < 2; ++d) p.refresh_diff_band(s[d].launches, s[d].diff_tab_off, s[d].diff_tab);
    count("swapped");
  }
  std::vector<double> bad = pool; bad[5] = std::nan("");
  try { p.set_shared_pool(bad.data()); std::printf("NaN accepted?\n"); return 1; } catch (const std::exception& ex) { std::printf("refused: %s\n", ex.what()); }
  try { p.set_shared_pool(nullptr); return 1; } catch (const std::exception& ex) { std::printf("refused: %s\n", ex.what()); }
  count("after the refusals");
  return 0;
}
